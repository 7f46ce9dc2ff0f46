"""Columns 11 to 13 of the device's feature rows (kmer_score / pos_score of pjb_features.hip.h, behind pjb_filt_features and
pjb_filt_scores) against what the reference's own lib/src/markov_model.cc scored (tests/golden/markov, made by
tests/golden/make_markov_fixture.py, whose docstring lists the cases), composed in the reference's order of operations.  The small
genomes are uploaded as they are, soft-masked and with their IUPAC letters; the rows are built by hand from the fixture's junctions on
contigs 0 and 1 (the 70 kb contig matters to training, which is the host's work); the dense tables come from the oracle, which
tests/test_oracle_markov_witness.py pins to the same witness.  A model the witness left empty is passed as None.

The rule is that of test_gpu_filt_features.py, 1e-6 * max(1, |x|); rows whose every term is exact on any machine (windows of 5 bases
or fewer, sums of -300, the zeros of an empty position model) are bit-equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import forest_util as fu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_markov_fixture as fx  # noqa: E402  (genomes, junctions, windows; it touches nothing on import)

pytestmark = pytest.mark.gpu

WITNESS = {c["name"]: c for c in fx.load_cases()}
BY_NAME = {c["name"]: c for c in fx.CASES}
MRL = 100.0
BLOCK = 256                                     # rows per block of kg_features


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi as f
    assert f.device_count() >= 1
    return f


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def genomes():
    return fx.genomes()


@pytest.fixture(scope="module")
def ctx(ffi, genomes):
    with ffi.Context(0, "UNKNOWN") as c:
        c.set_refs([len(genomes[0]), len(genomes[1])])
        for tid in (0, 1):
            c.upload_contig(tid, genomes[tid].encode())
        yield c


@pytest.fixture(scope="module")
def setups(ffi, orc, genomes):
    """name -> (device rows, models for the device, wanted columns [rows, 3], which of them are exact); made once, never changed"""
    out = {}
    for case in fx.CASES:
        w, bits = WITNESS[case["name"]], fx.load_bits(case["name"])
        idx = fx.case_rows(case)
        _, M, _ = orc.filt_features([len(g) for g in genomes], dict(enumerate(genomes)), fx.junction_rows(orc.ROW_DTYPE, idx), [], case["cp"], case["passing"], case["failing"])
        models = {name: (M[name] if w["trained"][k] else None) for k, name in enumerate(fx.MODEL_NAMES)}
        models.update({k: M[k] for k in ("exon_size", "intron_size", "donor_pw_size", "acceptor_pw_size")})
        on_device = np.array([fx.JUNCTIONS[k][0] in (0, 1) for k in idx])
        want = fx.compose(case, bits, w["trained"], genomes)[on_device]
        rows = fx.junction_rows(ffi.ROW_DTYPE, [k for k in idx if fx.JUNCTIONS[k][0] in (0, 1)])
        out[case["name"]] = (rows, models, want, fx.exact_rows(bits)[on_device])
    return out


def ulps(a, b):
    """the largest distance in representable doubles between a and b (same sign or zero, finite)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2**63) - i, i)
    return int(np.abs(key(a) - key(b)).max())


@pytest.mark.parametrize("name", list(BY_NAME))
def test_columns_match_the_witness(ffi, ctx, setups, name):
    rows, models, want, exact = setups[name]
    tables = [models[m] is not None for m in fx.MODEL_NAMES]
    if name in ("one_pass", "fail_only", "intron_gated", "short6"):
        assert any(tables) and not all(tables)                 # a mixed set: some models trained, some None
    if name == "all":
        assert all(tables) and exact.any() and not exact.all() and (want[:, 1] == -600.0).any() and (np.abs(want) > 1).any()
    F = ctx.filt_features(rows, MRL, 0, models)
    got = np.ascontiguousarray(F[:, 11:14])
    worst = fx.assert_columns(got, want, exact, 1e-6)
    print(f"markov witness {name}: {len(rows)} rows, worst |device - witness| = {worst:.3e}, {ulps(got, want)} ulp")


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_block_edges(ffi, ctx, setups, n):
    """The rows repeated to the edges of kg_features' block: every copy is the first one, and nothing lands behind row n."""
    base, models, want, exact = setups["all"]
    rows = np.resize(base, n)
    m, keep = ctx._markov_models(models)
    guard = np.float64(-12345.678)
    out = np.full((n + 4, ffi.N_FEATURES), guard)
    ctx._check(ctx._L.pjb_filt_features(ctx._h, rows.ctypes.data_as(C.c_void_p), n, MRL, 0, C.byref(m), out.ctypes.data_as(C.c_void_p)))
    assert (out[n:] == guard).all()
    first = ctx.filt_features(base, MRL, 0, models)
    k = np.arange(n) % len(base)
    assert (out[:n].view(np.uint64) == first[k].view(np.uint64)).all()
    fx.assert_columns(np.ascontiguousarray(out[:n, 11:14]), want[k], exact[k], 1e-6)


@pytest.mark.parametrize("name", ["all", "fail_only"])
def test_fused_call_gives_the_same_rows(ffi, ctx, setups, name):
    rows, models, want, exact = setups[name]
    forest, _, _ = fu.witness()
    ctx.forest_load(forest)
    F = ctx.filt_features(rows, MRL, 0, models)
    _, F2 = ctx.filt_scores(rows, MRL, 0, models, fu.ACTIVE_FEATURES, want_features=True)
    assert F2.shape == F.shape and (F2.view(np.uint64) == F.view(np.uint64)).all()
    fx.assert_columns(np.ascontiguousarray(F2[:, 11:14]), want, exact, 1e-6)
