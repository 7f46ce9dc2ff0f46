"""`portcullis_amd filt --self_train` end to end on the generated 640-junction table (tests/golden/make_selftrain_sets_fixture.py) over
tests/golden/spombe_III_30k.fa, once in the SMOTE shape (rule set lenient: twice as many positives as negatives), once in the under-sampling
shape (rule set strict: more negatives than positives) and once with --enn.  Every link is checked on its own, without a tolerance: the set
files against the reference's own script (selftrain_sets.json), the training matrix's rows and labels against the sets, its synthetic rows
against the Python restatement of Smote::execute (pinned by test_host_selftrain.py) over ctx.knn of the file's own negative rows, the forest
against ctx.forest_grow of the file's matrix, what passes against ctx.forest_predict of the testing matrix, the rows ENN keeps against the
restated mask.  One link has a tolerance, test_gpu_filt_features.py's: the feature columns against ctx.filt_features with the Markov models
the oracle trains on the same sets."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forest_util as fu
from test_gpu_filt_cli import rows_of
from util_bam import PREP_FA, read_fasta, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_knn_fixture as kx  # noqa: E402  (restatements; they touch nothing on import)
import make_selftrain_sets_fixture as sx  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
SETS = sx.load_sets()["rulesets"]
TREES = 250  # DEFAULT_SELFTRAIN_TREES


def read_tab(path):
    lines = [l.split("\t") for l in open(path).read().split("\n") if l]
    return lines[0], lines[1:]


def keys_of(path):
    h, rows = read_tab(path)
    return [sx.key(h, r) for r in rows]


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi as f
    assert f.device_count() >= 1
    return f


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("selftrain")
    (name, seq), = read_fasta(os.path.join(ROOT, "tests", "golden", "spombe_III_30k.fa"))   # (seq: bytes)
    assert (name, len(seq)) == (sx.GENOME_NAME, sx.GENOME_LEN)
    prep = d / "prep"
    prep.mkdir()
    write_fasta(str(prep / PREP_FA), [(name, seq)])
    header, rows = sx.selftrain_table()
    tab = d / "in.junctions.tab"
    tab.write_text(sx.table_text(header, rows))
    return dict(dir=d, prep=str(prep), tab=str(tab), header=header, rows=rows, genome=seq, by_key={tuple(sx.key(header, r)): k for k, r in enumerate(rows)})


@pytest.fixture(scope="module")
def ctx(ffi, world):
    with ffi.Context(0, "UNKNOWN") as c:
        c.set_refs([sx.GENOME_LEN])
        c.upload_contig(0, world["genome"])
        yield c


@pytest.fixture(scope="module")
def runs(world):
    """name -> output prefix of one run of the program; each is made once"""
    done = {}

    def run(name, ruleset, *opts):
        if name not in done:
            out = str(world["dir"] / name / "pc")
            env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
            p = subprocess.run([EXE, "filt", "--self_train", sx.DATA, "--training_rule", ruleset, "--save_matrix", "--save_features", "--save_bad", *opts,
                                "-o", out, world["prep"], world["tab"]], capture_output=True, text=True, timeout=300, env=env)
            assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
            done[name] = (out, p.stdout)
        return done[name]
    return run


def real_rows(world, ruleset, neg_kept=None):
    """(table rows of sorted(pos + neg2), their labels): one target, so JunctionSystem::sort is (start, end) order -- the table's own"""
    pos = [world["by_key"][tuple(k)] for k in SETS[ruleset]["pos"]]
    neg = sorted(world["by_key"][tuple(k)] for k in SETS[ruleset]["neg"])
    if neg_kept is not None:
        neg = [neg[i] for i in neg_kept]
    order = sorted(pos + neg)
    return order, np.array([1.0 if k in set(pos) else 0.0 for k in order])


def check_sets(out, ruleset):
    assert keys_of(out + ".selftrain.initialset.pos.junctions.tab") == SETS[ruleset]["pos"]
    assert keys_of(out + ".selftrain.initialset.neg.junctions.tab") == SETS[ruleset]["neg"]
    assert open(out + ".selftrain.initialset.L95_intron_size.txt").read() == f"Length of intron at 95th percentile\n{SETS[ruleset]['L95']}\n"


def check_forest_and_partition(ffi, ctx, world, out, M):
    grown = ctx.forest_grow(M, n_trees=TREES)
    assert open(out + ".selftrain.forest", "rb").read() == grown.to_bytes()
    T = np.fromfile(out + ".testing.matrix.f64", dtype="<f8").reshape(-1, 29)
    assert len(T) == len(world["rows"])
    ctx.forest_load(grown)
    passes = 1.0 - ctx.forest_predict(T)[:, 0] >= 0.5
    assert 0 < passes.sum() < len(T)
    all_keys = [sx.key(world["header"], r) for r in world["rows"]]
    assert keys_of(out + ".pass.junctions.tab") == [k for k, p in zip(all_keys, passes) if p]
    assert keys_of(out + ".fail.junctions.tab") == [k for k, p in zip(all_keys, passes) if not p]
    return T


def compare_active(F, G):
    """test_gpu_filt_features.py's _compare over the active columns but the label: its integer-valued columns exact, the others to 1e-6"""
    exact = [0, 1, 2, 3, 6, 7, 10]
    for j, a in enumerate(fu.ACTIVE_FEATURES[1:]):
        f, g = F[:, j], G[:, j]
        assert (np.isnan(f) == np.isnan(g)).all() and (np.isinf(f) == np.isinf(g)).all(), a
        fin = np.isfinite(g)
        assert (f[~fin & ~np.isnan(g)] == g[~fin & ~np.isnan(g)]).all(), a
        if a in exact:
            assert (f[fin] == g[fin]).all(), a
        else:
            assert (np.abs(f[fin] - g[fin]) <= 1e-6 * np.maximum(1.0, np.abs(g[fin]))).all(), (a, float(np.abs(f[fin] - g[fin]).max()))


def check_features(ffi, ctx, world, ruleset, order, M, T):
    """the feature columns against ctx.filt_features with the models the oracle trains on the same sets and the script's L95"""
    from oracle import oracle as orc
    drows = rows_of(ffi, world["header"], world["rows"])
    pos = [world["by_key"][tuple(k)] for k in SETS[ruleset]["pos"]]
    neg = [world["by_key"][tuple(k)] for k in SETS[ruleset]["neg"]]
    orows = np.zeros(len(drows), dtype=orc.ROW_DTYPE)   # the oracle's row is wider than the device's: field by field
    for name in set(orc.ROW_DTYPE.names) & set(ffi.ROW_DTYPE.names):
        orows[name] = drows[name]
    _, models, _ = orc.filt_features([sx.GENOME_LEN], {0: world["genome"]}, orows, pos, pos, pos, neg)
    F = ctx.filt_features(drows, float(world["rows"][0][world["header"].index("mean_readlen")]), SETS[ruleset]["L95"], models)
    A = F[:, fu.ACTIVE_FEATURES]
    compare_active(T[:, 1:], A[:, 1:])                       # every junction as scored
    compare_active(M[: len(order), 1:], A[order][:, 1:])     # the real rows of the training matrix


def test_smote_shape(ffi, ctx, world, runs):
    out, stdout = runs("lenient", "lenient")
    check_sets(out, "lenient")
    n_pos, n_neg = len(SETS["lenient"]["pos"]), len(SETS["lenient"]["neg"])
    N = n_pos // n_neg - 1
    assert N >= 1 and "Oversampling negative set to balance with positive set using SMOTE" in stdout
    M = np.fromfile(out + ".selftrain.matrix.f64", dtype="<f8").reshape(-1, 29)
    order, labels = real_rows(world, "lenient")
    assert len(M) == len(order) + N * n_neg
    assert np.array_equal(M[: len(order), 0], labels) and (M[len(order):, 0] == 0.0).all()
    # the synthetic rows: Smote::execute over the file's own negative rows and the device's neighbour lists
    negatives = np.ascontiguousarray(M[: len(order)][labels == 0.0][:, 1:])
    nn = ctx.knn(negatives, 5)
    assert np.array_equal(kx.smote(negatives, nn, N).view(np.uint64), np.ascontiguousarray(M[len(order):, 1:]).view(np.uint64))
    T = check_forest_and_partition(ffi, ctx, world, out, M)
    check_features(ffi, ctx, world, "lenient", order, M, T)
    # --save_features: the real rows, the label in front, at the stream's six digits
    fh, frows = read_tab(out + ".selftrain.features")
    assert fh == ["refid", "refname", "reflen", "start", "end"] + [ffi.FEATURE_NAMES[k] for k in fu.ACTIVE_FEATURES] and len(frows) == len(order)
    for fr, k, m in zip(frows, order, M):
        assert [fr[1], int(fr[3]), int(fr[4])] == sx.key(world["header"], world["rows"][k])[:3] and fr[5:] == ["%g" % v for v in m]


def test_undersampling_shape(ffi, ctx, world, runs):
    out, stdout = runs("strict", "strict")
    check_sets(out, "strict")
    n_pos, n_neg = len(SETS["strict"]["pos"]), len(SETS["strict"]["neg"])
    assert n_neg > n_pos and "Undersampling negative set to balance with positive set" in stdout
    kept, _ = kx.undersample(n_neg, n_pos)             # (pinned against the reference's own lines by test_host_selftrain.py)
    order, labels = real_rows(world, "strict", kept)
    M = np.fromfile(out + ".selftrain.matrix.f64", dtype="<f8").reshape(-1, 29)
    assert len(M) == len(order) == 2 * n_pos and np.array_equal(M[:, 0], labels)
    T = check_forest_and_partition(ffi, ctx, world, out, M)
    check_features(ffi, ctx, world, "strict", order, M, T)


def test_enn_keeps_the_rows_of_the_mask(ffi, ctx, world, runs):
    plain, _ = runs("lenient", "lenient")
    out, stdout = runs("lenient_enn", "lenient", "--enn")
    check_sets(out, "lenient")
    M0 = np.fromfile(plain + ".selftrain.matrix.f64", dtype="<f8").reshape(-1, 29)
    keep = kx.enn_keep(ctx.knn(np.ascontiguousarray(M0[:, 1:]), 3), M0[:, 0] == 1.0)   # over the whole matrix, synthetic rows included
    assert 0 < keep.sum() < len(M0), "ENN must discard some rows and keep some"
    M = np.fromfile(out + ".selftrain.matrix.f64", dtype="<f8").reshape(-1, 29)
    assert M.shape == (int(keep.sum()), 29) and np.array_equal(M.view(np.uint64), np.ascontiguousarray(M0[keep == 1]).view(np.uint64))
    assert f"Marked {int(keep.sum())} to be kept and {int((keep == 0).sum())} to be discarded." in stdout
    check_forest_and_partition(ffi, ctx, world, out, M)
