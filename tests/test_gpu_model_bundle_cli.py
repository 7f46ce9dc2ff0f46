"""The Markov model file through the programs, on the 640-junction table of test_gpu_selftrain_cli.py (rule set lenient):
`filt --self_train --save_models` writes <out>.selftrain.models, `filt --model_file --models_file` scores with it and gives the self-training
run's own tables byte for byte, `train --markov` trains the same models from the run's initial sets and grows its forest on rows that carry
them, and `full --save_models` leaves the file the chained commands leave.  Tables are compared bit for bit (f64 viewed as u64)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import forest_util as fu
from test_gpu_filt_cli import rows_of
from test_gpu_full_cli import DATA as FULL_DATA, RULES as FULL_RULES, make_input
from test_gpu_selftrain_cli import SETS, ctx, ffi, keys_of, read_tab, real_rows, world  # noqa: F401  (ctx, ffi, world: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_selftrain_sets_fixture as sx  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
RULESET = "lenient"
TABLES = ("exon", "intron", "donor_t", "donor_f", "acceptor_t", "acceptor_f", "donor_pw", "acceptor_pw")
KMER_TABLE, PW_TABLE, HEADER_BYTES = 3125 * 5, 32 * 5, 8 + 3 * 4 + 8 * 4
MODEL_COLUMNS = ("rna_intron", "dna_pws", "dna_ss")   # of the four model columns (9, 11 to 13) the ones a features table holds: dna_coding is not active


def run(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    p = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    return p


def read_bundle(path):
    """the file as a models dict (what ctx.filt_features takes) with L95; ModelBundle::check's conditions are asserted on the way"""
    data = open(path, "rb").read()
    assert len(data) == HEADER_BYTES + (6 * KMER_TABLE + 2 * PW_TABLE) * 8 and data[:8] == b"PJBMODL1"
    l95, order, pw_len = struct.unpack_from("<3I", data, 8)
    assert (order, pw_len) == (5, 32)
    sizes = struct.unpack_from("<8i", data, 20)
    out, at = {"L95": l95}, HEADER_BYTES
    for name, size in zip(TABLES, sizes):
        n = PW_TABLE if name.endswith("_pw") else KMER_TABLE
        t = np.frombuffer(data, dtype="<f8", count=n, offset=at).copy()
        at += 8 * n
        assert np.isfinite(t).all() and (t >= 0).all() and (t <= 1).all(), name
        sums = t.reshape(-1, 5).sum(axis=1)
        trained = (t.reshape(-1, 5) != 0).any(axis=1)
        assert (np.abs(sums[trained] - 1.0) <= 1e-12).all() and int(trained.sum()) == size, name
        out[name], out[name + "_size"] = t, size
    return out


def same_tables(a, b):
    for name in TABLES:
        assert np.array_equal(a[name].view(np.uint64), b[name].view(np.uint64)), name
        assert a[name + "_size"] == b[name + "_size"], name


@pytest.fixture(scope="module")
def selftrained(world):
    """the self-training run with --save_models, and the same run without"""
    out = {}
    for name, opts in (("with", ("--save_models",)), ("without", ())):
        prefix = str(world["dir"] / ("bundle_" + name) / "pc")
        p = run("filt", "--self_train", sx.DATA, "--training_rule", RULESET, "--save_features", "--save_bad", *opts, "-o", prefix, world["prep"], world["tab"])
        out[name] = (prefix, p.stdout)
    return out


def listing(prefix):
    return sorted(os.listdir(os.path.dirname(prefix)))


def test_self_training_saves_what_it_trained(ffi, world, selftrained):
    from oracle import oracle as orc
    (out, stdout), (plain, plain_stdout) = selftrained["with"], selftrained["without"]
    b = read_bundle(out + ".selftrain.models")
    assert b["L95"] == SETS[RULESET]["L95"]
    assert f"Saved L95 and Markov models to file {out}.selftrain.models" in stdout and ".selftrain.models" not in plain_stdout
    # the oracle's models on the fixture's sets
    drows = rows_of(ffi, world["header"], world["rows"])
    pos = [world["by_key"][tuple(k)] for k in SETS[RULESET]["pos"]]
    neg = [world["by_key"][tuple(k)] for k in SETS[RULESET]["neg"]]
    orows = np.zeros(len(drows), dtype=orc.ROW_DTYPE)
    for name in set(orc.ROW_DTYPE.names) & set(ffi.ROW_DTYPE.names):
        orows[name] = drows[name]
    _, models, _ = orc.filt_features([sx.GENOME_LEN], {0: world["genome"]}, orows, pos, pos, pos, neg)
    for name in TABLES:
        assert np.array_equal(b[name].view(np.uint64), models[name].view(np.uint64)), name
    for k in ("exon_size", "intron_size", "donor_pw_size", "acceptor_pw_size"):
        assert b[k] == models[k] > 0, k
    # the flag adds one file and changes no other
    assert "pc.selftrain.models" not in listing(plain) and listing(out) == sorted(listing(plain) + ["pc.selftrain.models"])
    for name in (".pass.junctions.tab", ".fail.junctions.tab", ".selftrain.forest", ".selftrain.features", ".features.testing",
                 ".selftrain.initialset.pos.junctions.tab", ".selftrain.initialset.neg.junctions.tab"):
        assert open(out + name, "rb").read() == open(plain + name, "rb").read(), name


def model_columns(path):
    h, rows = read_tab(path)
    return [[r[h.index(c)] for c in MODEL_COLUMNS] for r in rows]


def test_the_saved_model_reapplied_gives_the_runs_own_tables(world, selftrained):
    out, _ = selftrained["with"]
    again = str(world["dir"] / "bundle_again" / "pc")
    run("filt", "--model_file", out + ".selftrain.forest", "--models_file", out + ".selftrain.models", "--save_bad", "--save_features", "-o", again, world["prep"],
        world["tab"])
    for name in (".pass.junctions.tab", ".fail.junctions.tab", ".features.testing"):
        assert open(again + name, "rb").read() == open(out + name, "rb").read(), name
    assert len(keys_of(again + ".pass.junctions.tab")) > 0 and len(keys_of(again + ".fail.junctions.tab")) > 0
    # without the models the forest sees other rows: the test can see the models
    bare = str(world["dir"] / "bundle_bare" / "pc")
    run("filt", "--model_file", out + ".selftrain.forest", "--save_bad", "--save_features", "-o", bare, world["prep"], world["tab"])
    mine, theirs = model_columns(bare + ".features.testing"), model_columns(out + ".features.testing")
    assert len(mine) == len(theirs) == len(world["rows"]) and mine != theirs
    assert not os.path.exists(bare + ".selftrain.models") and not os.path.exists(again + ".selftrain.models")


def test_train_markov(ffi, ctx, world, selftrained):
    out, _ = selftrained["with"]
    pos_tab, neg_tab = out + ".selftrain.initialset.pos.junctions.tab", out + ".selftrain.initialset.neg.junctions.tab"
    model = str(world["dir"] / "bundle_train" / "model")
    run("train", "--markov", "--trees", "8", "-o", model, world["prep"], pos_tab, neg_tab)
    assert sorted(os.listdir(os.path.dirname(model))) == ["model.forest", "model.models"]
    b = read_bundle(model + ".models")
    same_tables(b, read_bundle(out + ".selftrain.models"))
    h, prow = read_tab(pos_tab)
    sizes = sorted(int(r[h.index("end")]) - int(r[h.index("start")]) + 1 for r in prow)
    assert b["L95"] == sizes[int(0.95 * len(sizes))]
    # the forest: grown on the rows those models make (one target: the table's own order is the sorted order)
    order, labels = real_rows(world, RULESET)
    drows = rows_of(ffi, world["header"], world["rows"])[order]
    mrl = float(world["rows"][0][world["header"].index("mean_readlen")])

    def grown_on(l95, models):
        M = np.ascontiguousarray(ctx.filt_features(drows, mrl, l95, models)[:, fu.ACTIVE_FEATURES])
        M[:, 0] = labels
        return M, ctx.forest_grow(M, n_trees=8).to_bytes()
    M, forest = grown_on(b["L95"], b)
    assert open(model + ".forest", "rb").read() == forest
    assert (M[:, fu.ACTIVE_FEATURES.index(12)] != 0).any() and (M[:, fu.ACTIVE_FEATURES.index(9)] > 0).any()
    # without the flag: what train writes today
    plain = str(world["dir"] / "bundle_train_plain" / "model")
    p = run("train", "--trees", "8", "-o", plain, world["prep"], pos_tab, neg_tab)
    assert os.listdir(os.path.dirname(plain)) == ["model.forest"] and "Markov" not in p.stdout
    M0, forest0 = grown_on(0, {})
    assert open(plain + ".forest", "rb").read() == forest0 and forest0 != forest


def test_full_passes_save_models_on(tmp_path):
    fa, bam = make_input(tmp_path, 300, 3, 1500, 90, 30000)   # (test_gpu_full_cli.py's trained input: 654 junctions)
    x, y = str(tmp_path / "chain"), str(tmp_path / "full")
    run("prep", "-o", f"{x}/1-prep", fa, bam)
    run("junc", "-o", f"{x}/2-junc/portcullis_all", f"{x}/1-prep")
    run("filt", "--self_train", FULL_DATA, "--training_rule", FULL_RULES, "--save_models", "-o", f"{x}/3-filt/portcullis_filtered", f"{x}/1-prep",
        f"{x}/2-junc/portcullis_all.junctions.tab")
    run("full", "--keep_temp", "--save_models", "--self_train", FULL_DATA, "--training_rule", FULL_RULES, "-o", y, fa, bam)
    name = "3-filt/portcullis_filtered.selftrain.models"
    assert read_bundle(os.path.join(y, name))["exon_size"] > 0
    assert open(os.path.join(y, name), "rb").read() == open(os.path.join(x, name), "rb").read()
    assert sorted(os.listdir(os.path.join(y, "3-filt"))) == sorted(os.listdir(os.path.join(x, "3-filt")))
