"""Self-training where it needs no device: the initial sets against what the reference's own create_training_sets made of the same table under
pandas (tests/golden/selftrain_sets.json, made by tests/golden/make_selftrain_sets_fixture.py), SMOTE's synthesis, ENN's mask and the
under-sampling against the reference's own code (tests/golden/selftrain, made by tests/golden/make_knn_fixture.py), the Python restatements
the GPU tests lean on against the same witnesses, and the refusals of `filt --self_train`.  The C++ side is tests/cpp/self_train.cc, built
under AddressSanitizer + UndefinedBehaviorSanitizer (PJB_TEST_SANITIZE=0: without them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_knn_fixture as kx  # noqa: E402  (generators and restatements; they touch nothing on import)
import make_selftrain_sets_fixture as sx  # noqa: E402

EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = sx.DATA
SETS = sx.load_sets()
CASES = kx.load_cases()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("self_train") / "self_train")
    host = os.path.join(ROOT, "portcullis_amd", "host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"] if os.environ.get("PJB_TEST_SANITIZE", "1") != "0" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", *san, f"-I{host}/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "self_train.cc"),
                           os.path.join(host, "src", "self_train.cc"), os.path.join(host, "src", "rule_filter.cc")])
    return exe


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(header, rows, path of the 640-junction table, directory)"""
    d = tmp_path_factory.mktemp("selftrain_in")
    header, rows = sx.selftrain_table()
    assert len(rows) == SETS["n_rows"] >= 600
    path = d / "in.junctions.tab"
    path.write_text(sx.table_text(header, rows))
    return header, rows, str(path), d


def run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120)


def filt(*args):
    """the program with the devices hidden: nothing here may open one"""
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([EXE, "filt", *args], capture_output=True, text=True, timeout=60, env=env)


def test_fixture_covers_both_branches():
    r = SETS["rulesets"]
    assert set(r) == {"balanced", "precise", "lenient", "strict"}
    assert r["balanced"]["positive_layer_reverted"] and not r["lenient"]["positive_layer_reverted"]
    assert all(len(s["pos"]) >= 50 and len(s["neg"]) >= 50 for s in r.values())
    assert len(r["lenient"]["pos"]) >= 2 * len(r["lenient"]["neg"]) and len(r["strict"]["neg"]) > len(r["strict"]["pos"])


@pytest.mark.parametrize("ruleset", ["balanced", "precise", "lenient", "strict"])
def test_initial_sets_equal_the_reference(driver, table, ruleset):
    header, rows, path, _ = table
    p = run(driver, "sets", path, ruleset, DATA)
    assert p.returncode == 0, p.stderr
    got = {}
    for line in p.stdout.strip().split("\n"):
        name, *cells = line.split(" ")
        got.setdefault(name, []).append(cells)
    want = SETS["rulesets"][ruleset]
    pos_files, neg_files = sx.layer_files(ruleset)
    assert [c[0] for c in got["posfile"]] == pos_files and [c[0] for c in got["negfile"]] == neg_files   # by layer number
    assert int(got["L95"][0][0]) == want["L95"]
    assert [sx.key(header, rows[int(k)]) for k in got["pos"][0]] == want["pos"]
    assert [sx.key(header, rows[int(k)]) for k in got["neg"][0]] == want["neg"]
    # the tables --save_layers writes: one per layer that was applied, and the intron-size layers
    n_pos_layers = len(got["poslayer"]) - int(got["possizelayer"][0][0])
    names = [f"pos_layer_{k + 1}.tab" for k in range(n_pos_layers)] + ["pos_layer_intronsize.tab"] * int(got["possizelayer"][0][0])
    names += [f"neg_layer_{k + 1}.tab" for k in range(len(got["neglayer"]) - 1)] + ["neg_layer_intronsize.tab"]
    assert sorted(names) == want["layer_tables"]
    if want["positive_layer_reverted"]:   # the last layer applied left 100 rows or fewer, and the set is the layer before it (cut by size)
        assert len(got["poslayer"][n_pos_layers - 1]) <= 100 < len(got["pos"][0]) and n_pos_layers == len(pos_files) == 3


def test_a_directory_is_a_rule_set_and_a_missing_one_is_refused(driver, table, tmp_path):
    _, _, path, _ = table
    p = run(driver, "sets", path, os.path.join(DATA, "lenient"), str(tmp_path))     # a directory by that name wins over the data directory
    assert p.returncode == 0 and f"L95 {SETS['rulesets']['lenient']['L95']}\n" in p.stdout
    p = run(driver, "sets", path, "nosuch", DATA)
    assert p.returncode == 4 and "Could not find suitable directory containing training rules for ruleset" in p.stderr
    only_pos = tmp_path / "onlypos"
    only_pos.mkdir()
    (only_pos / "selftrain_initial_pos.layer1.json").write_text(open(sx.layer_files("lenient")[0][0]).read())
    p = run(driver, "sets", path, str(only_pos), DATA)
    assert p.returncode == 4 and "Not enough positive and negative layers found in " + str(only_pos) + " ruleset." in p.stderr


@pytest.mark.parametrize("case", CASES["smote"], ids=lambda c: c["name"])
def test_smote_synthesis_is_bit_equal_to_the_reference(driver, tmp_path, case):
    m = kx.case_matrix(case)
    nn = np.load(kx.path(case["name"] + ".nn.npy"))
    want = np.fromfile(kx.path(case["name"] + ".synth.u64"), dtype="<u8").reshape(case["synthetic_rows"], case["cols"])
    assert nn.shape == (case["rows"], case["k_used"]) and case["synthetic_rows"] == case["smoteness"] * case["rows"]
    m.astype("<f8").tofile(tmp_path / "m.f64")
    nn.astype("<u4").tofile(tmp_path / "nn.u32")
    p = run(driver, "smote", tmp_path / "m.f64", case["rows"], case["cols"], tmp_path / "nn.u32", nn.shape[1], case["smoteness"], tmp_path / "out.f64")
    assert p.returncode == 0, p.stderr
    got = np.fromfile(tmp_path / "out.f64", dtype="<u8").reshape(want.shape)
    assert np.array_equal(got, want)
    assert np.array_equal(kx.smote(m, nn, case["smoteness"]).view(np.uint64), want)   # the restatement the GPU tests use


@pytest.mark.parametrize("case", CASES["under"], ids=lambda c: c["name"])
def test_undersampling_survivors_equal_the_reference(driver, case):
    want = np.load(kx.path(case["name"] + ".left.npy"))
    p = run(driver, "under", case["size"], case["keep"])
    assert p.returncode == 0, p.stderr
    assert [int(v) for v in p.stdout.split()[1:]] == list(want) and len(want) == case["keep"]
    mine, at_end = kx.undersample(case["size"], case["keep"])
    assert list(mine) == list(want) and at_end == case["draws_at_end"]


def test_a_draw_past_the_last_index_removes_the_last_element():
    hit = [c for c in CASES["under"] if c["draws_at_end"] > 0]
    assert hit, "no witness case drew the vector's size"
    # such a draw is what tells the inclusive bound from an exclusive one: with uniform_int(0, size - 1) the survivors differ
    case = hit[0]
    gen, left = kx.Mt19937(kx.SEED), list(range(case["size"]))
    while len(left) > case["keep"]:
        del left[kx.uniform_int(gen, len(left) - 1)]
    assert left != list(np.load(kx.path(case["name"] + ".left.npy")))


@pytest.mark.parametrize("case", CASES["enn"], ids=lambda c: c["name"])
def test_enn_mask_equals_the_reference(driver, tmp_path, case):
    nn = np.load(kx.path(case["name"] + ".nn.npy"))
    lab = kx.case_labels(case)
    want = np.fromfile(kx.path(case["name"] + ".keep.u8"), dtype=np.uint8)
    nn.astype("<u4").tofile(tmp_path / "nn.u32")
    lab.tofile(tmp_path / "lab.u8")
    p = run(driver, "enn", tmp_path / "nn.u32", case["rows"], nn.shape[1], tmp_path / "lab.u8", 3)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip() == "".join(str(v) for v in want) and int(want.sum()) == case["kept"]
    assert np.array_equal(kx.enn_keep(nn, lab), want)


# ---- the program ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prep(table):
    d = table[3] / "prep"
    d.mkdir()
    (d / "portcullis.genome.fa").write_text(">unused\nACGT\n")
    return str(d)


def refused(p, *texts):
    assert p.returncode == 4, (p.returncode, p.stdout[-300:], p.stderr[-300:])
    for t in texts:
        assert t in p.stderr, (t, p.stderr)


def test_self_train_with_no_ml_or_a_model_is_refused(table, prep, tmp_path):
    _, _, path, _ = table
    out = str(tmp_path / "pc")
    refused(filt("--self_train", DATA, "--no_ml", "-o", out, prep, path), "--self_train", "--no_ml", "--model_file")
    refused(filt("--self_train", DATA, "-m", str(tmp_path / "x.forest"), "-o", out, prep, path), "--self_train", "--model_file")
    refused(filt("--self_train", str(tmp_path / "nodata"), "-o", out, prep, path), "Could not find the self-training data directory at: " + str(tmp_path / "nodata"))


def test_a_missing_rule_set_is_refused(table, prep, tmp_path):
    _, _, path, _ = table
    refused(filt("--self_train", DATA, "--training_rule", "nosuch", "-o", str(tmp_path / "pc"), prep, path),
            "Could not find suitable directory containing training rules for ruleset")


def test_300_junctions_are_refused_with_the_limit(table, prep, tmp_path):
    header, rows, _, _ = table
    tab = tmp_path / "in300.junctions.tab"
    tab.write_text(sx.table_text(header, rows[:300]))
    refused(filt("--self_train", DATA, "-o", str(tmp_path / "pc"), prep, str(tab)), "500 junctions", "holds 300", "--model_file")


def test_150_junctions_take_the_lenient_rule_file_and_open_no_device(table, prep, tmp_path):
    """fewer than 200 junctions: low_juncs_filter.json is the rule file, with the reference's message; the devices are hidden here"""
    header, rows, _, _ = table
    tab = tmp_path / "in150.junctions.tab"
    tab.write_text(sx.table_text(header, rows[:150]))
    out = str(tmp_path / "pc")
    p = filt("--self_train", DATA, "--save_bad", "-o", out, prep, str(tab))
    assert p.returncode == 0, p.stderr[-500:]
    assert "Less that 200 junctions found in input set.  This is not enough to build a trained model.  Will apply a lenient rule-based filter instead." in p.stdout
    g = lambda r, n: r[header.index(n)]
    want = [sx.key(header, r) for r in rows[:150]
            if int(g(r, "maxmmes")) >= 10 and int(g(r, "hamming5p")) >= 4 and int(g(r, "hamming3p")) >= 4 and g(r, "canonical_ss") in ("C", "S")]
    assert 10 < len(want) < 140
    lines = [l.split("\t") for l in open(out + ".pass.junctions.tab").read().split("\n") if l]
    assert [sx.key(lines[0], r) for r in lines[1:]] == want
    assert not os.path.exists(out + ".selftrain.forest")


def test_without_the_flag_every_refusal_stands(table, prep, tmp_path):
    _, _, path, _ = table
    out = str(tmp_path / "pc")
    refused(filt("-o", out, prep, path), "Self-training", "--model_file", "--no_ml", "--filter_file")
    for opt in (["--training_rule", "precise"], ["--no_smote"], ["--enn"], ["--save_layers"], ["--save_matrix"]):
        refused(filt("--no_ml", *opt, "-o", out, prep, path), opt[0], "not built into portcullis_amd filt", "--model_file")
        refused(filt(*opt, "-o", out, prep, path), opt[0], "not built into portcullis_amd filt")


def test_help_lists_the_self_training_options():
    p = filt("--help")
    assert p.returncode == 1
    for opt in ("--self_train", "--training_rule", "--no_smote", "--enn", "--save_layers", "--save_matrix"):
        assert opt in p.stdout, opt
