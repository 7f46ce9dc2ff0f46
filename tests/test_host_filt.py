"""`portcullis_amd filt` where it needs no device (--no_ml): the rule engine against what the reference's own script and pandas made of the same
rule files over the same tables (tests/golden/filt_rules.json, made by tests/golden/make_rule_filter_fixture.py), the columns calcJunctionStats
recomputes, the post filters, the reference rescue, every refusal; the forest file reader against the Python reader of the same layout; and
pjb_forest_check, which is host arithmetic."""
import json
import os
import subprocess

import numpy as np
import pytest

import forest_util as fu
from filt_cases import build_cases, tab_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
RULES = os.path.join(ROOT, "tests", "golden", "filt_rules")
WITNESS = json.load(open(os.path.join(ROOT, "tests", "golden", "filt_rules.json")))


def filt(*args):
    """the program with the devices hidden: nothing here may open one"""
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([EXE, "filt", *args], capture_output=True, text=True, timeout=60, env=env)


def read_tab(path_or_text, is_text=False):
    """(header, rows): the cells of a .junctions.tab as text"""
    text = path_or_text if is_text else open(path_or_text).read()
    lines = [l for l in text.split("\n") if l]
    return lines[0].split("\t"), [l.split("\t") for l in lines[1:]]


def ident(header, row):
    g = lambda n: row[header.index(n)]
    return [g("refname"), int(g("start")), int(g("end")), g("consensus-strand")]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (prep dir, .tab path, header, rows).  filt asks the prep directory for its genome file only; --no_ml never reads it."""
    d = tmp_path_factory.mktemp("filt_in")
    out = {}
    for name, case in build_cases().items():
        prep = d / (name + "_prep")
        prep.mkdir()
        (prep / "portcullis.genome.fa").write_text(">unused\nACGT\n")
        tab = d / (name + ".junctions.tab")
        tab.write_text(tab_of(case))
        header, rows = read_tab(str(tab))
        assert len(rows) == WITNESS["cases"][name]["n_rows"]
        out[name] = (str(prep), str(tab), header, rows)
    return out


# ---- the rule files the reference's script cannot evaluate (see make_rule_filter_fixture.py): their meaning, restated
OWN = {
    "x01_plain_and_suffixed_key.json": lambda g: 4 <= int(g("nb_raw_aln")) <= 200,
    "x02_string_eq.json": lambda g: (g("read-strand") == "+" or g("canonical_ss") == "C") and int(g("size")) < 500,
}


@pytest.mark.parametrize("name", sorted(WITNESS["cases"]))
def test_rule_files_pass_what_pandas_passed(cases, tmp_path, name):
    prep, tab, header, rows = cases[name]
    rule_files = sorted(os.listdir(RULES))
    assert len(rule_files) == 10 and set(rule_files) == set(WITNESS["cases"][name]["rules"])
    for rule in rule_files:
        rec = WITNESS["cases"][name]["rules"][rule]
        if "passed" in rec:
            want = rec["passed"]
        else:
            assert rec["reference_fails_with"] == "SyntaxError"
            want = [ident(header, r) for r in rows if OWN[rule](lambda n, r=r: r[header.index(n)])]
        out = str(tmp_path / rule / "pc")
        p = filt("--no_ml", "--filter_file", os.path.join(RULES, rule), "--save_bad", "-o", out, prep, tab)
        assert p.returncode == 0, (rule, p.stdout[-500:], p.stderr[-500:])
        h, got = read_tab(out + ".pass.junctions.tab")
        assert h == header
        assert [ident(h, r) for r in got] == want, rule                # (the input is in JunctionSystem::sort order, and so is what passes)
        _, bad = read_tab(out + ".fail.junctions.tab")
        assert [ident(h, r) for r in bad] == [ident(header, r) for r in rows if ident(header, r) not in want], rule
        assert not os.path.exists(out + ".rules_in.junctions.tab") and not os.path.exists(out + ".rules_out.passed.junctions.tab")


def junction_stats(header, rows):
    """JunctionSystem::calcJunctionStats (lib/src/junction_system.cc:250-320) on a system that was filled by addJunction: its mean query length
    is 0, flags that are set stay set.  rows: lists of text cells, changed in place."""
    col = {n: header.index(n) for n in header}
    g = lambda r, n: int(r[col[n]])
    n = len(rows)
    if n == 0:
        return
    i = 0
    while i < n:                                                     # createJunctionGroup: a chain of neighbours sharing donor or acceptor
        group, cur = [i], i
        j = i + 1
        while j < n and g(rows[cur], "refid") == g(rows[j], "refid") and (g(rows[cur], "start") == g(rows[j], "start") or g(rows[cur], "end") == g(rows[j], "end")):
            group.append(j)
            cur = j
            j += 1
        best, most = group[0], 0
        for k in group:
            if most < g(rows[k], "nb_raw_aln"):
                most, best = g(rows[k], "nb_raw_aln"), k
            rows[k][col["uniq_junc"]] = "1" if len(group) == 1 else "0"
        rows[best][col["primary_junc"]] = "1"
        i = j
    NONE = str(2**32 - 1)
    lastdiff = False
    for i in range(n - 1):
        a, b = rows[i], rows[i + 1]
        diff = str(max(0, g(b, "start") - g(a, "end")))
        if g(a, "refid") != g(b, "refid"):
            a[col["dist_2_up_junc"]] = NONE
            b[col["dist_2_down_junc"]] = NONE
            if i == 0 or lastdiff:
                a[col["dist_2_down_junc"]] = NONE
            if i == n - 2:
                b[col["dist_2_up_junc"]] = NONE
            lastdiff = True
        else:
            if i == 0:
                a[col["dist_2_down_junc"]] = NONE
            a[col["dist_2_up_junc"]] = diff
            b[col["dist_2_down_junc"]] = diff
            if i == n - 2 and i != 0:
                b[col["dist_2_up_junc"]] = NONE
            lastdiff = False
    for r in rows:
        s = lambda v: v - 2**32 if v >= 2**31 else v
        down, up = s(g(r, "dist_2_down_junc")), s(g(r, "dist_2_up_junc"))
        near = max(down, up) if (down == -1 or up == -1) else min(down, up)
        r[col["dist_nearest_junc"]] = str(near % 2**32)
        r[col["mean_readlen"]] = "0"


def test_columns_of_the_pass_table_and_bed_score(cases, tmp_path):
    """every column but the ones calcJunctionStats recomputes equals the input row's; those equal the restatement above (the oracle's finalize
    also sorts, numbers the rows and knows the mean query length: not this step); the BED carries the score, as outputBED does with bedscore"""
    prep, tab, header, rows = cases["fuzz_wide_FR"]
    out = str(tmp_path / "pc")
    p = filt("-n", "-f", os.path.join(RULES, "default_filter.json"), "-o", out, "--source", "src", prep, tab)
    assert p.returncode == 0, p.stderr[-500:]
    want_ids = WITNESS["cases"]["fuzz_wide_FR"]["rules"]["default_filter.json"]["passed"]
    want = [list(r) for r in rows if ident(header, r) in want_ids]
    assert 100 < len(want) < len(rows)
    junction_stats(header, want)
    h, got = read_tab(out + ".pass.junctions.tab")
    recomputed = {"uniq_junc", "primary_junc", "dist_2_up_junc", "dist_2_down_junc", "dist_nearest_junc", "mean_readlen"}
    changed = set()
    by_id = {tuple(ident(header, r)): r for r in rows}
    for g_, w in zip(got, want):
        assert g_ == w
        src = by_id[tuple(ident(h, g_))]
        changed |= {h[k] for k in range(len(h)) if g_[k] != src[k]}
    assert changed <= recomputed and {"dist_2_up_junc", "mean_readlen"} <= changed
    assert not os.path.exists(out + ".fail.junctions.tab")           # (no --save_bad)
    bed = open(out + ".pass.junctions.bed").read().split("\n")
    assert bed[0].startswith("track name=\"junctions\"") and bed[-1] == "" and len(bed) == len(got) + 2
    for line, r in zip(bed[1:], got):
        c = line.split("\t")
        g = lambda n: r[h.index(n)]
        strand = g("consensus-strand")
        assert c == [g("refname"), g("left"), str(int(g("right")) + 1), "src_pass_" + g("index"), "0.000", "." if strand == "?" else strand, g("start"),
                     str(int(g("end")) + 1), "255,0,0", "2", f"{int(g('start')) - int(g('left'))},{int(g('right')) - int(g('end'))}",
                     f"0,{int(g('end')) - int(g('left')) + 1}"]


def _post(header, r, max_length=0, keep="OFF", min_cov=1):
    g = lambda n: r[header.index(n)]
    if max_length and int(g("size")) > max_length:
        return False
    if keep != "OFF" and g("canonical_ss") not in keep.split(","):
        return False
    return int(g("nb_raw_aln")) >= min_cov


@pytest.mark.parametrize("opts,kw", [
    (["--max_length", "300"], dict(max_length=300)),
    (["--canonical", "C"], dict(keep="C")),
    (["--canonical=C,S"], dict(keep="C,S")),
    (["--canonical", "OFF", "--min_cov", "5"], dict(min_cov=5)),
    (["--max_length", "1000", "--canonical", "n,s", "--min_cov", "2"], dict(max_length=1000, keep="N,S", min_cov=2)),
])
def test_post_filters(cases, tmp_path, opts, kw):
    prep, tab, header, rows = cases["fuzz_wide_FR"]
    out = str(tmp_path / "pc")
    p = filt("--no_ml", *opts, "-b", "-o", out, prep, tab)
    assert p.returncode == 0, p.stderr[-500:]
    want = [ident(header, r) for r in rows if _post(header, r, **kw)]
    assert 20 < len(want) < len(rows) - 20
    h, got = read_tab(out + ".pass.junctions.tab")
    assert [ident(h, r) for r in got] == want
    _, bad = read_tab(out + ".fail.junctions.tab")
    assert [ident(h, r) for r in bad] == [ident(header, r) for r in rows if not _post(header, r, **kw)]


def test_no_filter_at_all_keeps_every_junction(cases, tmp_path):
    prep, tab, header, rows = cases["fuzz3_FR"]
    out = str(tmp_path / "pc")
    p = filt("--no_ml", "-o", out, prep, tab)
    assert p.returncode == 0, p.stderr[-500:]
    h, got = read_tab(out + ".pass.junctions.tab")
    assert [ident(h, r) for r in got] == [ident(header, r) for r in rows]


def test_reference_bed_brings_discarded_junctions_back(cases, tmp_path):
    prep, tab, header, rows = cases["fuzz_wide_FR"]
    keep = lambda r: _post(header, r, min_cov=8)
    lost = [r for r in rows if not keep(r)]
    kept = [r for r in rows if keep(r)]
    g = lambda r, n: r[header.index(n)]

    def bed12(r, strand=None):
        return "\t".join([g(r, "refname"), g(r, "left"), str(int(g(r, "right")) + 1), "j", "0", strand or g(r, "consensus-strand"), g(r, "start"),
                          str(int(g(r, "end")) + 1), "255,0,0", "2", "1,1", "0,1"])
    back = lost[::7]
    lines = ["track name=\"junctions\""] + [bed12(r) for r in back] + [bed12(kept[0]), bed12(kept[1])]
    lines.append("\t".join(bed12(lost[1]).split("\t")[:6]))          # six columns: no entry
    lines.append(bed12(lost[2]) + "\textra")                         # thirteen columns: no entry
    wrong = "+" if g(lost[3], "consensus-strand") != "+" else "-"
    lines.append(bed12(lost[3], wrong))                              # the strand is part of the key
    lines.append("ctgX\t0\t10\tj\t0\t+\t3\t8\t255,0,0\t2\t1,1\t0,1")  # not in the sample
    assert lost[1] not in back and lost[2] not in back and lost[3] not in back
    ref = tmp_path / "ref.bed"
    ref.write_text("\n".join(lines) + "\n")
    out = str(tmp_path / "pc")
    p = filt("--no_ml", "--min_cov", "8", "-r", str(ref), "--save_bad", "-o", out, prep, tab)
    assert p.returncode == 0, p.stderr[-500:]
    h, got = read_tab(out + ".pass.junctions.tab")
    assert [ident(h, r) for r in got] == [ident(header, r) for r in kept] + [ident(header, r) for r in back]   # brought back behind what passed
    _, refkept = read_tab(out + ".ref.junctions.tab")
    assert [ident(h, r) for r in refkept] == [ident(header, r) for r in back]
    _, bad = read_tab(out + ".fail.junctions.tab")
    assert [ident(h, r) for r in bad] == [ident(header, r) for r in lost]                                       # (the discarded set keeps them)
    assert f"Brought back {len(back)} junctions" in p.stdout and f"Found {len(back) + 4} junctions in reference." in p.stdout
    assert f"Your sample contains {len(back) + 2} / {len(back) + 4} (" in p.stdout


def _rule(tmp_path, obj, name="rule.json"):
    path = tmp_path / name
    path.write_text(obj if isinstance(obj, str) else json.dumps(obj))
    return str(path)


def test_refusals_and_errors(cases, tmp_path):
    prep, tab, header, rows = cases["micro_FR"]
    out = str(tmp_path / "o" / "pc")

    def refused(p, *texts):
        assert p.returncode == 4, (p.returncode, p.stdout[-300:], p.stderr[-300:])
        for t in texts:
            assert t in p.stderr, (t, p.stderr)

    # self-training, the reference's default, and everything that belongs to it: refused with the way out
    refused(filt("-o", out, prep, tab), "Self-training", "--model_file", "--no_ml", "--filter_file")
    for opt in (["--training_rule", "precise"], ["--no_smote"], ["--enn"], ["--save_layers"]):
        refused(filt("--no_ml", *opt, "-o", out, prep, tab), opt[0], "not built into portcullis_amd filt", "--model_file")
    genuine = tmp_path / "genuine.txt"
    genuine.write_text("1\n" * len(rows))
    refused(filt("--no_ml", "-g", str(genuine), "-o", out, prep, tab), "--genuine", "not built into portcullis_amd filt")
    refused(filt("--no_ml", "--frobnicate", "-o", out, prep, tab), "Unknown option: --frobnicate")
    # existence checks, the reference's messages
    refused(filt("--no_ml", "-o", out, prep, tab + ".nope"), "Could not find junction file at: " + tab + ".nope")
    refused(filt("--no_ml", "-o", out, str(tmp_path / "noprep"), tab), "Could not find prepared genome file at: " + str(tmp_path / "noprep"))
    refused(filt("-m", str(tmp_path / "no.forest"), "-o", out, prep, tab), "Could not find filter model file at: ")
    refused(filt("--no_ml", "-f", str(tmp_path / "no.json"), "-o", out, prep, tab), "Could not find filter configuration file at: ")
    refused(filt("--no_ml", "-r", str(tmp_path / "no.bed"), "-o", out, prep, tab), "Could not find reference BED file at: ")
    blocker = tmp_path / "file"
    blocker.write_text("x")
    refused(filt("--no_ml", "-o", str(blocker / "pc"), prep, tab), "File exists with name of suggested output directory: " + str(blocker))
    refused(filt("--no_ml", "--canonical", "C,S,N,OFF", "-o", out, prep, tab), "Canonical filter mode contains too many modes.  Max is 2.")
    # the rule engine's error cases, the script's messages
    P = {"size": {"operator": "gt", "value": 10}}
    refused(filt("-n", "-f", _rule(tmp_path, {"parameters": {"size": {"operator": "ge", "value": 1}}, "expression": "size"}), "-o", out, prep, tab),
            "Unrecognized operator for size: ge")
    refused(filt("-n", "-f", _rule(tmp_path, {"parameters": {"sizes.1": {"operator": "gt", "value": 1}}, "expression": "sizes.1"}), "-o", out, prep, tab),
            "Unrecognized parameters: sizes\nFieldnames:\n\trefid\n\trefname", "\n\tJAD20\nParameter names:\n\tsizes")
    refused(filt("-n", "-f", _rule(tmp_path, {"parameters": P, "expression": "size & entropy"}), "-o", out, prep, tab),
            "Expression and required parameters mismatch:\n\tentropy")
    faulty = "Configuration is faulty - please ensure that the JSON has valid \"parameters\" and \"expression\" fields."
    refused(filt("-n", "-f", _rule(tmp_path, {"parameters": P}), "-o", out, prep, tab), faulty)
    refused(filt("-n", "-f", _rule(tmp_path, {"expression": "size"}), "-o", out, prep, tab), faulty)
    refused(filt("-n", "-f", _rule(tmp_path, {"parameters": {"index": {"operator": "gt", "value": 1}}, "expression": "index"}), "-o", out, prep, tab),
            "Unrecognized parameters: index")                        # (the table's index is no field)
    refused(filt("-n", "-f", _rule(tmp_path, '{"parameters": {'), "-o", out, prep, tab), "Could not read the filter configuration as JSON")
    refused(filt("-n", "-f", _rule(tmp_path, {"parameters": P, "expression": "size & ( size"}), "-o", out, prep, tab), "Could not read the filter's expression")
    refused(filt("-n", "-f", _rule(tmp_path, {"parameters": {"refname": {"operator": "gt", "value": 1}}, "expression": "refname"}), "-o", out, prep, tab),
            "holds strings, which take the operators eq, in and not in")
    assert not os.path.exists(out + ".pass.junctions.tab")


def test_help_lists_the_options():
    p = filt("--help")
    assert p.returncode == 1 and "Usage: portcullis_amd filt [options] <prep_data_dir> <junction_tab_file>" in p.stdout
    for opt in ("--output", "--save_bad", "--exon_gff", "--intron_gff", "--source", "--filter_file", "--reference", "--no_ml", "--model_file", "--max_length",
                "--canonical", "--min_cov", "--threshold", "--save_features", "--threads", "--verbose", "--help", "--devices"):
        assert opt in p.stdout, opt
    assert filt().returncode == 1
    p = subprocess.run([EXE, "frobnicate"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "portcullis_amd filt [options] <prep_data_dir> <junction_tab_file>" in p.stderr


def test_a_model_that_cannot_be_used_opens_no_device(cases, tmp_path):
    """a forest of other variables, or one that fails the check, is refused before a device is asked for (the devices are hidden here)"""
    import struct
    prep, tab, header, rows = cases["micro_FR"]
    raw = open(os.path.join(fu.WITNESS_DIR, "witness.forest"), "rb").read()
    out = str(tmp_path / "pc")
    other = tmp_path / "other.forest"                                 # 30 variables: header says so, one more ordered flag
    other.write_bytes(raw[:16] + struct.pack("<Q", 30) + b"\1" * 30 + struct.pack("<Q", 30) + raw[16 + 8 + 29 + 8:])
    p = filt("-m", str(other), "-o", out, prep, tab)
    assert p.returncode == 4 and "trained on 30 variables" in p.stderr and "29 columns" in p.stderr, p.stderr
    short = tmp_path / "short.forest"
    short.write_bytes(raw[:-9])
    p = filt("-m", str(short), "-o", out, prep, tab)
    assert p.returncode == 4 and "truncated file" in p.stderr, p.stderr
    # --no_ml wins over --model_file, as in the reference
    p = filt("-n", "-m", str(short), "-o", out, prep, tab)
    assert p.returncode == 0, p.stderr


# ---- the forest file reader -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parsers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filt_parsers") / "filt_parsers")
    host = os.path.join(ROOT, "portcullis_amd", "host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", f"-I{host}/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "filt_parsers.cc"),
                           os.path.join(host, "src", "forest.cc"), os.path.join(host, "src", "rule_filter.cc")])
    return exe


def test_forest_reader_against_the_python_reader(parsers, tmp_path):
    path = os.path.join(fu.WITNESS_DIR, "witness.forest")
    p = subprocess.run([parsers, "forest", path], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    got = {l.split(" ")[0]: l.split(" ")[1:] for l in p.stdout.strip().split("\n")}
    forest, _, _ = fu.witness()
    assert [int(v) for v in got["header"]] == [forest.n_trees, forest.n_vars, forest.dependent_var] == [8, 29, 0]
    assert [int(v) for v in got["is_ordered"]] == list(forest.is_ordered)
    assert [float.fromhex(v) for v in got["class_values"]] == forest.class_values == [0.0, 1.0]
    for name in ("tree_off", "left", "right", "count_off"):
        assert [int(v) for v in got[name]] == list(getattr(forest, name)), name
    internal = forest.left >= 0
    assert (np.array([int(v) for v in got["split_var"]])[internal] == forest.split_var[internal]).all()
    for name in ("split_value", "counts"):
        a = np.array([float.fromhex(v) for v in got[name]])
        assert (a.view(np.uint64) == getattr(forest, name).view(np.uint64)).all(), name
    raw = open(path, "rb").read()
    for cut, what in ((len(raw) - 1, "truncated file"), (len(raw) // 2, "truncated file"), (40, "truncated file"), (0, "truncated file")):
        f = tmp_path / "cut.forest"
        f.write_bytes(raw[:cut])
        p = subprocess.run([parsers, "forest", str(f)], capture_output=True, text=True, timeout=60)
        assert p.returncode == 4 and what in p.stderr, (cut, p.stderr)
    f = tmp_path / "long.forest"
    f.write_bytes(raw + b"\0")
    p = subprocess.run([parsers, "forest", str(f)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 4 and "goes on after its last tree (1 bytes too long)" in p.stderr, p.stderr
    for reader_input in (raw[:-1], raw + b"\0"):                      # the Python reader refuses the same files
        f.write_bytes(reader_input)
        from portcullis_amd import ffi
        with pytest.raises(ValueError):
            ffi.Forest.from_file(str(f))


def test_rule_engine_alone_matches_the_program(parsers, cases):
    """the parser program of the sanitizer run gives the witness's answers too"""
    prep, tab, header, rows = cases["fuzz3_FR"]
    for rule, rec in WITNESS["cases"]["fuzz3_FR"]["rules"].items():
        if "passed" not in rec:
            continue
        p = subprocess.run([parsers, "rules", os.path.join(RULES, rule), tab], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        flags = p.stdout.strip()
        assert len(flags) == len(rows)
        assert [ident(header, r) for r, f in zip(rows, flags) if f == "1"] == rec["passed"], rule


# ---- pjb_forest_check: host arithmetic, no device ------------------------------------------------------------------------------------------
def _tree(left, right, var=None, counts=None, n_classes=2):
    n = len(left)
    return dict(left=left, right=right, split_var=var or [1] * n, split_value=[0.5] * n,
                counts=counts or [[] if left[k] >= 0 or right[k] >= 0 else [1.0] * n_classes for k in range(n)])


def test_forest_check_accepts_and_refuses():
    from portcullis_amd import ffi
    forest, _, _ = fu.witness()
    assert forest.check() is None
    F = lambda trees, **kw: ffi.Forest(kw.pop("n_vars", 4), 2, trees, **kw)
    assert F([_tree([1, -1, -1], [2, -1, -1])]).check() is None
    assert F([_tree([-1], [-1])]).check() is None                     # a single terminal node
    refused = [
        (F([_tree([1, 0, -1], [2, 2, -1])]), "tree 0, node 1: a child is not behind its parent"),           # child <= parent
        (F([_tree([-1], [-1]), _tree([0, -1, -1], [2, -1, -1])]), "tree 1, node 0: a child is not behind its parent"),
        (F([_tree([1, -1, -1], [3, -1, -1])]), "tree 0, node 0: a child lies outside the tree"),
        (F([_tree([1, -1, -1], [-1, -1, -1])]), "tree 0, node 0 has one child only"),
        (F([_tree([1, -1, -1], [2, -1, -1])], is_ordered=[1, 0, 1, 1]), "variable 1 is unordered"),
        (F([_tree([1, -1, -1], [2, -1, -1], var=[0, 0, 0])]), "tree 0, node 0 splits on the dependent variable"),
        (F([_tree([1, -1, -1], [2, -1, -1], var=[4, 0, 0])]), "tree 0, node 0 splits on a variable the data does not have"),
        (F([_tree([1, -1, -1], [2, -1, -1], counts=[[], [1.0, 1.0], []])]), "tree 0, node 2: a terminal node without its class counts"),
        (F([]), "0 trees"),
        (F([_tree([1, 3, -1, -1], [2, 3, -1, -1])]), "a child has two parents"),
    ]
    for f, text in refused:
        msg = f.check()
        assert msg is not None and text in msg, (text, msg)
