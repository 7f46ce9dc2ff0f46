"""`portcullis_amd full` gives, file for file and byte for byte, the directory that `prep`, `junc`, `filt --self_train` and `bamfilt` leave
when they are run one after another.  The yardstick is always that chain, run in the same session; each input runs the chain and `full`
once, and the tests compare the two directories.  Three generated inputs, one per route of self-training: a forest is grown (500
junctions or more), the lenient rule file takes its place (fewer than 200), filt refuses (200 to 499).  The junction counts were
established on the CPU with oracle/orc_bam2tab (654, 100 and 305) and are asserted on the chain's own table."""
import os
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import PREP_BAM, PREP_FA, write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")
RULES = "balanced"  # 126 positive and 93 negative initial junctions on the trained input (filt's own count, on the oracle's table)
PREPARED = (PREP_BAM, PREP_BAM + ".bai", PREP_FA, PREP_FA + ".fai")


def run(*args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    env.update(env_extra or {})
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)


def tail(p):
    return f"status {p.returncode}\n" + p.stdout[-1500:] + p.stderr[-1500:]


def make_input(d, seed, n_targets, n_reads, n_tx, glen):
    """A genome and a coordinate-sorted BAM, neither with an index: (genome, bam)."""
    refs, contigs, reads = [], [], []
    for tid in range(n_targets):
        genome, rr = make_reads(seed + tid, n_reads=n_reads, glen=glen, n_tx=n_tx)
        for r in rr:
            r["tid"] = tid
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    bam, fa = str(d / "in.bam"), str(d / "genome.fa")
    write_bam(bam, refs, reads, write_index=False)
    write_fasta(fa, contigs, write_index=False)
    return fa, bam


def chain(x, fa, bam, junc_opts=(), filt_opts=(), bamfilt=False):
    """The four commands into x, each a process of its own; stops at the first that fails.  Returns the processes."""
    steps = [("prep", "-o", f"{x}/1-prep", fa, bam),
             ("junc", *junc_opts, "-o", f"{x}/2-junc/portcullis_all", f"{x}/1-prep"),
             ("filt", "--self_train", DATA, "--training_rule", RULES, *filt_opts, "-o", f"{x}/3-filt/portcullis_filtered", f"{x}/1-prep",
              f"{x}/2-junc/portcullis_all.junctions.tab")]
    if bamfilt:
        steps.append(("bamfilt", "-o", f"{x}/portcullis.filtered.bam", f"{x}/3-filt/portcullis_filtered.pass.junctions.tab", f"{x}/1-prep/{PREP_BAM}"))
    done = []
    for s in steps:
        done.append(run(*s))
        if done[-1].returncode != 0:
            break
    return done


def tree(top, under=""):
    """relative path -> ("link", where it points) | ("file", its bytes) of everything under top/under"""
    out = {}
    for dirpath, dirnames, filenames in os.walk(os.path.join(top, under)):
        for n in dirnames + filenames:
            p = os.path.join(dirpath, n)
            if os.path.islink(p):
                out[os.path.relpath(p, top)] = ("link", os.readlink(p))
            elif os.path.isfile(p):
                out[os.path.relpath(p, top)] = ("file", open(p, "rb").read())
    return out


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k


def data_rows(tab_bytes):
    return tab_bytes.count(b"\n") - 1


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp("full_trained")
    fa, bam = make_input(d, 300, 3, 1500, 90, 30000)
    x, y = str(d / "chain"), str(d / "full")
    steps = chain(x, fa, bam, filt_opts=("--save_bad",), bamfilt=True)
    assert len(steps) == 4 and steps[-1].returncode == 0, tail(steps[-1])
    want = tree(x)
    # a degenerate input must fail here, not pass on the rule file's route
    assert data_rows(want["2-junc/portcullis_all.junctions.tab"][1]) >= 500
    assert "3-filt/portcullis_filtered.selftrain.forest" in want
    assert data_rows(want["3-filt/portcullis_filtered.pass.junctions.tab"][1]) > 0 and data_rows(want["3-filt/portcullis_filtered.fail.junctions.tab"][1]) > 0
    args = ("full", "-b", "--keep_temp", "--save_bad", "--self_train", DATA, "--training_rule", RULES, "-o", y, fa, bam)
    p = run(*args)
    assert p.returncode == 0, tail(p)
    return dict(want=want, got=tree(y), stdout=p.stdout, args=args, y=y)


@pytest.fixture(scope="module")
def few(tmp_path_factory):
    d = tmp_path_factory.mktemp("full_few")
    fa, bam = make_input(d, 90, 3, 400, 12, 20000)
    before = (open(fa, "rb").read(), open(bam, "rb").read())
    x, y = str(d / "chain"), str(d / "full")
    steps = chain(x, fa, bam)
    assert len(steps) == 3 and steps[-1].returncode == 0, tail(steps[-1])
    want = tree(x)
    assert 0 < data_rows(want["2-junc/portcullis_all.junctions.tab"][1]) < 200
    args = ("full", "--self_train", DATA, "--training_rule", RULES, "-o", y, fa, bam)
    p = run(*args)
    assert p.returncode == 0, tail(p)
    return dict(d=d, fa=fa, bam=bam, before=before, x=x, want=want, got=tree(y), stdout=p.stdout, args=args, y=y)


@pytest.fixture(scope="module")
def refused(tmp_path_factory):
    d = tmp_path_factory.mktemp("full_refused")
    fa, bam = make_input(d, 300, 2, 1000, 70, 25000)
    x, y = str(d / "chain"), str(d / "full")
    steps = chain(x, fa, bam, bamfilt=True)
    assert len(steps) == 3 and steps[-1].returncode == 4, tail(steps[-1])  # filt refuses; bamfilt is not reached
    want = tree(x)
    assert 200 <= data_rows(want["2-junc/portcullis_all.junctions.tab"][1]) < 500
    p = run("full", "-b", "--keep_temp", "--self_train", DATA, "--training_rule", RULES, "-o", y, fa, bam)
    return dict(want=want, got=tree(y), p=p, chain_filt=steps[-1])


def test_a_trained_run_leaves_the_chains_directory(trained):
    assert_same(trained["got"], trained["want"])
    got = trained["got"]
    for name in PREPARED[:1] + PREPARED[2:3]:
        assert got["1-prep/" + name][0] == "link"
    assert got["portcullis.filtered.bam"][0] == "file" and got["portcullis.filtered.bam.bai"][0] == "file"
    out = trained["stdout"]
    for text in ("Running full portcullis pipeline", "Preparing input data (BAMs + genome)", "Identifying junctions and calculating metrics", "Filtering junctions",
                 "Filtering BAMs"):
        assert f"{text}\n{'-' * len(text)}\n" in out, text
    assert "Self training mode activated." in out and "Portcullis completed.\nTotal runtime: " in out
    assert "Cleaning temporary files" not in out  # --keep_temp


def test_few_junctions_take_the_rule_file_and_clean_removes_links_only(few):
    assert "Less that 200 junctions found in input set." in few["stdout"]
    want = {k: v for k, v in few["want"].items() if not k.startswith("1-prep/")}
    assert "3-filt/portcullis_filtered.selftrain.forest" not in want and "3-filt/portcullis_filtered.pass.junctions.tab" in want
    assert_same(few["got"], want)  # no 1-prep entry, no filtered BAM
    assert os.path.isdir(os.path.join(few["y"], "1-prep")) and os.listdir(os.path.join(few["y"], "1-prep")) == []
    assert not os.path.exists(os.path.join(few["y"], "portcullis.filtered.bam"))
    assert "Cleaning temporary files... done." in few["stdout"]
    assert (open(few["fa"], "rb").read(), open(few["bam"], "rb").read()) == few["before"]


def test_200_to_499_junctions_are_refused_with_filts_message_and_the_stages_before_are_complete(refused):
    p = refused["p"]
    assert p.returncode == 4, tail(p)
    assert "Not enough junctions to create training set" in p.stderr
    assert p.stderr.strip().split("\n")[-1] == refused["chain_filt"].stderr.strip().split("\n")[-1]
    got, want = refused["got"], refused["want"]
    for stage in ("1-prep/", "2-junc/"):
        assert_same({k: v for k, v in got.items() if k.startswith(stage)}, {k: v for k, v in want.items() if k.startswith(stage)})
    assert sorted(k for k in got if k.startswith("1-prep/")) == sorted("1-prep/" + n for n in PREPARED)
    assert not any(k.endswith(".pass.junctions.tab") for k in got) and "portcullis.filtered.bam" not in got
    assert "Filtering BAMs" not in p.stdout and "Portcullis completed." not in p.stdout


def test_extra_gives_the_files_of_junc_extra(few, tmp_path):
    x, y = str(tmp_path / "chain"), str(tmp_path / "full")
    os.makedirs(x)
    os.symlink(os.path.join(few["x"], "1-prep"), os.path.join(x, "1-prep"))  # (the chain's prepared directory, made once)
    for s in (("junc", "--extra", "-o", f"{x}/2-junc/portcullis_all", f"{x}/1-prep"),
              ("filt", "--self_train", DATA, "--training_rule", RULES, "-o", f"{x}/3-filt/portcullis_filtered", f"{x}/1-prep", f"{x}/2-junc/portcullis_all.junctions.tab")):
        p = run(*s)
        assert p.returncode == 0, tail(p)
    p = run("full", "--extra", "--self_train", DATA, "--training_rule", RULES, "-o", y, few["fa"], few["bam"])
    assert p.returncode == 0, tail(p)
    want = {k: v for k, v in tree(x).items() if k != "1-prep"}
    assert want["2-junc/portcullis_all.junctions.tab"] != few["want"]["2-junc/portcullis_all.junctions.tab"]  # the extra metrics are in it
    assert_same(tree(y), want)


def test_early_return_gives_the_same_files_and_status(few, tmp_path):
    y = str(tmp_path / "full")
    args = [a if a != few["y"] else y for a in few["args"]]
    p = run(*args, env_extra={"PORTCULLIS_EARLY_RETURN": "1"})
    assert p.returncode == 0, tail(p)
    assert_same(tree(y), few["got"])
    assert "Portcullis completed." in p.stdout


def test_a_second_run_finds_the_prepared_files_and_reproduces_the_outputs(trained):
    p = run(*trained["args"])  # the same output directory, no --force
    assert p.returncode == 0, tail(p)
    assert "Pre-indexed BAM detected" in p.stdout and "Prepped genome file detected" in p.stdout
    assert_same(tree(trained["y"]), trained["want"])
