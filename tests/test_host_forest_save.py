"""The saving half of the forest file (ml::Forest::save, ffi.Forest.to_bytes): the exact inverse of the readers, on every committed forest;
and `portcullis_amd train` where it needs no device: its help and every refusal, with the devices hidden."""
import glob
import os
import subprocess

import pytest

from filt_cases import build_cases, tab_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
FORESTS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*", "*.forest")))


def test_every_committed_forest_is_found():
    names = {os.path.basename(p) for p in FORESTS}
    assert {"witness.forest", "G2.forest", "G3.forest", "G4a.forest", "G4b.forest", "G5.forest"} <= names


@pytest.fixture(scope="module")
def roundtrip(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("forest_roundtrip") / "forest_roundtrip")
    host = os.path.join(ROOT, "portcullis_amd", "host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", f"-I{host}/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "forest_roundtrip.cc"),
                           os.path.join(host, "src", "forest.cc")])
    return exe


@pytest.mark.parametrize("path", FORESTS, ids=[os.path.basename(p) for p in FORESTS])
def test_save_is_the_inverse_of_load(roundtrip, tmp_path, path):
    out = str(tmp_path / "again.forest")
    p = subprocess.run([roundtrip, path, out], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    raw = open(path, "rb").read()
    assert open(out, "rb").read() == raw
    assert p.stdout.split()[-1] == str(len(raw))


def test_save_says_when_it_cannot_write(roundtrip, tmp_path):
    p = subprocess.run([roundtrip, FORESTS[0], str(tmp_path / "no" / "such" / "dir.forest")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 3 and "Could not write to output file" in p.stderr


@pytest.mark.parametrize("path", FORESTS, ids=[os.path.basename(p) for p in FORESTS])
def test_to_bytes_is_the_inverse_of_from_file(path):
    from portcullis_amd import ffi
    assert ffi.Forest.from_file(path).to_bytes() == open(path, "rb").read()


# ---- the program --------------------------------------------------------------------------------------------------------------------------
def train(*args):
    """the program with the devices hidden: nothing here may open one"""
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([EXE, "train", *args], capture_output=True, text=True, timeout=60, env=env)


def test_help_and_usage():
    p = train("--help")
    assert p.returncode == 1 and "Usage: portcullis_amd train [options] <prep_data_dir> <positive_tab_file> <negative_tab_file>" in p.stdout
    for opt in ("--output", "--trees arg (=250)", "--seed arg (=1236456789)", "--save_features", "--verbose", "--help"):
        assert opt in p.stdout, opt
    assert train().returncode == 1 and train("prep", "pos.tab").returncode == 1
    p = subprocess.run([EXE, "frobnicate"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "portcullis_amd train [options] <prep_data_dir> <positive_tab_file> <negative_tab_file>" in p.stderr
    assert "portcullis_amd filt [options] <prep_data_dir> <junction_tab_file>" in p.stderr


def test_refusals_with_the_devices_hidden(tmp_path):
    case = sorted(build_cases().items())[0][1]
    lines = tab_of(case).split("\n")
    head, rows = lines[0], [l for l in lines[1:] if l]
    assert len(rows) >= 4
    prep = tmp_path / "prep"
    prep.mkdir()
    (prep / "portcullis.genome.fa").write_text(">unused\nACGT\n")

    def tab(name, some):
        (tmp_path / name).write_text("\n".join([head] + some) + "\n")
        return str(tmp_path / name)

    pos, neg, none, both = tab("pos.tab", rows[::2]), tab("neg.tab", rows[1::2]), tab("none.tab", []), tab("both.tab", rows[1::2] + rows[:1])
    out = str(tmp_path / "out" / "model")

    def refused(p, *texts):
        assert p.returncode == 4, (p.returncode, p.stdout[-500:], p.stderr[-500:])
        for t in texts:
            assert t in p.stderr, (t, p.stderr)
        assert not os.path.exists(out + ".forest")

    refused(train("-o", out, str(prep), str(tmp_path / "missing.tab"), neg), "Could not find positive junction file at: ", "missing.tab")
    refused(train("-o", out, str(prep), pos, str(tmp_path / "missing.tab")), "Could not find negative junction file at: ", "missing.tab")
    refused(train("-o", out, str(tmp_path / "noprep"), pos, neg), "Could not find prepared genome file at: ")
    refused(train("-o", out, str(prep), none, neg), "The positive set is empty: ")
    refused(train("-o", out, str(prep), pos, none), "The negative set is empty: ")
    refused(train("-o", out, str(prep), pos, both), "is in the positive and in the negative set")
    refused(train("-o", out, "--trees", "0", str(prep), pos, neg), "--trees must be at least 1")
    refused(train("-o", out, "--frobnicate", str(prep), pos, neg), "Unknown option: --frobnicate")
    refused(train("-o", out, str(prep), pos, neg), "No MI355X (HIP device) is visible", "no CPU fallback")
