"""The Markov model file (ml::ModelBundle: <prefix>.selftrain.models of `filt --self_train --save_models`, <prefix>.models of `train --markov`)
where it needs no device: the format and its check in a stand-alone program built under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/cpp/model_bundle_check.cc; PJB_TEST_SANITIZE=0: without them), and the refusals of `filt` around --save_models and --models_file --
every one with status 4, the file and the fault in the message, and the devices hidden: a bundle is checked before one is looked for."""
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_selftrain_sets_fixture as sx  # noqa: E402  (it touches nothing on import)

HOST = os.path.join(ROOT, "portcullis_amd", "host")
EXE = os.path.join(HOST, "portcullis_amd")
HEADER_BYTES = 8 + 3 * 4 + 8 * 4
FILE_BYTES = HEADER_BYTES + (6 * 3125 * 5 + 2 * 32 * 5) * 8


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("model_bundle") / "model_bundle_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"] if os.environ.get("PJB_TEST_SANITIZE", "1") != "0" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", *san, f"-I{HOST}/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "model_bundle_check.cc"),
                           os.path.join(HOST, "src", "model_bundle.cc")])
    return exe


def run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120)


def program(mode, *args):
    """the program with the devices hidden: nothing here may open one"""
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([EXE, mode, *args], capture_output=True, text=True, timeout=60, env=env)


def refused(p, *texts):
    assert p.returncode == 4, (p.returncode, p.stdout[-300:], p.stderr[-300:])
    for t in texts:
        assert t in p.stderr, (t, p.stderr)


@pytest.fixture(scope="module")
def world(tmp_path_factory, checker):
    d = tmp_path_factory.mktemp("bundle_in")
    header, rows = sx.selftrain_table()
    tab = d / "in.junctions.tab"
    tab.write_text(sx.table_text(header, rows))
    prep = d / "prep"
    prep.mkdir()
    (prep / "portcullis.genome.fa").write_text(">unused\nACGT\n")
    forest = d / "some.forest"
    forest.write_bytes(b"not a forest")
    good = d / "good.models"
    assert run(checker, "make", good, "trained").returncode == 0
    return dict(dir=d, tab=str(tab), prep=str(prep), forest=str(forest), good=str(good), bytes=good.read_bytes())


def test_the_format_in_a_sanitized_program(checker, tmp_path):
    p = run(checker, "selftest", tmp_path)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
    for kind in ("trained", "untrained"):
        f = tmp_path / (kind + ".made")
        assert run(checker, "make", f, kind).returncode == 0
        data = f.read_bytes()
        assert len(data) == FILE_BYTES == 752612 and data[:8] == b"PJBMODL1" and struct.unpack_from("<3I", data, 8)[1:] == (5, 32)
        p = run(checker, "check", f)
        assert p.returncode == 0 and p.stdout.startswith("ok L95 "), p.stderr
        sizes = struct.unpack_from("<8i", data, 20)
        assert p.stdout.split()[-8:] == [str(v) for v in sizes] and (all(v == 0 for v in sizes) if kind == "untrained" else all(v > 0 for v in sizes))
        if kind == "untrained":
            assert not any(data[HEADER_BYTES:])


def test_models_file_needs_a_model_file(world, tmp_path):
    out = str(tmp_path / "pc")
    tail = ("-o", out, world["prep"], world["tab"])
    for opts in (["--models_file", world["good"]], ["--models_file", world["good"], "--no_ml"], ["--models_file", world["good"], "--no_ml", "-m", world["forest"]],
                 ["--models_file", world["good"], "--self_train", sx.DATA]):
        refused(program("filt", *opts, *tail), "--models_file " + world["good"], "--model_file", "--self_train", "--no_ml")
    assert not os.path.exists(out + ".pass.junctions.tab")


def test_save_models_belongs_to_self_training(world, tmp_path):
    tail = ("-o", str(tmp_path / "pc"), world["prep"], world["tab"])
    refused(program("filt", "--no_ml", "--save_models", *tail), "--save_models", "not built into portcullis_amd filt without --self_train", "--model_file")
    refused(program("filt", "-m", world["forest"], "--save_models", *tail), "--save_models", "not built into portcullis_amd filt without --self_train")


def test_a_missing_models_file_is_said_to_be_missing(world, tmp_path):
    gone = str(tmp_path / "gone.models")
    refused(program("filt", "-m", world["forest"], "--models_file", gone, "-o", str(tmp_path / "pc"), world["prep"], world["tab"]),
            "Could not find Markov model file at: " + gone)


def corrupt(data, kind):
    b = bytearray(data)
    row = next(r for r in range(3125) if any(b[HEADER_BYTES + 40 * r:HEADER_BYTES + 40 * r + 40]))   # a trained row of the exon model
    at = HEADER_BYTES + 40 * row
    if kind == "magic":
        b[:8] = b"PJBMODL2"
    elif kind == "truncated":
        del b[len(b) // 2:]
    elif kind == "nan":
        struct.pack_into("<d", b, at, float("nan"))
    elif kind == "half":
        struct.pack_into("<5d", b, at, 0.25, 0.25, 0.0, 0.0, 0.0)
    elif kind == "size":
        struct.pack_into("<i", b, 20 + 4, struct.unpack_from("<i", b, 20 + 4)[0] + 1)
    return bytes(b)


@pytest.mark.parametrize("kind,fault", [("magic", "magic PJBMODL1"), ("truncated", "truncated"), ("nan", "not a probability"), ("half", "sums to 0.5"),
                                        ("size", "intron states")])
def test_a_corrupt_models_file_is_refused_on_the_host(world, checker, tmp_path, kind, fault):
    bad = tmp_path / (kind + ".models")
    bad.write_bytes(corrupt(world["bytes"], kind))
    out = str(tmp_path / "pc")
    p = program("filt", "-m", world["forest"], "--models_file", str(bad), "-o", out, world["prep"], world["tab"])
    refused(p, "The Markov model file " + str(bad) + " cannot be used", fault)
    assert "Loading junctions" not in p.stdout and not os.path.exists(out + ".pass.junctions.tab")
    q = run(checker, "check", bad)
    assert q.returncode == 3 and fault in q.stderr


def test_a_sound_models_file_passes_the_check(world, tmp_path):
    """... and the run goes on to the next file it reads: the forest, which is none here"""
    p = program("filt", "-m", world["forest"], "--models_file", world["good"], "-o", str(tmp_path / "pc"), world["prep"], world["tab"])
    assert p.returncode == 4 and "Markov model file" not in p.stderr and "Loading junctions" in p.stdout, p.stderr


def test_help_lists_the_new_options():
    for mode, opts in (("filt", ("--save_models", "--models_file")), ("train", ("--markov",)), ("full", ("--save_models",))):
        p = program(mode, "--help")
        assert p.returncode == 1
        for opt in opts:
            assert opt in p.stdout, (mode, opt)
