"""`--device_mem` where it needs no device: the help of `junc` and `full` lists it, a size that is not an integer with an optional
K, M or G is refused before the prepared directory is opened, a good one shows up in the settings block -- and the policy behind
the budget (portcullis_amd/csrc/pjb_memory.hip.h: what a context releases before it refuses an allocation, and when it gives up)
runs clean as a stand-alone host program built with the address and undefined-behaviour sanitizers (tests/cpp/memory_policy.cc)."""
import os
import shutil
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import make_prep_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")


def run(*args, env_extra=None):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"  # (on a GPU box: none of this may need a device)
    env.update(env_extra or {})
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60, env=env)


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    genome, reads = make_reads(77, n_reads=200, glen=12000)
    for r in reads:
        r["tid"] = 0
    return make_prep_dir(str(tmp_path_factory.mktemp("devmem") / "prep"), [("chr1", len(genome))], [("chr1", genome)], reads)


def test_help_lists_the_option():
    p = run("junc", "--help")
    assert p.returncode == 0 and "--device_mem <size>" in p.stdout and "PORTCULLIS_DEVICE_MEM" in p.stdout
    p = run("full", "--help")
    assert p.returncode == 1 and "--device_mem arg" in p.stdout


@pytest.mark.parametrize("size", ["12x", "-5", "", "1.5G", "G", "4GB", "99999999999999999999", "17179869184G", "8589934592G", "9223372036854775808"])
def test_a_bad_size_is_refused_before_a_file_is_touched(tmp_path, size):
    missing = str(tmp_path / "no_such_prep")
    out = str(tmp_path / "out" / "pc")
    for p in (run("junc", "-o", out, "--device_mem", size, missing),
              run("junc", "-o", out, missing, env_extra={"PORTCULLIS_DEVICE_MEM": size}),
              run("full", "-o", out, "--self_train", DATA, "--device_mem", size, str(tmp_path / "no.fa"), str(tmp_path / "no.bam"))):
        assert p.returncode == 4, (p.returncode, p.stdout[-300:], p.stderr[-300:])
        assert "--device_mem takes a number of bytes" in p.stderr and f"'{size}'" in p.stderr, p.stderr
        assert "Could not find" not in p.stderr  # (the option's own refusal, not the missing directory's)
    assert not os.path.exists(str(tmp_path / "out"))


@pytest.mark.parametrize("size,nbytes", [("1G", 1 << 30), ("512M", 512 << 20), ("1048576", 1048576), ("3k", 3072), ("8589934591G", 8589934591 << 30)])
def test_a_good_size_is_in_the_settings_block(prep, tmp_path, size, nbytes):
    # (without a device the run ends once it needs one: the settings have been printed by then)
    for p in (run("junc", "-o", str(tmp_path / "a" / "pc"), "--device_mem", size, prep),
              run("junc", "-o", str(tmp_path / "b" / "pc"), prep, env_extra={"PORTCULLIS_DEVICE_MEM": size})):
        assert p.returncode == 4 and "No MI355X (HIP device) is visible" in p.stderr, (p.returncode, p.stdout[-500:], p.stderr[-500:])
        assert f" - Separate BAMs: false\n - Device memory: {nbytes} bytes per GPU\n\n" in p.stdout, p.stdout
    p = run("junc", "-o", str(tmp_path / "c" / "pc"), prep)  # no budget: the block is as it always was
    assert " - Separate BAMs: false\n\n" in p.stdout and "Device memory" not in p.stdout


def test_memory_policy(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    exe = str(tmp_path / "memory_policy")
    subprocess.check_call([cxx, "-fsanitize=address,undefined", "-O1", "-g", "-std=c++17", "-Wall", f"-I{ROOT}/portcullis_amd/csrc", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "memory_policy.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
