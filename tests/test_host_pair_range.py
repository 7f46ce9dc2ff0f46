"""The fragment rule of k4_pairs / k5_frag_reduce -- a fragment's slot, the slots of a chain, the slots left unused, the room a chain's
limits need (frag_slot and its neighbours in portcullis_amd/csrc/pjb_device.hip.h) -- on the CPU: tests/cpp/pair_range_slots.cc walks
seeded random id arrays with ranges of 1, 2, 4 and 16 slices.  The program is host code with a main of its own, built with the
address and undefined-behaviour sanitizers linked in, and run directly: no context, no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_range_slots(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "pair_range_slots")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                           "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", f"-I{ROOT}/portcullis_amd/csrc",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "pair_range_slots.cc")])
    out = subprocess.run([exe], capture_output=True, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
