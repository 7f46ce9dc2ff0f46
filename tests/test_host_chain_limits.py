"""The limit policy of a `junc` chain -- the first limits, what an overflow changes, the attempt budget, a group member's
span (portcullis_amd/csrc/pjb_limits.hip.h) -- on the CPU: tests/cpp/chain_limits.cc holds the cases and their expected
values, written out by hand from the expressions the policy had inside pjb_api.hip.  The program is host code with a main
of its own, built with the address and undefined-behaviour sanitizers linked in, and run directly: no context, no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_limits(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "chain_limits")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                           "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", f"-I{ROOT}/portcullis_amd/csrc",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "chain_limits.cc")])
    out = subprocess.run([exe], capture_output=True, text=True,
                         env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
