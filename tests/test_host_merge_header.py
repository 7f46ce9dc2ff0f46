"""The header of a merged BAM (`prep --merge`: mergeBamHeaders of portcullis/merge_header.hpp, a pure function) -- identical headers,
later @RG / @PG / @CO lines appended once, @HD made to say SO:coordinate, ID collisions and differing dictionaries refused by name:
tests/cpp/merge_header.cc holds the cases.  The program is host code with a main of its own, built with the address and
undefined-behaviour sanitizers linked in, and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_header(tmp_path):
    exe = str(tmp_path / "merge_header")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-fsanitize=address,undefined", "-O1", "-g", "-std=c++17", "-Wall",
                           f"-I{ROOT}/portcullis_amd/host/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "merge_header.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
