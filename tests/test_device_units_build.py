"""tests/hip/device_units (the unit tests of the device building blocks, run by test_gpu_device_units.py) cross-compiles for gfx950 on a
machine without a GPU, and every kernel header of portcullis_amd/csrc is one of its prerequisites: an edit to any of them rebuilds it."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPDIR = os.path.join(ROOT, "tests", "hip")
BIN = os.path.join(HIPDIR, "device_units")


def find_hipcc():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return hipcc if os.path.isfile(hipcc) and os.access(hipcc, os.X_OK) else None


def test_device_units_cross_compiles():
    if not find_hipcc():
        pytest.skip("hipcc not found")
    out = subprocess.run(["make", "-C", HIPDIR], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    assert os.path.isfile(BIN) and os.access(BIN, os.X_OK)
    assert subprocess.run(["make", "-q", "-C", HIPDIR], capture_output=True).returncode == 0  # fresh: nothing left to do
    # without a group it explains itself and starts nothing on a device
    usage = subprocess.run([BIN], capture_output=True, text=True)
    assert usage.returncode == 2 and "wave|scan|sort|cmp4|cmp2|k0" in usage.stderr
    headers = sorted(glob.glob(os.path.join(ROOT, "portcullis_amd", "csrc", "*.hip.h")))
    assert len(headers) >= 20
    for h in headers + sorted(glob.glob(os.path.join(HIPDIR, "*.hip*"))):  # (-W: as if the file had just been modified)
        stale = subprocess.run(["make", "-q", "-C", HIPDIR, "-W", os.path.relpath(h, HIPDIR)], capture_output=True)
        assert stale.returncode == 1, f"{os.path.relpath(h, ROOT)} is not a prerequisite of tests/hip/device_units"


def test_device_units_flags_are_the_librarys():
    """The kernels under test are compiled as the library compiles them: the library's HIPFLAGS without -fPIC."""
    import re

    def flags(path):
        text = open(path).read()
        return re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1).split()

    lib = [f for f in flags(os.path.join(ROOT, "portcullis_amd", "csrc", "Makefile")) if f != "-fPIC"]
    assert flags(os.path.join(HIPDIR, "Makefile")) == lib
