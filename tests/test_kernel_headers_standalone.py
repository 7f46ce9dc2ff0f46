"""The stages of the junc chain that have a header of their own, and the helper headers they share (the `#include "pjb_*.hip.h"` lines of
portcullis_amd/csrc/pjb_kernels.hip.h: a listed header with a `__global__` kernel in it is a stage, one without is a helper).  No stage
header includes another: what two stages use stands in pjb_device.hip.h or in a helper, so that nothing depends on the order they are
included in.  Here: the stages that have been cut out stay cut out, every kernel is defined in one place, no stage header includes a stage,
and every listed header compiles on its own with the Makefile's flags (device side, syntax only: nothing is launched, no assembly is
looked at)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "portcullis_amd", "csrc")
INDEX = "pjb_kernels.hip.h"
INCLUDE = re.compile(r'^\s*#\s*include\s+"(pjb_[A-Za-z0-9_]+\.hip\.h)"', re.M)
KERNEL = re.compile(r"__global__[^;{]*?\bvoid\s+([a-z0-9_]+)\s*\(")


def text_of(name):
    return open(os.path.join(CSRC, name)).read()


def includes_of(name):
    return INCLUDE.findall(text_of(name))


def kernels_of(name):
    return KERNEL.findall(text_of(name))


LISTED = includes_of(INDEX)
SHARED = "pjb_device.hip.h"  # (every unit's: the generic scan's kernels are in it)
STAGES = [h for h in LISTED if h != SHARED and kernels_of(h)]
HELPERS = [h for h in LISTED if h == SHARED or not kernels_of(h)]


def makefile_hipflags():
    text = text_of("Makefile")
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    return re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


def test_the_stages_cut_out_stay_cut_out():
    assert {"pjb_k2d_ids.hip.h", "pjb_k2_sort.hip.h", "pjb_k2s_runs.hip.h", "pjb_k4_pairs.hip.h"} <= set(STAGES), STAGES
    assert {"pjb_device.hip.h", "pjb_basecmp.hip.h", "pjb_readops.hip.h"} <= set(HELPERS), HELPERS
    assert len(set(LISTED)) == len(LISTED), LISTED
    # a kernel is defined in one place: none of a stage header's kernels is left, or comes back, in the file that lists it
    names = [k for h in [INDEX] + STAGES for k in kernels_of(h)]
    assert len(names) >= 29 and sorted(set(names)) == sorted(names), sorted(n for n in set(names) if names.count(n) > 1)
    # and none of a stage's families begins in one file and goes on in another (kd_*, rs_*, k2_*, kf_*, k4*)
    for prefix in ("kd_", "rs_", "k2_", "kf_", "k4"):
        assert not [k for k in kernels_of(INDEX) if k.startswith(prefix)], prefix


@pytest.mark.parametrize("name", STAGES + HELPERS)
def test_no_header_includes_a_stage(name):
    named = [h for h in includes_of(name) if h in STAGES or h == INDEX]
    assert not named, f"{name} includes the stage header(s) {named}: what two stages use belongs in pjb_device.hip.h or a helper header"
    unlisted = [h for h in includes_of(name) if h not in LISTED]
    assert not unlisted, f"{name} includes {unlisted}, which {INDEX} does not list"


@pytest.mark.parametrize("name", STAGES + HELPERS)
def test_header_compiles_on_its_own(name):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (os.path.isfile(hipcc) and os.access(hipcc, os.X_OK)):
        pytest.skip("hipcc not found")
    out = subprocess.run([hipcc] + makefile_hipflags() + ["--offload-device-only", "-fsyntax-only", "-x", "hip", name], cwd=CSRC,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
