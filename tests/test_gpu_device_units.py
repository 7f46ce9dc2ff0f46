"""The device building blocks on the inputs they accept, not only on those a legal chain produces: tests/hip/device_units (a program of its
own over the kernel headers: no library, no context; tests/hip/device_units.hip says what a case is) run one group per test.  Every
comparison in it is exact, against plain host loops; this module only starts it, reads its verdict and holds the number of cases.

Time limits: a group's wall time on the MI355X (program start to exit; the slowest of three runs), times ten, at least 30 s --
    wave 0.38 s, scan 0.91 s, sort 4.94 s, cmp4 0.92 s, cmp2 3.24 s, k0 0.51 s
-- most of it the host's side: building the inputs, the references, the copies (faster runs took 3.6 s for sort and 1.4 s for cmp2).

A child that ends by a signal, an abort, a HIP error (exit status 3) or its time limit is a fault, not a failed assertion: the module
remembers it, and every later group fails at once without starting a process.  Nothing is retried."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPDIR = os.path.join(ROOT, "tests", "hip")
BIN = os.path.join(HIPDIR, "device_units")

# seconds: max(30, 10 x the measured wall time in the docstring)
LIMITS = {"wave": 30, "scan": 30, "sort": 49, "cmp4": 30, "cmp2": 32, "k0": 30}
# cases a group prints (a case dropped from the program shows here); cmp4: 2 functions x 3 widths x 2 flags x 3 placements, each over
# the 64 x 150 lattice; cmp2: 2 placements over the 256 x 241 lattice
CASES = {"wave": 649, "scan": 725, "sort": 6206, "cmp4": 36, "cmp2": 2, "k0": 1054}
LATTICE = {"cmp4": 64 * 150, "cmp2": 256 * 241}

_fault = []  # the first fault of the module


@pytest.fixture(scope="module")
def binary():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.isfile(hipcc) and os.access(hipcc, os.X_OK):
        out = subprocess.run(["make", "-C", HIPDIR], capture_output=True, text=True)  # (nothing to do when the program is fresh)
        assert out.returncode == 0, out.stderr[-4000:]
    if not (os.path.isfile(BIN) and os.access(BIN, os.X_OK)):
        pytest.fail("no hipcc to build tests/hip/device_units with, and build() left no binary")
    return BIN


def run_group(binary, group):
    if _fault:
        pytest.fail(f"not started: {_fault[0]}")
    try:
        p = subprocess.run([binary, group], capture_output=True, text=True, timeout=LIMITS[group])
    except subprocess.TimeoutExpired:
        _fault.append(f"group {group} did not end within its {LIMITS[group]} s")
        pytest.fail(_fault[0])
    lines = p.stdout.splitlines()
    fails = [l for l in lines if l.startswith("FAIL")]
    if p.returncode not in (0, 1):
        _fault.append(f"group {group} ended with status {p.returncode}: {p.stderr.strip()[-500:]}")
        pytest.fail(_fault[0] + "\n" + "\n".join(fails[:40]))
    assert p.returncode == 0 and not fails, f"{len(fails)} case(s) of group {group} failed:\n" + "\n".join(fails[:40])
    oks = [l for l in lines if l.startswith("ok ")]
    assert lines and lines[-1] == f"{group}: {len(oks)} cases, 0 failed", lines[-1:]
    assert len(oks) == CASES[group], (len(oks), CASES[group])
    return oks


def test_wave_and_block_primitives(binary):
    oks = run_group(binary, "wave")
    for name in ("wave_fold/wave_total<DppAdd>", "wave_fold/wave_total<DppMax>", "wave_fold/wave_total<DppMin>", "wave_iscan<u32>", "wave_iscan<u64>",
                 "wave_iscan_dpp", "wave_sum<u64>", "wave_max<u32>", "wave_min<u32>", "block_escan<1,", "block_escan<2,", "block_escan<4,u32,true>",
                 "block_escan_256<u64> twice", "seg_reduce_to_head<Add>", "seg_reduce_to_head<Min>", "seg_reduce_to_head<Max>", "wave_hist_add",
                 "wave_match_digit<0>", "wave_match_digit<9>", "wave_match_digit<10>", "wave_match_digit<11>", "member_of n=31", "make_key/unpack_key raw",
                 "make_key/unpack_key packed lbits=31", "window_reach"):
        assert any(name in l for l in oks), name


def test_generic_scan_both_routes(binary):
    oks = run_group(binary, "scan")
    for n in (0, 1, 255, 256, 257, 2047, 2048, 2049, 2048 * 1024, 2048 * 1024 + 1, 2048 * 4096, 2048 * 4096 + 1):
        assert any(f" n={n} " in l and "route=reduce+tiles+apply" in l for l in oks), n
        assert n > 2048 * 4096 or any(f" n={n} " in l and "route=reduce+apply2" in l for l in oks), n
    for tiles in (1, 1023, 1024, 1025, 2048, 2049, 5000):
        assert f"ok scan scan_tiles_kernel tiles={tiles}" in oks


def test_radix_pass_and_rs_place(binary):
    oks = run_group(binary, "sort")
    for key in ("u32", "u64"):
        for width in ("bits=1 rs_scatter<0>", "bits=4 rs_scatter<0>", "bits=8 rs_scatter<0>", "bits=9 rs_scatter<9>", "bits=9 rs_scatter<0>",
                      "bits=10 rs_scatter<10>", "bits=10 rs_scatter<0>", "bits=11 rs_scatter<11>", "bits=11 rs_scatter<0>", "bits=12 rs_scatter<0>"):
            for n in (1, 63, 64, 65, 4095, 4096, 4097, 64 * 4096, 64 * 4096 + 1, 3 * 4096 + 17):
                assert any(f"sort pass {key} {width} " in l and f" n={n} " in l for l in oks), (key, width, n)
    assert sum("-tiles" in l for l in oks) == 36 and sum(l.startswith("ok sort full ") for l in oks) == 2
    assert sum(l.startswith("ok sort rs_place ") for l in oks) == 8


def test_base_compare_4_bits(binary):
    oks = run_group(binary, "cmp4")
    assert all(f": {LATTICE['cmp4']} lattice points, " in l for l in oks), oks[:3]


def test_base_compare_2_bits(binary):
    oks = run_group(binary, "cmp2")
    assert all(f": {LATTICE['cmp2']} lattice points, " in l for l in oks), oks


def test_k0_kernels(binary):
    oks = run_group(binary, "k0")
    for kernel, least in (("k0_upper", 500), ("k0_encode ", 24), ("k0_encode2", 200), ("k0_fasta", 40)):
        assert sum(f"ok k0 {kernel}" in l for l in oks) >= least, kernel
    assert sum(" bad: " in l for l in oks) == 9


def test_the_limits_follow_the_measured_times():
    measured = dict(re.findall(r"(wave|scan|sort|cmp4|cmp2|k0) ([0-9.]+) s", __doc__))
    assert set(measured) == set(LIMITS)
    for group, seconds in measured.items():
        assert LIMITS[group] == max(30, round(10 * float(seconds))), group
