"""The C-ABI library loads (no GPU needed) and exports every function include/portcullis_amd.h
declares; struct sizes seen from Python match the header."""
import ctypes
import os

import pytest
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "portcullis_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pjb_[a-z_]+)\s*\(", hdr))
    assert {"pjb_create", "pjb_submit_batch", "pjb_finish_contig", "pjb_collect"} <= declared
    from portcullis_amd import ffi

    lib = ffi.load()
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, missing
    assert set(ffi.EXPORTS) == declared


def test_struct_sizes():
    from portcullis_amd import ffi

    assert ffi.ROW_DTYPE.itemsize == 200
    assert ctypes.sizeof(ffi.PjbBatch) == 8 + 14 * 8  # (ABI 4: + seq2, seq_exc)
    assert ffi.EXTRA_DTYPE.itemsize == 24
    assert ctypes.sizeof(ffi.PjbRegionResult) == 56
    assert ctypes.sizeof(ffi.PjbConfig) == 20


def test_struct_sizes_match_the_header_compiled(tmp_path):
    """sizeof of every struct the stub mirrors, as gcc sees it in include/portcullis_amd.h (pjb_timing grew in ABI 3)."""
    import subprocess
    from portcullis_amd import ffi

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "portcullis_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(pjb_timing), '
                   'sizeof(pjb_batch), sizeof(pjb_region_result), sizeof(pjb_config), sizeof(pjb_junction_row), PJB_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    timing, batch, region, config, row, abi = (int(x) for x in out)
    assert timing == ctypes.sizeof(ffi.PjbTiming)
    assert batch == ctypes.sizeof(ffi.PjbBatch) and region == ctypes.sizeof(ffi.PjbRegionResult) and config == ctypes.sizeof(ffi.PjbConfig)
    assert row == ffi.ROW_DTYPE.itemsize and abi == ffi.ABI_VERSION


def test_no_device_is_a_loud_error():
    """Without a GPU pjb_create must fail with PJB_ERR_NO_DEVICE -- there is no CPU fallback."""
    from portcullis_amd import ffi

    if ffi.device_count() > 0:
        return
    try:
        ffi.Context(0)
    except ffi.PjbError as e:
        assert e.code == -18 and "no CPU fallback" in str(e)
    else:
        raise AssertionError("pjb_create succeeded without a device")


def test_no_device_is_the_same_loud_error_on_every_ingest_route(tmp_path):
    """Without a GPU `portcullis_amd junc` must leave with status 4 and the context's own message whichever way the targets' bytes
    would have travelled: host decode, the whole-target block, file pieces (which must not read the file for a device that is not there)."""
    import subprocess

    from fuzzgen import make_reads
    from portcullis_amd import ffi
    from util_bam import make_prep_dir

    if ffi.device_count() > 0:
        return
    exe = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
    if not os.path.exists(exe):
        pytest.skip("host program not built")
    refs, contigs, reads = [], [], []
    for tid in range(3):
        genome, rr = make_reads(70 + tid, n_reads=300, glen=20000 + 1000 * tid)
        for r in rr:
            r["tid"] = tid
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    prep = make_prep_dir(str(tmp_path / "prep"), refs, contigs, reads)
    for ingest, env_extra in (("host", {}), ("device", {}), ("device", {"PORTCULLIS_PIECE_BYTES": "4096"})):
        env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
        env.update(env_extra)
        p = subprocess.run([exe, "junc", "-t", "3", "--ingest", ingest, "-o", str(tmp_path / "out" / "pc"), prep],
                           capture_output=True, text=True, timeout=10, env=env)
        assert p.returncode == 4, (ingest, env_extra, p.returncode, p.stderr[-500:])
        assert "No MI355X (HIP device) is visible" in p.stderr, (ingest, env_extra, p.stderr[-500:])


def test_host_library_builds_and_links():
    host = os.path.join(ROOT, "portcullis_amd", "host")
    assert os.path.exists(os.path.join(host, "libportcullis_host.so"))
    ctypes.CDLL(os.path.join(host, "libportcullis_host.so"))


def test_c_caller_of_plan_groups_and_merge_rows(tmp_path):
    """A plain C program (gcc, no HIP headers) links the library and calls the two host-arithmetic entry points of ABI 4 -- the chain plan and
    the receive side of the multi-GPU merge -- without a context or a device: tests/cpp/merge_plan_check.c."""
    import subprocess

    lib_dir = os.path.join(ROOT, "portcullis_amd", "csrc")
    if not os.path.exists(os.path.join(lib_dir, "libportcullis_amd.so")):
        pytest.skip("library not built")
    exe = tmp_path / "merge_plan_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "merge_plan_check.c"),
                    "-L", lib_dir, "-lportcullis_amd", f"-Wl,-rpath,{lib_dir}"], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
