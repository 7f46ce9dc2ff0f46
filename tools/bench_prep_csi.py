#!/usr/bin/env python3
"""Measurement of the device indexer's CSI mode (`portcullis_amd prep --build_csi`, pjb_index_begin_csi / _piece / _end_csi)
beside the BAI build it shares its kernels with, and of the BAI build against another build of the library (`--other-lib`:
the parent commit's libportcullis_amd.so, built from a checkout of that commit).

Every library gets a worker process of its own that loads the BAM file, makes one context and answers "bai" / "csi" with
the wall time of one index build through the C ABI (the file in host memory, pieces of `--piece-mb`).  The legs alternate
-- other BAI, this BAI, this CSI -- `--reps` times after one warm-up each; medians and spreads go into one JSON line.
The condition recorded with them: this tree's BAI median may exceed the other library's by no more than the other
library's own max - min.  `kernels_ms` is the device time by kernel of one extra CSI build on a context that times its
kernels (never part of the walls).

The input is `--bam` or, without it, the one tools/bench_index.py generates (the BASELINE configs[2] shape scaled to
`--reads` / `--junctions`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def worker(lib_path, bam, piece_mb):
    """Answers lines on stdin ("bai", "csi", "quit") with the seconds one index build took."""
    import numpy as np

    from portcullis_amd import ffi  # (for the file helpers and the structs only: the library is the one named)

    L = C.CDLL(lib_path)
    L.pjb_last_error.restype = C.c_char_p
    L.pjb_last_error.argtypes = [C.c_void_p]
    L.pjb_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(ffi.PjbConfig)]
    L.pjb_destroy.argtypes = [C.c_void_p]
    L.pjb_set_refs.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.pjb_index_begin.argtypes = [C.c_void_p]
    L.pjb_index_piece.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    L.pjb_index_end.argtypes = [C.c_void_p, C.POINTER(ffi.PjbIndexResult)]
    has_csi = hasattr(L, "pjb_index_begin_csi")
    if has_csi:
        L.pjb_index_begin_csi.argtypes = [C.c_void_p, C.c_int32]
        L.pjb_index_end_csi.argtypes = [C.c_void_p, C.POINTER(ffi.PjbCsiResult)]
    data = np.fromfile(bam, dtype=np.uint8)
    starts = np.array(ffi.bgzf_block_starts(memoryview(data)), dtype=np.int64)
    ref_lens, header_bytes = ffi.bam_header(data[: 1 << 26].tobytes(), [int(s) for s in starts[:4096]])
    n_blocks = len(starts) - 1
    block_of = {int(o): k for k, o in enumerate(starts)}
    h = C.c_void_p()
    cfg = ffi.PjbConfig(ffi.ABI_VERSION, 0, 0, 3, ffi.FLAG_NO_CHAINS)

    def check(rc):
        if rc:
            raise SystemExit(f"{lib_path}: {L.pjb_last_error(h).decode(errors='replace')}")

    check(L.pjb_create(C.byref(h), C.byref(cfg)))
    lens = np.ascontiguousarray(ref_lens, dtype=np.int32)
    check(L.pjb_set_refs(h, len(lens), lens.ctypes.data))

    def build(csi):
        check(L.pjb_index_begin_csi(h, -1) if csi else L.pjb_index_begin(h))
        k, uoff, nv = 0, header_bytes, C.c_uint64()
        while True:
            k1 = min(int(np.searchsorted(starts, starts[k] + (piece_mb << 20), side="left")), n_blocks)
            p = data[starts[k]:starts[k1]]
            check(L.pjb_index_piece(h, p.ctypes.data_as(C.c_void_p), len(p), int(starts[k]), uoff, int(k1 == n_blocks), C.byref(nv)))
            if k1 == n_blocks:
                break
            k, uoff = block_of[nv.value >> 16], nv.value & 0xFFFF
        if csi:
            r = ffi.PjbCsiResult()
            check(L.pjb_index_end_csi(h, C.byref(r)))
        else:
            r = ffi.PjbIndexResult()
            check(L.pjb_index_end(h, C.byref(r)))
        return r

    build(False)  # warm-up
    if has_csi:
        build(True)
    print(f"ready {len(data)}", flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        t0 = time.perf_counter()
        r = build(cmd == "csi")
        print(f"{time.perf_counter() - t0:.6f} {r.n_records} {r.n_chunks} {getattr(r, 'depth', -1)}", flush=True)
    L.pjb_destroy(h)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bam", help="a coordinate-sorted BAM file (default: the one tools/bench_index.py generates)")
    ap.add_argument("--other-lib", help="another build of libportcullis_amd.so whose BAI build is the yardstick (the parent commit's)")
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--junctions", type=int, default=25_000)
    ap.add_argument("--workdir", default=os.environ.get("PJB_BENCH_INDEX_WORKDIR", "/tmp/pjb_bench_index"))
    ap.add_argument("--piece-mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    bam = args.bam
    if not bam:  # (generated with torch, which wants to be the first to open the device in its process)
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench_prep_csi.py needs an MI355X (no CPU fallback)")
        import bench_index

        bam, _ = bench_index.make_bam(args.workdir, args.reads, args.junctions)

    from portcullis_amd import ffi

    if ffi.device_count() <= 0:
        raise SystemExit("bench_prep_csi.py needs an MI355X (no CPU fallback)")

    def start(lib):
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", lib, bam, str(args.piece_mb)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                             text=True)
        line = p.stdout.readline()
        if not line.startswith("ready"):
            raise SystemExit(f"the worker for {lib} did not start")
        return p

    def ask(p, what):
        p.stdin.write(what + "\n")
        p.stdin.flush()
        f = p.stdout.readline().split()
        if len(f) != 4:
            raise SystemExit("a worker ended early")
        return float(f[0]), int(f[1]), int(f[2]), int(f[3])

    this = start(ffi.LIB_PATH)
    other = start(args.other_lib) if args.other_lib else None
    t_other, t_bai, t_csi, shape = [], [], [], {}
    for _ in range(args.reps):
        if other:
            t_other.append(ask(other, "bai")[0])
        s, n, ch, _ = ask(this, "bai")
        t_bai.append(s)
        shape.update(records=n, bai_chunks=ch)
        s, n, ch, depth = ask(this, "csi")
        t_csi.append(s)
        shape.update(csi_chunks=ch, csi_depth=depth)
    for p in (this, other):
        if p:
            p.stdin.write("quit\n")
            p.stdin.flush()
            p.wait()

    # device time by kernel, one CSI build on a timed context
    import numpy as np

    data = np.fromfile(bam, dtype=np.uint8)
    starts = np.array(ffi.bgzf_block_starts(memoryview(data)), dtype=np.int64)
    ref_lens, header_bytes = ffi.bam_header(data[: 1 << 26].tobytes(), [int(s) for s in starts[:4096]])
    n_blocks = len(starts) - 1
    block_of = {int(o): k for k, o in enumerate(starts)}
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS | ffi.FLAG_KERNEL_TIMING) as c:
        c.set_refs(ref_lens)
        c.index_begin(-1)
        k, uoff = 0, header_bytes
        while True:
            k1 = min(int(np.searchsorted(starts, starts[k] + (args.piece_mb << 20), side="left")), n_blocks)
            nv = c.index_piece(data[starts[k]:starts[k1]], int(starts[k]), uoff, k1 == n_blocks)
            if k1 == n_blocks:
                break
            k, uoff = block_of[nv >> 16], nv & 0xFFFF
        c.index_end_csi()
        kt = c.kernel_timing()
    kernels_ms = {name: [int(n), round(ms, 4)] for name, (n, ms) in sorted(kt.items()) if name.startswith(("bai_", "csi_"))}
    new_ms = round(sum(ms for name, (_, ms) in kt.items() if name.startswith("csi_")), 4)

    def stats(v):
        return dict(median_s=round(statistics.median(v), 4), min_s=round(min(v), 4), max_s=round(max(v), 4), runs_s=[round(x, 4) for x in v])

    line = dict(metric="bam_csi_build", bam_bytes=int(len(data)), piece_mb=args.piece_mb, **shape, bai=stats(t_bai), csi=stats(t_csi),
                kernels_ms=kernels_ms, new_kernels_ms=new_ms,
                note="kernels_ms: [launches, device ms] by kernel from one extra CSI build on a timed context; csi_* are the new kernels "
                     "(bai_win_reduce and bai_win_tiles also run once more over the windows at the end of a CSI build)")
    if other:
        so = stats(t_other)
        spread = so["max_s"] - so["min_s"]
        line["other_bai"] = so
        line["condition"] = dict(rule="bai.median_s - other_bai.median_s <= other_bai.max_s - other_bai.min_s", excess_s=round(line["bai"]["median_s"] - so["median_s"], 4),
                                 allowed_s=round(spread, 4), holds=bool(line["bai"]["median_s"] - so["median_s"] <= spread))
    txt = json.dumps(line)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
