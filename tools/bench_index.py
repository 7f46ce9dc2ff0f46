#!/usr/bin/env python3
"""Measurement of the device BAM indexer (`portcullis_amd prep`, pjb_index_begin / _piece / _end): the wall time of the index
build through ffi over a BAM file held in host memory, beside the wall time of the inflate alone (pjb_inflate_bgzf) over the
same pieces -- the part of the work no indexer can avoid.  The two legs alternate, both are warmed up first; the medians and
the spread of `--reps` runs each are reported in one JSON line, and the wall of the `prep` program on the same file (a host
clock around the process) beside them.

The input is `--bam` (e.g. the BAM `bench.py --full` leaves in its work directory) or, without it, a BAM of the BASELINE
configs[2] shape scaled to `--reads` / `--junctions`, written as bench.py's end-to-end leg writes it (synth -> tools/soa2bam).

Note on the inflate leg: pjb_inflate_bgzf also copies the inflated bytes back to the host (that is its contract), which the
indexer does not do; `kernels_s`, from a context that times its kernels, is the device time by kernel family (inflate, record walk, index)."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_bam(workdir, reads, junctions):
    """A prepared directory of the configs[2] shape, as bench.py's e2e leg writes it; returns (bam, genome)."""
    import torch

    from portcullis_amd import synth

    prep = os.path.join(workdir, "prep")
    bam = os.path.join(prep, "portcullis.sorted.alignments.bam")
    fa = os.path.join(prep, "portcullis.genome.fa")
    tag = os.path.join(workdir, f"made_{reads}_{junctions}")
    if os.path.exists(tag) and os.path.exists(bam):
        return bam, fa
    shutil.rmtree(workdir, ignore_errors=True)
    os.makedirs(prep)
    ext = dict(pos="i32", flag="u16", mapq="u8", xs="u8", l_qseq="i32", mtid="i32", mpos="i32", cig_off="u32", cigar="u32", seq_off="u32", seq4="u8")
    dirs = []
    for tid, cfg in enumerate(synth.c3_contig_configs(reads, junctions)):
        d = synth.generate(cfg, device="cuda", tid=tid)
        sub = os.path.join(workdir, f"contig{tid}")
        os.makedirs(sub)
        open(os.path.join(sub, "name.txt"), "w").write(synth.GRCH38_NAMES[tid])
        d["genome"].cpu().numpy().tofile(os.path.join(sub, "genome.u8"))
        for k, e in ext.items():
            d["batch"][k].cpu().numpy().tofile(os.path.join(sub, f"{k}.{e}"))
        dirs.append(sub)
        del d
        torch.cuda.empty_cache()
    exe = os.path.join(ROOT, "tools", "soa2bam")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "soa2bam.cc"), "-lz", "-lpthread"])
    subprocess.check_call([exe, prep, str(min(16, os.cpu_count() or 1))] + dirs, stdout=subprocess.DEVNULL)
    for sub in dirs:
        shutil.rmtree(sub, ignore_errors=True)
    os.sync()
    open(tag, "w").write("ok")
    return bam, fa


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bam", help="a coordinate-sorted BAM file (default: one is generated)")
    ap.add_argument("--genome", help="its genome FASTA, for the timing of the `prep` program (generated BAMs bring theirs)")
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--junctions", type=int, default=25_000)
    ap.add_argument("--workdir", default=os.environ.get("PJB_BENCH_INDEX_WORKDIR", "/tmp/pjb_bench_index"))
    ap.add_argument("--piece-mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    import numpy as np
    import torch

    from portcullis_amd import ffi

    if not torch.cuda.is_available() or ffi.device_count() <= 0:
        raise SystemExit("bench_index.py needs an MI355X (no CPU fallback)")
    bam, fa = (args.bam, args.genome) if args.bam else make_bam(args.workdir, args.reads, args.junctions)
    data = np.fromfile(bam, dtype=np.uint8)
    raw = data.tobytes() if len(data) < (1 << 28) else None  # (the header reader wants bytes; large files: only their head)
    head = raw if raw is not None else data[: 1 << 26].tobytes()
    starts = np.array(ffi.bgzf_block_starts(raw if raw is not None else memoryview(data)), dtype=np.int64)
    ref_lens, header_bytes = ffi.bam_header(head, [int(s) for s in starts[:4096]])
    isize = int(sum(int.from_bytes(data[int(e) - 4:int(e)].tobytes(), "little") for e in starts[1:]))
    piece_bytes = args.piece_mb << 20
    block_of = {int(o): k for k, o in enumerate(starts)}
    n_blocks = len(starts) - 1

    def piece_end(k):  # the first block start at least piece_bytes behind block k
        return min(int(np.searchsorted(starts, starts[k] + piece_bytes, side="left")), n_blocks)

    # room for the inflated bytes of the piece with the most blocks (a block inflates to 64 KB at most)
    ends = np.minimum(np.searchsorted(starts, starts[:-1] + piece_bytes, side="left"), n_blocks)
    out = np.empty((int((ends - np.arange(n_blocks)).max()) + 1) * 65536, dtype=np.uint8)

    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as ctx, ffi.Context(flags=ffi.FLAG_NO_CHAINS | ffi.FLAG_KERNEL_TIMING) as tctx:
        ctx.set_refs(ref_lens)
        L, h = ctx._L, ctx._h
        pieces_used = []

        def index_leg(c=ctx):
            c.index_begin()
            k, uoff, pieces = 0, header_bytes, []
            while True:
                k1 = piece_end(k)
                pieces.append((k, k1))
                nv = c.index_piece(data[starts[k]:starts[k1]], int(starts[k]), uoff, k1 == n_blocks)
                if k1 == n_blocks:
                    break
                k, uoff = block_of[nv >> 16], nv & 0xFFFF
            res = c.index_end()
            return res, pieces

        def inflate_leg(pieces):
            n = C.c_int64()
            for k, k1 in pieces:
                p = data[starts[k]:starts[k1]]
                rc = L.pjb_inflate_bgzf(h, p.ctypes.data_as(C.c_void_p), len(p), out.ctypes.data_as(C.c_void_p), len(out), C.byref(n))
                if rc:
                    raise SystemExit(f"pjb_inflate_bgzf: {L.pjb_last_error(h).decode()}")

        res, pieces_used = index_leg()  # warm-up of both legs
        n_records, n_chunks = int(res["n_records"]), len(res["chunks"])
        inflate_leg(pieces_used)
        t_index, t_inflate = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            index_leg()
            t_index.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            inflate_leg(pieces_used)
            t_inflate.append(time.perf_counter() - t0)
        # device time per kernel family, one more run on a context that brackets every launch (never part of the walls above)
        tctx.set_refs(ref_lens)
        tctx.reset_kernel_timing()
        index_leg(tctx)
        kt = tctx.kernel_timing()
        fam = {"inflate": ("bgzf_",), "walk": ("bam_",), "index": ("bai_",)}
        kernels_s = {f: round(sum(ms for name, (_, ms) in kt.items() if name.startswith(pre)) / 1e3, 4) for f, pre in fam.items()}

    prep_wall = None
    exe = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
    if fa and os.path.exists(exe):
        runs = []
        for _ in range(3):
            d = os.path.join(args.workdir, "prep_timing")
            shutil.rmtree(d, ignore_errors=True)
            src = os.path.join(args.workdir, "prep_in.bam")  # (a link without an index beside it: the index must be built)
            if os.path.lexists(src):
                os.unlink(src)
            os.makedirs(args.workdir, exist_ok=True)
            os.symlink(os.path.realpath(bam), src)
            t0 = time.perf_counter()
            p = subprocess.run([exe, "prep", "-o", d, fa, src], capture_output=True, text=True)
            runs.append(time.perf_counter() - t0)
            if p.returncode != 0:
                raise SystemExit("prep failed: " + p.stderr[-800:])
        prep_wall = dict(median_s=round(statistics.median(runs), 3), runs_s=[round(x, 3) for x in runs])

    def stats(v):
        return dict(median_s=round(statistics.median(v), 4), min_s=round(min(v), 4), max_s=round(max(v), 4), runs_s=[round(x, 4) for x in v])

    mi, mf = statistics.median(t_index), statistics.median(t_inflate)
    line = dict(metric="bam_index_build", bam_bytes=int(len(data)), inflated_bytes=isize, records=n_records, chunks=n_chunks, pieces=len(pieces_used),
                piece_mb=args.piece_mb, index=stats(t_index), inflate_only=stats(t_inflate), index_over_inflate=round(mi / mf, 3),
                compressed_GBps=round(len(data) / mi / 1e9, 2), inflated_GBps=round(isize / mi / 1e9, 2), kernels_s=kernels_s, prep_program=prep_wall,
                note="inflate_only is pjb_inflate_bgzf (its D2H copy of the inflated bytes included); kernels_s: device time by kernel family from one extra timed run")
    txt = json.dumps(line)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
