#!/usr/bin/env python3
"""Measurement of `portcullis_amd prep --merge` (pjb_bam_merge_begin / _file / _end), one JSON document on stdout (and in --out):

- the input: the C2 BAM of tests/e2e_bench.py (10 M reads on one target), split stably into `--files` files round-robin by record
  (record k goes to file k mod files), each written without an index beside it;
- wall time of `prep --merge -t T` on the split files, alternating with `prep` on the unsplit file (link + index build: the
  floor), `--reps` runs each into fresh directories, a host clock around the process;
- device time per launch name (a context that times its kernels, through ffi): the merge of the one target, and the index pass
  over the merged file afterwards;
- the gather's rate: (bytes read + bytes written) / device time of mg_gather.

Needs an MI355X; nothing here falls back to the CPU.  The split runs on the host (numpy) and is not timed."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
PREP_BAM, PREP_FA = "portcullis.sorted.alignments.bam", "portcullis.genome.fa"
BLOCK = 0xFF00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def inflate_file(ctx, data, starts, piece_blocks=4096):
    out = []
    for k in range(0, len(starts) - 1, piece_blocks):
        out.append(np.frombuffer(ctx.inflate_bgzf(data[starts[k]:starts[min(k + piece_blocks, len(starts) - 1)]]), dtype=np.uint8))
    return np.concatenate(out)


def deflate_to(ctx, f, raw, piece_blocks=4096):
    step = piece_blocks * BLOCK
    for at in range(0, len(raw), step):
        members, _ = ctx.deflate_bgzf(raw[at:at + step].tobytes(), BLOCK)
        f.write(members)


def split(ctx, ffi, bam, n_files, workdir):
    """-> (paths, records, raw record bytes, how)"""
    data = open(bam, "rb").read()
    starts = ffi.bgzf_block_starts(data)
    _, head = ffi.bam_header(data, starts)
    raw = inflate_file(ctx, data, starts)
    header, body = raw[:head], raw[head:]
    offs, o, n = [], 0, len(body)
    view = memoryview(body)
    while o < n:
        offs.append(o)
        o += 4 + int.from_bytes(view[o:o + 4], "little")
    offs = np.array(offs + [n], dtype=np.int64)
    sizes = np.diff(offs)
    paths = []
    for f in range(n_files):
        p = os.path.join(workdir, f"split{f}.bam")
        with open(p, "wb") as out:
            deflate_to(ctx, out, header)
            idx = np.arange(f, len(sizes), n_files)
            for c in range(0, len(idx), 1 << 18):  # a quarter of a million records at a time
                i = idx[c:c + (1 << 18)]
                sz = sizes[i]
                dst = np.concatenate([[0], np.cumsum(sz)])
                take = np.repeat(offs[i] - dst[:-1], sz) + np.arange(dst[-1], dtype=np.int64)
                deflate_to(ctx, out, body[take])
            out.write(EOF_BLOCK)
        paths.append(p)
    return paths, len(sizes), int(n), f"record k of the file's {len(sizes)} alignment records goes to file k mod {n_files}; every file keeps the header; members of {BLOCK} bytes, written by pjb_deflate_bgzf; no index beside any of them"


def timed(*args):
    t = time.time()
    p = subprocess.run([EXE, *args], capture_output=True, text=True)
    w = time.time() - t
    if p.returncode != 0:
        raise SystemExit(p.stdout[-2000:] + p.stderr[-2000:])
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default="/tmp/pjb_prep_merge")
    ap.add_argument("--config", default="C2")
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from portcullis_amd import ffi

    wd = a.workdir
    shutil.rmtree(wd, ignore_errors=True)
    os.makedirs(wd)
    e2e = os.path.join(wd, "e2e")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "e2e_bench.py"), "--config", a.config, "--threads", str(a.threads), "--workdir", e2e,
                           "--keep", "--no-oracle", "--repeat", "1"], stdout=subprocess.DEVNULL)
    bam, fa = os.path.join(e2e, "prep", PREP_BAM), os.path.join(e2e, "prep", PREP_FA)
    whole = os.path.join(wd, "whole.bam")  # (no index beside it: prep builds one)
    shutil.copyfile(bam, whole)
    res = dict(input=f"tests/e2e_bench.py --config {a.config}: BAM {os.path.getsize(whole) / 1e6:.1f} MB", threads=a.threads)
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as ctx:
        paths, n_rec, raw_bytes, how = split(ctx, ffi, whole, a.files, wd)
    res.update(split=how, records=n_rec, raw_record_bytes=raw_bytes, split_mb=[round(os.path.getsize(p) / 1e6, 1) for p in paths])
    # ---- wall time, alternating
    merge_s, floor_s = [], []
    for rep in range(a.reps + 1):  # (the first pair warms the page cache and is dropped)
        m = timed("prep", "--merge", "-t", str(a.threads), "-o", os.path.join(wd, f"m{rep}"), fa, *paths)
        f = timed("prep", "-o", os.path.join(wd, f"f{rep}"), fa, whole)
        if rep:
            merge_s.append(round(m, 3))
            floor_s.append(round(f, 3))
        if rep < a.reps:
            shutil.rmtree(os.path.join(wd, f"m{rep}"))
    res.update(prep_merge_s=merge_s, prep_merge_median_s=statistics.median(merge_s), prep_merge_range_s=[min(merge_s), max(merge_s)],
               prep_unsplit_s=floor_s, prep_unsplit_median_s=statistics.median(floor_s), prep_unsplit_range_s=[min(floor_s), max(floor_s)])
    merged = os.path.join(wd, f"m{a.reps}", PREP_BAM)
    # ---- device time per launch name
    with ffi.Context(flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as ctx:
        shares = []
        for p in paths:
            d = open(p, "rb").read()
            lens, head = ffi.bam_header(d)
            shares.append((np.frombuffer(d, dtype=np.uint8), head))
        ctx.set_refs(lens)
        ctx.bam_merge(0, shares)  # warm-up: code objects, buffers
        ctx.reset_kernel_timing()
        out = ctx.bam_merge(0, shares)
        kt = ctx.kernel_timing()
        res["merge_device_ms"] = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in sorted(kt.items())}
        assert out["n_records"] == n_rec and out["raw_bytes"] == raw_bytes, (out["n_records"], out["raw_bytes"])
        ms = lambda *names: sum(v[1] for k, v in kt.items() if k.startswith(names))
        inflate, order = ms("bgzf_decode", "bgzf_resolve"), ms("mg_keys", "rs_", "mg_off", "mg_gather")
        g = kt["mg_gather"][1]
        res.update(inflate_ms=round(inflate, 3), keys_sort_scan_gather_ms=round(order, 3), sort_ms=round(ms("rs_"), 3), deflate_ms=round(ms("bgzf_deflate", "bgzf_pack"), 3),
                   claim_keys_sort_gather_below_inflate=bool(order < inflate),
                   gather_GB_per_s=round(2 * raw_bytes / (g * 1e-3) / 1e9, 1), gather_of_8TBps_hbm_peak=round(2 * raw_bytes / (g * 1e-3) / 8e12, 3))
        ctx.reset_kernel_timing()
        ctx.index_bam(merged)
        kt = ctx.kernel_timing()
        res["index_pass_device_ms"] = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in sorted(kt.items())}
        res["index_pass_total_ms"] = round(sum(v[1] for v in kt.values()), 3)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    shutil.rmtree(wd, ignore_errors=True)


if __name__ == "__main__":
    main()
