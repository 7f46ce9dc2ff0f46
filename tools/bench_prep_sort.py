#!/usr/bin/env python3
"""Measurement of `portcullis_amd prep --sort` (pjb_bam_sort_begin / _piece / _end), one JSON document on stdout (and in --out):

- the input: the C2 BAM of tests/e2e_bench.py (10 M reads on one target) with its records shuffled in blocks of `--block` records
  (the blocks permuted, the order inside a block kept), written as one BAM without an index beside it;
- wall time of `prep --sort -t T` on it, alternating with its two neighbours -- `prep` on the sorted file (link + index build) and
  `prep --merge` on the sorted file split `--files` ways round-robin by record (tools/bench_prep_merge.py's split) --, `--reps` runs
  each into fresh directories after one dropped warm-up round, a host clock around the process and a pause of `--pause` seconds
  before every run;
- one run of `prep --sort` with PORTCULLIS_SORT_RUN_BYTES set so that the file becomes `--runs` runs that the merge then joins:
  what the run-then-merge route costs;
- what `prep --sort -v` says the device held at most during a run of the default size;
- device time per launch name of one run through ffi (a context that times its kernels): keys, sort, scan, gather, deflate, beside
  the inflate; and the gather's rate: (bytes read + bytes written) / device time of mg_gather.

Needs an MI355X; nothing here falls back to the CPU.  Shuffle and split run on the host (numpy) and are not timed."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_prep_merge import EOF_BLOCK, EXE, PREP_BAM, PREP_FA, deflate_to, inflate_file, split  # noqa: E402


def shuffle(ctx, ffi, bam, block, workdir, seed=1):
    """The records of `bam` in blocks of `block` records, the blocks in random order -> (path, records, raw record bytes, how)"""
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
    n_rec = len(offs) - 1
    order = np.random.default_rng(seed).permutation((n_rec + block - 1) // block)
    p = os.path.join(workdir, "shuffled.bam")
    with open(p, "wb") as out:
        deflate_to(ctx, out, header)
        for b in order:  # (a block of records is one stretch of the stream)
            deflate_to(ctx, out, body[offs[b * block]:offs[min((b + 1) * block, n_rec)]])
        out.write(EOF_BLOCK)
    return p, n_rec, int(n), f"the file's {n_rec} alignment records in blocks of {block}, the {len(order)} blocks permuted (numpy default_rng({seed})), the order inside a block kept; no index beside it"


def timed(pause, *args, env_extra=None):
    time.sleep(pause)
    env = dict(os.environ, **(env_extra or {}))
    t = time.time()
    p = subprocess.run([EXE, *args], capture_output=True, text=True, env=env)
    w = time.time() - t
    if p.returncode != 0:
        raise SystemExit(p.stdout[-2000:] + p.stderr[-2000:])
    return w, p.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", default="/tmp/pjb_prep_sort")
    ap.add_argument("--config", default="C2")
    ap.add_argument("--block", type=int, default=65536)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pause", type=float, default=1.0)
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
    res = dict(input=f"tests/e2e_bench.py --config {a.config}: BAM {os.path.getsize(whole) / 1e6:.1f} MB", threads=a.threads, pause_s=a.pause)
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as ctx:
        shuffled, n_rec, raw_bytes, how = shuffle(ctx, ffi, whole, a.block, wd)
        paths, _, _, how_split = split(ctx, ffi, whole, a.files, wd)
    res.update(shuffle=how, split=how_split, records=n_rec, raw_record_bytes=raw_bytes, shuffled_mb=round(os.path.getsize(shuffled) / 1e6, 1))
    # ---- wall time, alternating
    sort_s, floor_s, merge_s, verbose = [], [], [], ""
    t = str(a.threads)
    for rep in range(a.reps + 1):  # (the first round warms the page cache and is dropped)
        s, verbose = timed(a.pause, "prep", "--sort", "-v", "-t", t, "-o", os.path.join(wd, f"s{rep}"), fa, shuffled)
        f, _ = timed(a.pause, "prep", "-o", os.path.join(wd, f"f{rep}"), fa, whole)
        m, _ = timed(a.pause, "prep", "--merge", "-t", t, "-o", os.path.join(wd, f"m{rep}"), fa, *paths)
        if rep:
            sort_s.append(round(s, 3))
            floor_s.append(round(f, 3))
            merge_s.append(round(m, 3))
        for d in ("s", "m"):
            shutil.rmtree(os.path.join(wd, f"{d}{rep}"))
    summary = lambda v: dict(runs_s=v, median_s=statistics.median(v), range_s=[min(v), max(v)])
    res.update(prep_sort=summary(sort_s), prep_sorted_file=summary(floor_s), prep_merge_split=summary(merge_s))
    held = re.search(r"the device held at most (\d+) bytes", verbose)
    res["default_run_device_peak_bytes"] = int(held.group(1)) if held else None
    res["default_run_verbose"] = [line.strip() for line in verbose.splitlines() if "sort run" in line or "sorted:" in line]
    # ---- the run-then-merge route
    w, out = timed(a.pause, "prep", "--sort", "-v", "-t", t, "-o", os.path.join(wd, "runs"), fa, shuffled,
                   env_extra={"PORTCULLIS_SORT_RUN_BYTES": str(os.path.getsize(shuffled) // a.runs + 1)})
    n_runs = re.search(r"in (\d+) runs?;", out)
    res["runs_then_merge"] = dict(run_bytes=os.path.getsize(shuffled) // a.runs + 1, runs=int(n_runs.group(1)) if n_runs else None, wall_s=round(w, 3))
    shutil.rmtree(os.path.join(wd, "runs"))
    # ---- device time per launch name
    with ffi.Context(flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as ctx:
        d = np.frombuffer(open(shuffled, "rb").read(), dtype=np.uint8)
        ctx.bam_sort(d.tobytes(), piece_blocks=4096)  # warm-up: code objects, buffers
        ctx.reset_kernel_timing()
        out = ctx.bam_sort(d.tobytes(), piece_blocks=4096)
        kt = ctx.kernel_timing()
        mem = ctx.memory_info()
        res["sort_device_ms"] = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in sorted(kt.items())}
        assert out["n_records"] == n_rec and out["raw_bytes"] == raw_bytes and out["was_sorted"] == 0, (out["n_records"], out["raw_bytes"])
        ms = lambda *names: sum(v[1] for k, v in kt.items() if k.startswith(names))
        g = kt["mg_gather"][1]
        res.update(inflate_ms=round(ms("bgzf_decode", "bgzf_resolve"), 3), keys_ms=round(ms("sr_keys"), 3), sort_ms=round(ms("rs_"), 3), scan_ms=round(ms("sr_off"), 3),
                   gather_ms=round(g, 3), deflate_ms=round(ms("bgzf_deflate", "bgzf_pack"), 3),
                   gather_GB_per_s=round(2 * raw_bytes / (g * 1e-3) / 1e9, 1), gather_of_8TBps_hbm_peak=round(2 * raw_bytes / (g * 1e-3) / 8e12, 3),
                   merge_gather_GB_per_s_recorded=1200.0, ffi_run_peak_held_bytes=mem.get("peak_held"))
    res["not_measured"] = "the 33.5 GB input; inputs of many targets; counters of sr_keys and mg_gather"
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    shutil.rmtree(wd, ignore_errors=True)


if __name__ == "__main__":
    main()
