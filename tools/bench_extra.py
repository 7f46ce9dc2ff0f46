#!/usr/bin/env python3
"""Measurement of `junc --extra`: two targets of the BASELINE configs[1] shape through a
PJB_FLAG_EXTRA context (per-target depth of the unspliced records, flanking alignment counts, name codes; then
pjb_extra_finish: multiple-mapping score and coverage of every junction), against the same targets without the flag.
Parity with the oracle is checked on a 2 x 2 M-read copy of the workload (the oracle's pileup is per base and per
record); the timing runs on 2 x 10 M reads.  Prints one JSON line.

  --targets K (K >= 2): the many-target workload instead -- K targets of the configs[1] shape, scaled (--reads-per-target,
--contig-len, --junctions) -- finished in the chains of --plan: `targets` (a chain per target), `groups` (the chains pjb_plan_groups
makes with --group-bases) or `targets,groups` (one context per plan, their timed runs alternating: the comparison that decides the
program's default).  The plain step (no flag, the planner's groups) is timed beside them for the ratio; rows and extra rows of the
plans must be the same bytes."""
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make(cfg, synth, torch, seeds=(1, 2)):
    out = []
    for tid, seed in enumerate(seeds):
        d = synth.generate(dataclasses.replace(cfg, seed=seed), device="cuda", tid=tid)
        g = torch.Generator(device="cuda")
        g.manual_seed(100 + seed)
        n = d["n_reads"]
        # a fifth of the records share their name code with another record (multi-mapped fragments, also across targets)
        codes = torch.randint(1, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)
        dup = torch.rand(n, device="cuda", generator=g) < 0.2
        codes = torch.where(dup, codes % 50021 + 7, codes)
        d["batch"]["name_hash"] = codes
        out.append(d)
    torch.cuda.synchronize()
    return out


def run_device(ffi, torch, data, lens, extra, reps):
    flags = ffi.FLAG_EXTRA if extra else 0
    best = None
    with ffi.Context(0, "UNKNOWN", flags=flags) as ctx:
        ctx.set_refs(lens)
        for tid, d in enumerate(data):
            ctx.upload_contig_device(tid, d["genome"])
        for _ in range(reps + 1):
            ctx.clear_rows()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for tid, d in enumerate(data):   # both targets' chains queued: they run side by side (with and without the flag)
                ctx.submit_batch_device(tid, d["batch"], d["n_reads"])
                ctx.finish_contig_begin(tid)
            for tid in range(len(data)):
                ctx.finish_contig_end(tid)
            rows = ctx.collect(copy=False)  # (waits for the rows' DMA; the table stays in the context's page-locked memory)
            xr = ctx.extra_finish(copy=False) if extra else None
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            rows = rows.copy()
            xr = xr.copy() if extra else None
    return rows, xr, best


def run_chains(ffi, torch, ctx, data, chains, extra, queue):
    """One step: the chains queued `queue` at a time.  -> rows, extra rows (views of the context's tables), seconds"""
    ctx.clear_rows()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    queued = []

    def collect_oldest():
        g = queued.pop(0)
        if len(g) == 1:
            ctx.finish_contig_end(g[0])
        else:
            ctx.finish_group_end(g)

    for g in chains:
        for tid in g:
            ctx.submit_batch_device(tid, data[tid]["batch"], data[tid]["n_reads"])
        if len(g) == 1:
            ctx.finish_contig_begin(g[0])
        else:
            ctx.finish_group_begin(g)
        queued.append(g)
        if len(queued) >= queue:
            collect_oldest()
    while queued:
        collect_oldest()
    rows = ctx.collect(copy=False)
    xr = ctx.extra_finish(copy=False) if extra else None
    return rows, xr, time.perf_counter() - t0


def many_targets(args):
    import statistics

    import torch

    from portcullis_amd import ffi, synth

    cfg = dataclasses.replace(synth.CONFIGS["C2"], n_reads=args.reads_per_target, contig_len=args.contig_len, n_junctions=args.junctions)
    data = make(cfg, synth, torch, seeds=tuple(range(1, args.targets + 1)))
    lens = [cfg.contig_len] * args.targets
    tids = list(range(args.targets))
    groups = ffi.plan_groups(lens, tids, args.group_bases)
    plans = {"targets": [[t] for t in tids], "groups": groups}
    legs = [("plain", False, groups)] + [(p, True, plans[p]) for p in args.plan.split(",")]
    ctxs, times, out = {}, {}, {}
    try:
        for name, extra, chains in legs:
            ctx = ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_EXTRA if extra else 0)
            ctx.set_refs(lens)
            for tid, d in enumerate(data):
                ctx.upload_contig_device(tid, d["genome"])
            ctxs[name] = ctx
            rows, xr, _ = run_chains(ffi, torch, ctx, data, chains, extra, args.queue)  # (warm-up: the context's buffers)
            out[name] = (rows.tobytes(), xr.tobytes() if extra else None)
            times[name] = []
        for _ in range(args.runs):  # (alternating: whatever drifts on the machine meets every leg alike)
            for name, extra, chains in legs:
                times[name].append(run_chains(ffi, torch, ctxs[name], data, chains, extra, args.queue)[2])
    finally:
        for ctx in ctxs.values():
            ctx.close()
    for name, (rows, xr) in out.items():
        assert rows == out["plain"][0], name
        assert name == "plain" or xr == out[legs[1][0]][1], name
    n = sum(d["n_reads"] for d in data)

    def stats(v):
        return {"runs_ms": [round(t * 1e3, 2) for t in v], "median_ms": round(statistics.median(v) * 1e3, 2), "min_ms": round(min(v) * 1e3, 2),
                "max_ms": round(max(v) * 1e3, 2), "extra_over_plain": round(statistics.median(v) / statistics.median(times["plain"]), 2)}

    res = {"workload": f"junc --extra, {args.targets} targets of the BASELINE configs[1] shape scaled to {cfg.n_reads} reads on {cfg.contig_len} bases, "
                       f"{cfg.n_junctions} junctions each: {n} alignments, {len(out['plain'][0]) // ffi.ROW_DTYPE.itemsize} junctions, a fifth of the records multi-mapped",
           "arguments": " ".join(sys.argv[1:]), "queue": args.queue, "groups": groups,
           "note": "device-resident records, rows and extra rows on the host; one warmed context per leg, the legs' runs alternating; rows and extra "
                   "rows of the plans are the same bytes"}
    for name in times:
        res[name] = stats(times[name])
    if "targets" in times and "groups" in times:
        t, g = times["targets"], times["groups"]
        spread = max(t) - min(t)
        res["groups_faster_by_ms"] = round((statistics.median(t) - statistics.median(g)) * 1e3, 2)
        res["targets_spread_ms"] = round(spread * 1e3, 2)
        res["groups_beat_the_spread"] = bool(statistics.median(t) - statistics.median(g) > spread)
    print(json.dumps(res))


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--targets", type=int, default=0, help="K >= 2: the many-target workload (default: the two-target measurement)")
    ap.add_argument("--plan", default="targets,groups", help="targets | groups | targets,groups (many-target workload)")
    ap.add_argument("--reads-per-target", type=int, default=2_000_000)
    ap.add_argument("--contig-len", type=int, default=200_000_000)
    ap.add_argument("--junctions", type=int, default=20_000)
    ap.add_argument("--group-bases", type=int, default=0, help="bases of a group (0: pjb_plan_groups' own 2^30)")
    ap.add_argument("--queue", type=int, default=4, help="chains queued at once")
    ap.add_argument("--runs", type=int, default=5, help="timed runs per leg")
    args = ap.parse_args()
    if args.targets:
        if args.targets < 2 or not set(args.plan.split(",")) <= {"targets", "groups"}:
            ap.error("--targets K needs K >= 2 and --plan targets | groups | targets,groups")
        return many_targets(args)

    import numpy as np
    import torch

    from oracle import oracle as orc
    from portcullis_amd import ffi, synth

    base = synth.CONFIGS["C2"]
    # ---- parity on the small copy
    small = dataclasses.replace(base, n_reads=2_000_000, contig_len=20_000_000, n_junctions=10_000)
    data = make(small, synth, torch)
    lens = [small.contig_len] * 2
    rows, xr, _ = run_device(ffi, torch, data, lens, True, 0)
    soa, nh, rows_all = {}, {}, []
    tot = sum_len = max_len = 0
    t0 = time.perf_counter()
    for tid, d in enumerate(data):
        hb = synth.batch_to_numpy(d["batch"], 0, d["n_reads"])
        hb.name_hash = d["batch"]["name_hash"].cpu().numpy().view(np.uint64)
        soa[tid], nh[tid] = hb, hb.name_hash
        r, reg = orc.find_juncs(tid, lens[tid], d["genome"].cpu().numpy().tobytes().decode(), hb, "UNKNOWN")
        rows_all.append(r)
        tot += reg["spliced"] + reg["unspliced"]
        sum_len += reg["sum_len"]
        max_len = max(max_len, reg["max_len"])
    t_junc = time.perf_counter() - t0
    orows = orc.finalize(np.concatenate(rows_all), sum_len / tot)
    t0 = time.perf_counter()
    orows = orc.extra(lens, soa, nh, orows, max_len)
    t_extra_cpu = time.perf_counter() - t0
    assert len(rows) == len(orows) == len(xr)
    for col in ("coverage", "up_aln", "down_aln"):
        assert (xr[col] == orows[col]).all(), col
    worst = float(np.abs(xr["mm_score"] - orows["mm_score"]).max())
    assert worst <= 1e-6
    n_small = sum(d["n_reads"] for d in data)
    del data
    # ---- timing on 2 x 10 M reads
    data = make(base, synth, torch)
    lens = [base.contig_len] * 2
    n = sum(d["n_reads"] for d in data)
    rows0, _, t_plain = run_device(ffi, torch, data, lens, False, 3)
    rows1, xr1, t_extra = run_device(ffi, torch, data, lens, True, 3)
    assert rows0.tobytes() == rows1.tobytes()
    print(json.dumps({"workload": f"junc --extra, 2 targets of the BASELINE configs[1] shape: {n} alignments, {len(rows1)} junctions, "
                                  "a fifth of the records multi-mapped",
                      "plain_ms": round(t_plain * 1e3, 2), "extra_ms": round(t_extra * 1e3, 2),
                      "reads_per_sec_plain": n / t_plain, "reads_per_sec_extra": n / t_extra,
                      "note": "both targets queued (pjb_finish_contig_begin / _end), device-resident records, rows and extra rows on the host",
                      "extra_over_plain": round(t_extra / t_plain, 2),
                      "cpu_oracle": {"sample": f"{n_small} alignments (2 x 2 M reads), every coverage / up_aln / down_aln equal, max |mm_score diff| "
                                               f"{worst:.2g}", "junc_s": round(t_junc, 2), "extra_s": round(t_extra_cpu, 2),
                                     "reads_per_sec_extra": n_small / (t_junc + t_extra_cpu), "cores": 1}}))


if __name__ == "__main__":
    main()
