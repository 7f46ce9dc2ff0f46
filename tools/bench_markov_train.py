#!/usr/bin/env python3
"""Measurement of self-training's Markov stage: one JSON document to profiles/markov_train.json (and stdout).

Input: the 10 M-read C2 input of tests/e2e_bench.py (made here: synth -> soa2bam -> junc; 49 366 junctions), rule set balanced.
`filt --self_train` is run RUNS times with this tree's program and, alternating with it, with another build's (--other: the parent
commit's portcullis_amd, which trains on the host); of each run the wall time from "Feature learning from training set ..." to " done."
on the program's output (this tree: contig upload, the training on the device and the tables' way back) and the wall time of the whole
command.  Then, through the binding, pjb_markov_train on the run's own initial sets with kernel timing on: the device time of km_count
alone and of the other km_* kernels, and the transitions counted (the bases walked, less five a window that trains).

    timeout 900 python tools/bench_markov_train.py [--other /path/to/parent/portcullis_amd/host/portcullis_amd]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RUNS = 5
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
BEGIN, END = b"Feature learning from training set ...", b" done."


def timed_filt(exe, prep, tab, out):
    """(seconds between the stage's two messages, seconds of the whole command)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    t0 = time.perf_counter()
    p = subprocess.Popen([exe, "filt", "--self_train", DATA, "--training_rule", "balanced", "-o", out, prep, tab], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         env=env)
    seen, t_begin, t_end = b"", None, None
    while True:
        chunk = os.read(p.stdout.fileno(), 65536)
        now = time.perf_counter()
        if not chunk:
            break
        seen += chunk
        at = seen.find(BEGIN)
        if t_begin is None and at >= 0:
            t_begin = now
        if t_begin is not None and t_end is None and seen.find(END, at + len(BEGIN)) >= 0:
            t_end = now
    err = p.stderr.read()
    if p.wait() != 0 or t_end is None:
        raise SystemExit(f"{exe} filt failed ({p.returncode}):\n" + seen.decode(errors="replace")[-1500:] + err.decode(errors="replace")[-1500:])
    return t_end - t_begin, time.perf_counter() - t0


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), runs=[round(x, 4) for x in v])


def device_side(prep, prefix):
    """pjb_markov_train on the run's initial sets, kernel timing on"""
    import numpy as np
    from portcullis_amd import ffi
    from test_host_filt import read_tab
    from util_bam import PREP_FA, read_fasta

    contigs = read_fasta(os.path.join(prep, PREP_FA))
    strand = {"+": 0, "-": 1, "?": 2}
    sets = []
    for which in ("pos", "neg"):
        h, rows = read_tab(open(f"{prefix}.selftrain.initialset.{which}.junctions.tab").read(), is_text=True)
        r = np.zeros(len(rows), dtype=ffi.ROW_DTYPE)
        r["refid"] = [int(x[h.index("refid")]) for x in rows]
        r["start"] = [int(x[h.index("start")]) for x in rows]
        r["end"] = [int(x[h.index("end")]) for x in rows]
        r["cons_strand"] = [strand[x[h.index("consensus-strand")]] for x in rows]
        sets.append(r)
    rows = np.concatenate(sets)
    pos, neg = np.arange(len(sets[0])), len(sets[0]) + np.arange(len(sets[1]))
    with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_KERNEL_TIMING) as ctx:
        ctx.set_refs([len(s) for _, s in contigs])
        for t, (_, s) in enumerate(contigs):
            ctx.upload_contig(t, bytes(s))
        ctx.markov_train(rows, pos, pos, neg)  # (warm)
        count_ms, other_ms, wall = [], [], []
        for _ in range(RUNS):
            ctx.reset_kernel_timing()
            t0 = time.perf_counter()
            m = ctx.markov_train(rows, pos, pos, neg)
            wall.append(time.perf_counter() - t0)
            kt = ctx.kernel_timing()
            count_ms.append(kt["km_count"][1])
            other_ms.append(sum(ms for name, (_, ms) in kt.items() if name.startswith("km_") and name != "km_count"))
        launches = ctx.kernel_timing()["km_count"][0]
    return dict(positive=len(pos), negative=len(neg), transitions=m["transitions"], km_count_launches=launches, km_count_device_ms=spread(count_ms),
                other_km_kernels_device_ms=spread(other_ms), pjb_markov_train_wall_s=spread(wall),
                sizes={k: v for k, v in m.items() if k.endswith("_size")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="another build's portcullis_amd program (the parent commit's) to alternate with")
    ap.add_argument("--workdir", default="/tmp/pjb_markov_bench")
    args = ap.parse_args()
    wd = args.workdir
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "e2e_bench.py"), "--config", "C2", "--threads", "16", "--no-oracle", "--repeat", "1", "--keep",
                        "--workdir", wd], capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(p.stdout[-2000:] + p.stderr[-2000:])
    e2e = json.loads(p.stdout.strip().split("\n")[-1])
    prep, tab = os.path.join(wd, "prep"), os.path.join(wd, "out0", "pc.junctions.tab")
    exes = [("this", EXE)] + ([("other", args.other)] if args.other else [])
    stage = {k: [] for k, _ in exes}
    whole = {k: [] for k, _ in exes}
    for k, exe in exes:  # one run each that is not counted: page cache, the runtime's first start
        timed_filt(exe, prep, tab, os.path.join(wd, "filt_warm_" + k, "pc"))
    for run in range(RUNS):
        for k, exe in exes[::-1] if run % 2 else exes:
            s, w = timed_filt(exe, prep, tab, os.path.join(wd, f"filt_{k}_{run}", "pc"))
            stage[k].append(s)
            whole[k].append(w)
    res = dict(input=dict(config=e2e["config"], reads=e2e["reads"], junctions=e2e["junctions"], bam_mb=e2e["bam_mb"], ruleset="balanced"),
               stage_wall_s={k: spread(v) for k, v in stage.items()}, filt_wall_s={k: spread(v) for k, v in whole.items()},
               device=device_side(prep, os.path.join(wd, "filt_this_0", "pc")))
    if args.other:
        same = all(open(os.path.join(wd, f"filt_this_0", "pc" + n), "rb").read() == open(os.path.join(wd, f"filt_other_0", "pc" + n), "rb").read()
                   for n in (".pass.junctions.tab", ".selftrain.forest"))
        res["pass_table_and_forest_equal_the_other_builds"] = same
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "markov_train.json"), "w").write(text + "\n")
    import shutil
    shutil.rmtree(wd, ignore_errors=True)


if __name__ == "__main__":
    main()
