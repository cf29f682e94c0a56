"""Weighted matching fold (gs_matching_fold_device) on an MI355X against the sequential definition
(csrc/gs_matching_seq.hpp mt_fold_seq, built into tools/bin/matching_seq_bench) on one core, over
the same prefix.

The stream is RMAT-20 (gs_gen_rmat, scrambled ids), pre-staged in HBM with three value columns:
unit values, values 10..50 and uniform values below 2^40. It is folded from an empty matching in
2^16- and in 2^20-arrival folds. A pass is timed with a host clock around folds that each end in a
device synchronise; after one warm-up pass of every shape, `--reps` passes follow, the shapes
alternated pass by pass; medians and min-max over the passes are reported. Per fold, from
gs_testing_matching_stats: rounds, fixpoint passes, the arrivals the tail took over, the rounds
that fell back to plain reservations.

Before any number is printed, the accepted bytes and the event rows of the whole stream (one
2^20-arrival fold and 2^16-arrival folds) must equal the sequential fold's, for every value
column. The figure to report is GPU arrivals/s over sequential arrivals/s on that equal prefix.
`--iter-caps` and `--round-caps` list alternatives of two product constants (per-handle test
controls) to time against each other on the 10..50 column in one 2^20-arrival fold; a set round
cap also takes the tail threshold out of play, so the threshold itself is not compared.

There is no CPU fallback: without a GPU the script fails. Output: one JSON document.
Usage: python tools/matching_bench.py [--reps 5] [--edges 1048576] [--out profiles/matching_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCALE, SEED = 20, 0x5EED0020
FOLDS = (1 << 16, 1 << 20)
GEN = 1 << 20
COLUMNS = ("unit", "10..50", "uniform")


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def stage(gs, torch, edges):
    dev = torch.device("cuda", 0)
    src = torch.empty(edges, dtype=torch.int64, device=dev)
    dst = torch.empty(edges, dtype=torch.int64, device=dev)
    for b in range(0, edges, GEN):
        gs.gen_rmat(src[b:], dst[b:], b, min(GEN, edges - b), SCALE, SEED, True)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    vals = {"unit": torch.ones(edges, dtype=torch.int64, device=dev),
            "10..50": torch.randint(10, 51, (edges,), dtype=torch.int64, device=dev, generator=g),
            "uniform": torch.randint(0, 1 << 40, (edges,), dtype=torch.int64, device=dev, generator=g)}
    torch.cuda.synchronize()
    return src, dst, vals


def gpu_pass(m, src, dst, val, edges, fold, acc=None, events=None):
    """One pass from an empty matching; (seconds, per-fold stats). events: a list that receives
    every fold's rows with the arrival made global."""
    m.reset()
    m.sync()
    stats = []
    t0 = time.perf_counter()
    for b in range(0, edges, fold):
        n = min(fold, edges - b)
        m.fold_device(src[b:], dst[b:], val[b:], None if acc is None else acc[b:], n=n)
        m.sync()
        stats.append(m.stats())
        if events is not None:
            a, t, s, d, w = m.events()
            events.append((a.astype("int64") + b, t.astype("int64"), s, d, w))
    return time.perf_counter() - t0, stats


def shares(stats, edges):
    hist = {}
    for s in stats:
        hist[s["rounds"]] = hist.get(s["rounds"], 0) + 1
    return {"rounds_per_fold": {str(r): hist[r] for r in sorted(hist)},
            "fixpoint_passes": sum(s["iterations"] for s in stats),
            "tail_share_of_stream": sum(s["tail"] for s in stats) / edges,
            "fallback_rounds": sum(s["fallbacks"] for s in stats),
            "accepted_share": sum(s["accepted"] for s in stats) / edges}


def seq_baseline(np, src, dst, val, n, tmp):
    exe = os.path.join(ROOT, "tools", "bin", "matching_seq_bench")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "gelly-streaming_amd", "csrc"),
                           os.path.join(ROOT, "tools", "matching_seq_bench.cpp"), "-o", exe])
    arrivals, outf = os.path.join(tmp, "arrivals.bin"), os.path.join(tmp, "out.bin")
    with open(arrivals, "wb") as f:
        for x in (src, dst, val):
            f.write(x[:n].cpu().numpy().tobytes())
    secs, doc = [], None
    for _ in range(3):
        out = subprocess.run([exe, arrivals, str(n), outf], capture_output=True, text=True, check=True)
        doc = json.loads(out.stdout)
        secs.append(doc["seconds"])
    raw = np.fromfile(outf, dtype=np.uint8)
    doc["seconds"] = statistics.median(secs)
    return doc, raw[:n], raw[n:].view(np.int64).reshape(-1, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--edges", type=int, default=1 << 20)
    ap.add_argument("--iter-caps", default="1,2,4,6,12", help="fixpoint pass caps to compare ('' = none)")
    ap.add_argument("--round-caps", default="0,4,8,16,32,64", help="round caps to compare ('' = none)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    import gsamd as gs

    if not torch.cuda.is_available():
        sys.exit("matching_bench: no GPU (there is no CPU fallback)")
    src, dst, vals = stage(gs, torch, a.edges)
    doc = {"stream": "rmat%d" % SCALE, "edges": a.edges, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "constants": {"round_cap": gs.MATCHING_ROUND_CAP, "tail_threshold": gs.MATCHING_TAIL_THRESHOLD,
                         "iter_cap": gs.MATCHING_ITER_CAP},
           "columns": {}}
    lines = []
    with gs.Matching(vertex_hint=1 << SCALE) as m, tempfile.TemporaryDirectory() as tmp:
        # equality first: accepted bytes and event rows of every column, both fold sizes
        for c in COLUMNS:
            seq, seq_acc, seq_ev = seq_baseline(np, src, dst, vals[c], a.edges, tmp)
            for f in FOLDS:
                acc = torch.zeros(a.edges, dtype=torch.uint8, device=src.device)
                ev = []
                gpu_pass(m, src, dst, vals[c], a.edges, f, acc, ev)
                got = np.stack([np.concatenate([e[i] for e in ev]) for i in range(5)], axis=1)
                if not np.array_equal(acc.cpu().numpy(), seq_acc):
                    sys.exit("matching_bench: accepted bytes differ from the sequential fold's (%s, fold %d)" % (c, f))
                if not np.array_equal(got, seq_ev):
                    sys.exit("matching_bench: event rows differ from the sequential fold's (%s, fold %d)" % (c, f))
            doc["columns"][c] = {"sequential": {**seq, "edges_per_s": seq["edges"] / seq["seconds"]},
                                 "accepted_bytes_equal": True, "events_equal": True, "folds": {}}
        # timing
        passes = {(c, f): [] for c in COLUMNS for f in FOLDS}
        last = {}
        for rep in range(a.reps + 1):
            for c in COLUMNS:
                for f in FOLDS:
                    sec, stats = gpu_pass(m, src, dst, vals[c], a.edges, f)
                    if rep:  # (the first pass of every shape is the warm-up)
                        passes[(c, f)].append(sec)
                    last[(c, f)] = stats
        for c in COLUMNS:
            seq_rate = doc["columns"][c]["sequential"]["edges_per_s"]
            for f in FOLDS:
                rates = [a.edges / s for s in passes[(c, f)]]
                row = {"seconds": summary(passes[(c, f)]), "edges_per_s": summary(rates),
                       "gpu_over_sequential": statistics.median(rates) / seq_rate, **shares(last[(c, f)], a.edges)}
                doc["columns"][c]["folds"][str(f)] = row
                lines.append({"column": c, "fold": f, **row})
        # alternatives of the product constants, the 10..50 column in one fold
        val = vals["10..50"]
        sweeps = {"iter_cap": [int(x) for x in a.iter_caps.split(",") if x],
                  "round_cap": [int(x) for x in a.round_caps.split(",") if x]}
        for what, values in sweeps.items():
            times = {v: [] for v in values}
            for rep in range(a.reps + 1):
                for v in values:
                    m.tune(**{what: v})
                    sec = gpu_pass(m, src, dst, val, a.edges, a.edges)[0]
                    m.tune(**{what: -1})
                    if rep:
                        times[v].append(sec)
            doc[what + "_sweep"] = {str(v): summary(times[v]) for v in values}
            if values:
                lines.append({what + "_sweep": doc[what + "_sweep"]})
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
