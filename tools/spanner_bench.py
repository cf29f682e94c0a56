"""Spanner fold (gs_spanner_fold_device) on an MI355X against the sequential restatement of
Spanner.UpdateLocal (csrc/gs_spanner_seq.hpp, built into tools/bin/spanner_seq_bench) on one core.

The stream is RMAT-20 (gs_gen_rmat, scrambled ids), pre-staged in HBM, folded with k = 3 in
2^16- and in 2^20-edge folds from an empty spanner. A pass is timed with a host clock around
folds that each end in a device synchronise (the fold waits for its own counts); after one
warm-up pass, `--reps` passes follow, the fold sizes alternated pass by pass; medians and min-max
over the passes are reported. Per fold, from gs_testing_spanner_stats: the arrivals the filter
pass dropped, the pending edges, the rounds, the edges left to the serial tail, the searches
that took the heavy path and the longest row expanded -- from which the round histogram and
the filter, tail and heavy shares of the whole stream follow.

The baseline folds the first `--seq-edges` edges of the same stream; the GPU's accepted bytes
for that prefix must equal the baseline's, and the GPU is timed on that prefix too (a rate
falls as the spanner grows, so rates are compared on equal prefixes only). `--arenas` lists pool
sizes of the heavy path (the private test knob spanner_arenas) to time against each other on the
2^16-edge folds.

There is no CPU fallback: without a GPU the script fails. Output: one JSON document.
Usage: python tools/spanner_bench.py [--reps 5] [--edges 2097152] [--seq-edges 262144] [--out profiles/spanner_bench.json]
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

SCALE, SEED, K = 20, 0x5EED0020, 3
FOLDS = (1 << 16, 1 << 20)
GEN = 1 << 20


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def stage(gs, torch, edges):
    dev = torch.device("cuda", 0)
    src = torch.empty(edges, dtype=torch.int64, device=dev)
    dst = torch.empty(edges, dtype=torch.int64, device=dev)
    for b in range(0, edges, GEN):
        gs.gen_rmat(src[b:], dst[b:], b, min(GEN, edges - b), SCALE, SEED, True)
    torch.cuda.synchronize()
    return src, dst


def gpu_pass(gs, torch, sp, src, dst, edges, fold, acc=None):
    """One pass from an empty spanner; (seconds, per-fold stats, per-fold seconds)."""
    sp.reset()
    sp.sync()
    stats, secs = [], []
    t0 = time.perf_counter()
    for b in range(0, edges, fold):
        n = min(fold, edges - b)
        t = time.perf_counter()
        sp.fold_device(src[b:], dst[b:], None if acc is None else acc[b:], n=n)
        sp.sync()
        secs.append(time.perf_counter() - t)
        stats.append(sp.stats())
    return time.perf_counter() - t0, stats, secs


def shares(stats, edges):
    pend = sum(s["pending"] for s in stats)
    hist = {}
    for s in stats:
        hist[s["rounds"]] = hist.get(s["rounds"], 0) + 1
    return {"filter_drop_share": sum(s["filter_drops"] for s in stats) / edges,
            "pending": pend,
            "tail_share_of_pending": sum(s["tail"] for s in stats) / max(pend, 1),
            "tail_share_of_stream": sum(s["tail"] for s in stats) / edges,
            "heavy_searches": sum(s["heavy"] for s in stats),
            "heavy_share_of_stream": sum(s["heavy"] for s in stats) / edges,
            "longest_row": max(s["longest_row"] for s in stats),
            "round_histogram": {str(r): hist[r] for r in sorted(hist)}}


def seq_baseline(np, src, dst, n, tmp):
    exe = os.path.join(ROOT, "tools", "bin", "spanner_seq_bench")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "gelly-streaming_amd", "csrc"),
                           os.path.join(ROOT, "tools", "spanner_seq_bench.cpp"), "-o", exe])
    edges, accf = os.path.join(tmp, "edges.bin"), os.path.join(tmp, "acc.bin")
    with open(edges, "wb") as f:
        f.write(src[:n].cpu().numpy().tobytes())
        f.write(dst[:n].cpu().numpy().tobytes())
    out = subprocess.run([exe, edges, str(n), str(K), accf], capture_output=True, text=True, check=True)
    return json.loads(out.stdout), np.fromfile(accf, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--edges", type=int, default=1 << 21)
    ap.add_argument("--seq-edges", type=int, default=1 << 18)
    ap.add_argument("--arenas", default="8,32,64", help="pool sizes of the heavy path to compare ('' = none)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    import gsamd as gs

    if not torch.cuda.is_available():
        sys.exit("spanner_bench: no GPU (there is no CPU fallback)")
    src, dst = stage(gs, torch, a.edges)
    doc = {"stream": "rmat%d" % SCALE, "k": K, "edges": a.edges, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "knobs": {"round_cap": gs.SPANNER_ROUND_CAP, "lds_set": gs.SPANNER_LDS_SET, "arenas": gs.SPANNER_ARENAS},
           "folds": {}}
    with gs.Spanner(k=K, edge_hint=a.edges) as sp:
        seq_n = min(a.seq_edges, a.edges)
        passes = {f: [] for f in FOLDS}
        prefix = {f: [] for f in FOLDS}
        last = {}
        for f in FOLDS:  # warm-up: every shape once
            gpu_pass(gs, torch, sp, src, dst, a.edges, f)
        for _ in range(a.reps):
            for f in FOLDS:
                sec, stats, secs = gpu_pass(gs, torch, sp, src, dst, a.edges, f)
                passes[f].append(sec)
                last[f] = (stats, secs)
                prefix[f].append(gpu_pass(gs, torch, sp, src, dst, seq_n, min(f, seq_n))[0])
        for f in FOLDS:
            stats, secs = last[f]
            doc["folds"][str(f)] = {
                "seconds": summary(passes[f]),
                "edges_per_s": summary([a.edges / s for s in passes[f]]),
                "prefix_edges": seq_n,
                "prefix_edges_per_s": summary([seq_n / s for s in prefix[f]]),
                "fold_ms_first_last": [1e3 * secs[0], 1e3 * secs[-1]],
                **shares(stats, a.edges)}
            print(json.dumps({"fold": f, **doc["folds"][str(f)]}), flush=True)
        # the pool of the heavy path: the same stream in 2^16-edge folds, the sizes alternated
        sweep = [int(x) for x in a.arenas.split(",") if x]
        times = {n: [] for n in sweep}
        for rep in range(a.reps + 1):
            for n in sweep:
                with gs.testing(spanner_arenas=n):
                    sec = gpu_pass(gs, torch, sp, src, dst, a.edges, FOLDS[0])[0]
                if rep:  # (the first pass of each size allocates its pool)
                    times[n].append(sec)
        doc["arenas_sweep"] = {str(n): summary(times[n]) for n in sweep}
        if sweep:
            print(json.dumps({"arenas_sweep": doc["arenas_sweep"]}), flush=True)
        sp.reset()
        sp.fold_device(src, dst, n=a.edges)
        doc["edges_kept"], doc["vertices"] = sp.count()
        # the accepted bytes of the prefix, for the comparison with the baseline
        acc = torch.zeros(seq_n, dtype=torch.uint8, device=src.device)
        gpu_pass(gs, torch, sp, src, dst, seq_n, min(FOLDS[0], seq_n), acc)
        gpu_acc = acc.cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        seq, seq_acc = seq_baseline(np, src, dst, seq_n, tmp)
    doc["sequential"] = {**seq, "edges_per_s": seq["edges"] / seq["seconds"],
                         "accepted_bytes_equal": bool(np.array_equal(gpu_acc, seq_acc))}
    print(json.dumps({"sequential": doc["sequential"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    if not doc["sequential"]["accepted_bytes_equal"]:
        sys.exit("spanner_bench: the GPU's accepted bytes differ from the sequential fold's")


if __name__ == "__main__":
    main()
