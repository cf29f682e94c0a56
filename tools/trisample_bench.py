"""Sampling triangle estimate (gs_trisample_fold_device) on an MI355X against the sequential
definition (csrc/gs_trisample_seq.hpp ts_fold_seq, built into tools/bin/trisample_seq_bench) on one
core.

Two streams, pre-staged in HBM: the reference's default stream -- (k, (k + 2) % 1000) and
(k, (k + 4) % 1000) for k = 0 .. 999, 1000 vertices -- and the first 2^16 edges of RMAT-16
(gs_gen_rmat, plain ids, 65536 vertices). Each is folded from a reset handle in one fold, for
S in {1000, 10000, 100000} instances. A pass is timed with a host clock around a fold that ends
in a device synchronise; after one warm-up pass of every shape, `--reps` passes follow, the shapes
alternated pass by pass; medians and min-max over the passes are reported, as arrivals/s and as
(instance x arrival)/s. In one further pass per shape the handle brackets its phases with events
(gs_testing_trisample_tune, profile): the coin pass and the search pass per (instance x arrival).

Before any number is printed, the rows of every shape must equal the sequential fold's over the
prefix the sequential fold runs (`--seq-work` instance x arrivals at most: it is slow), and the
GPU's rows must be the same when the stream is cut into four folds. The figure to report is GPU
(instance x arrival)/s over sequential (instance x arrival)/s.

There is no CPU fallback: without a GPU the script fails. Output: one JSON document.
Usage: python tools/trisample_bench.py [--reps 5] [--out profiles/trisample_bench.json]
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

SAMPLES = (1000, 10000, 100000)
SCALE, SEED = 16, 0x5EED0016


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def stage(gs, torch):
    dev = torch.device("cuda", 0)
    k = torch.arange(1000, dtype=torch.int64, device=dev)
    d_src = torch.stack([k, k], dim=1).reshape(-1).contiguous()
    d_dst = torch.stack([(k + 2) % 1000, (k + 4) % 1000], dim=1).reshape(-1).contiguous()
    n = 1 << SCALE
    r_src = torch.empty(n, dtype=torch.int64, device=dev)
    r_dst = torch.empty(n, dtype=torch.int64, device=dev)
    gs.gen_rmat(r_src, r_dst, 0, n, SCALE, SEED, False)
    torch.cuda.synchronize()
    return {"default": (d_src, d_dst, 1000), "rmat%d" % SCALE: (r_src, r_dst, 1 << SCALE)}


def rows_of(np, ts):
    e, est, b = ts.rows()
    return np.stack([e, est, b], axis=1)


def gpu_pass(ts, src, dst, n, cuts=1, np=None):
    """One pass from a reset handle in `cuts` folds; (seconds, rows when np is given)."""
    ts.reset()
    ts.sync()
    rows = []
    step = (n + cuts - 1) // cuts
    t0 = time.perf_counter()
    for b in range(0, n, step):
        ts.fold_device(src[b:], dst[b:], n=min(step, n - b))
        if np is not None:
            rows.append(rows_of(np, ts))
    sec = time.perf_counter() - t0
    return sec, (np.concatenate(rows) if np is not None else None)


def seq_baseline(np, src, dst, n, samples, vertices, tmp):
    exe = os.path.join(ROOT, "tools", "bin", "trisample_seq_bench")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "gelly-streaming_amd", "csrc"),
                           os.path.join(ROOT, "tools", "trisample_seq_bench.cpp"), "-o", exe])
    arrivals, outf = os.path.join(tmp, "arrivals.bin"), os.path.join(tmp, "rows.bin")
    with open(arrivals, "wb") as f:
        for x in (src, dst):
            f.write(x[:n].cpu().numpy().tobytes())
    out = subprocess.run([exe, arrivals, str(n), str(samples), str(vertices), outf], capture_output=True, text=True,
                         check=True)
    return json.loads(out.stdout), np.fromfile(outf, dtype=np.int32).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seq-work", type=int, default=1 << 29, help="instance x arrivals of a sequential fold, at most")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    import gsamd as gs

    if not torch.cuda.is_available():
        sys.exit("trisample_bench: no GPU (there is no CPU fallback)")
    streams = stage(gs, torch)
    doc = {"reps": a.reps, "device": torch.cuda.get_device_name(0),
           "constants": {"chunk": gs.TRISAMPLE_CHUNK, "tile": gs.TRISAMPLE_TILE}, "shapes": []}
    shapes = [(name, S) for name in streams for S in SAMPLES]
    handles = {}
    with tempfile.TemporaryDirectory() as tmp:
        try:
            # equality first
            for name, S in shapes:
                src, dst, V = streams[name]
                n = src.numel()
                ts = handles[(name, S)] = gs.TriangleSampler(S, V)
                _, whole = gpu_pass(ts, src, dst, n, 1, np)
                _, cut = gpu_pass(ts, src, dst, n, 4, np)
                if not np.array_equal(whole, cut):
                    sys.exit("trisample_bench: the rows depend on the cut (%s, S = %d)" % (name, S))
                prefix = max(1, min(n, a.seq_work // S))
                seq, seq_rows = seq_baseline(np, src, dst, prefix, S, V, tmp)
                if not np.array_equal(whole[whole[:, 0] <= prefix], seq_rows):
                    sys.exit("trisample_bench: rows differ from the sequential fold's (%s, S = %d)" % (name, S))
                doc["shapes"].append({"stream": name, "samples": S, "arrivals": n, "vertices": V, "rows": len(whole),
                                      "rows_equal_on_prefix": prefix,
                                      "sequential": {**seq, "pairs_per_s": prefix * S / seq["seconds"]}})
            # timing, the shapes alternated
            passes = {k: [] for k in shapes}
            for rep in range(a.reps + 1):
                for name, S in shapes:
                    src, dst, _ = streams[name]
                    sec, _ = gpu_pass(handles[(name, S)], src, dst, src.numel())
                    if rep:  # (the first pass of every shape is the warm-up)
                        passes[(name, S)].append(sec)
            for row in doc["shapes"]:
                name, S, n = row["stream"], row["samples"], row["arrivals"]
                ts = handles[(name, S)]
                secs = passes[(name, S)]
                row["seconds"] = summary(secs)
                row["arrivals_per_s"] = summary([n / s for s in secs])
                row["pairs_per_s"] = summary([n * S / s for s in secs])
                row["gpu_over_sequential"] = row["pairs_per_s"]["median"] / row["sequential"]["pairs_per_s"]
                # the phases, in a pass of their own
                ts.tune(profile=True)
                gpu_pass(ts, streams[name][0], streams[name][1], n)
                stats, us = ts.phases()
                ts.tune(profile=False)
                row["phase_us"] = us
                row["coins"] = stats["coins"]
                row["coin_pairs_per_s"] = n * S / (us["coin"] * 1e-6) if us["coin"] else None
                row["search_pairs_per_s"] = n * S / (us["search"] * 1e-6) if us["search"] else None
                print(json.dumps(row), flush=True)
        finally:
            for ts in handles.values():
                ts.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
