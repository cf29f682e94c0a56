#!/usr/bin/env python3
"""One point of the hot index's grid on the flagship step (RMAT-26, 2^30 edges in 2^20-edge
batches, pipelining 3; reset + 1024 folds + label export per step): ms per step over --steps
steps after one warm-up step, and the digest of the final summary.

  GS_LIB_VARIANT=<name> python tools/hot_grid.py [--hot LOG2 FIRST EVERY] [--steps 4]

Without --hot the library's default rule runs (its size, refresh cadence, sample, sketch and
sample folds are the compile-time switches GS_HOT_LOG2, GS_HOT_REFRESH_EVERY, GS_HOT_SAMPLE_LOG2,
GS_HOT_SKETCH_ROWS, GS_HOT_SKETCH_LOG2, GS_HOT_SAMPLE_FOLDS of gs_capi.cpp: one `make variant`
library per setting, e.g. make variant V=f1 VFLAGS="-DGS_HOT_SAMPLE_FOLDS=1"). The caller
alternates the points (profiles/hot_buckets_grid.txt).

The build's counts can also be set per handle (gs_testing_hot_tune), so one library and one
process run a whole grid of them over one generated stream:

  python tools/hot_grid.py --sweep 17:1:4:1 17:2:5:4 18:2:5:4 ... [--rounds 2] [--steps 4]

Every point is LOG2:ROWS:SKETCH_LOG2:FOLDS. LOG2 0 is the default rule; another size is forced
with the default rule's first build and build cadence (2^26 edges, 2048 folds), which refreshes
every 128 folds and not every 16. The points run one after the other, --rounds times over
(profiles/hot_ways_grid.txt).

  GS_LIB_VARIANT=debug python tools/hot_grid.py --debug-counters 6 [--rows R --sketch-log2 S --sample-folds K]

prints, with the debug-counter library (make debug), the counter deltas of every 32 folds of the
first 32 x N folds of one step: the edges the index settled and those that fell back to the table
(profiles/hot_ways_debug_counters.txt)."""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--hot", type=int, nargs=3, default=None)
    p.add_argument("--steps", type=int, default=4)
    p.add_argument("--label", default="")
    p.add_argument("--rows", type=int, default=None)
    p.add_argument("--sketch-log2", type=int, default=None)
    p.add_argument("--sample-folds", type=int, default=None)
    p.add_argument("--sweep", nargs="+", default=None, metavar="LOG2:ROWS:SKETCH_LOG2:FOLDS")
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--debug-counters", type=int, default=0, metavar="N")
    a = p.parse_args()
    import torch
    gs = importlib.import_module("gelly-streaming_amd")
    scale, E, B = 26, 1 << 30, 1 << 20
    summ = gs.Summary("cc", capacity_hint=1 << (scale - 1))
    src = torch.empty(E, dtype=torch.int64, device="cuda")
    dst = torch.empty(E, dtype=torch.int64, device="cuda")
    gs.gen_rmat(src, dst, 0, E, scale, 0x5EED0026, True, stream=summ.stream)
    summ.sync()
    out_v = torch.empty((1 << scale) + 16, dtype=torch.int64, device="cuda")
    out_l = torch.empty_like(out_v)
    summ.set_pipelining(3)
    if a.hot:
        summ.set_hot_index(*a.hot)
    if (a.rows, a.sketch_log2, a.sample_folds) != (None, None, None):
        gs.testing_hot_tune(summ, a.rows, a.sketch_log2, a.sample_folds)

    def step():
        summ.reset()
        for o in range(0, E, B):
            summ.fold_device(src[o:], dst[o:], n=B)
        summ.export_labels_device(out_v, out_l)

    if a.debug_counters:
        summ.reset()
        last = summ.debug_counters()
        for k in range(a.debug_counters):
            for o in range(k * 32 * B, (k + 1) * 32 * B, B):
                summ.fold_device(src[o:], dst[o:], n=B)
            summ.sync()
            now = summ.debug_counters()
            st = summ.hot_index_stats()
            delta = {x: now[x] - last[x] for x in ("edges", "shortcut", "same_root", "hot_hits", "hot_fallbacks", "find_loads", "extra_probes", "key_cas")}
            print(a.label, 32 * (k + 1), "stats", {x: st[x] for x in ("builds", "entries", "log2_entries")}, "delta", delta, flush=True)
            last = now
        return
    if a.sweep:
        for rnd in range(a.rounds):
            for pt in a.sweep:
                log2, rows, sk, folds = (int(x) for x in pt.split(":"))
                summ.set_hot_index(log2, 1 << 26, 2048)
                gs.testing_hot_tune(summ, rows, sk, folds)
                step()
                summ.sync()
                ms = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    step()
                    summ.sync()
                    ms.append(round((time.perf_counter() - t0) * 1e3, 3))
                st = summ.hot_index_stats()
                print("RESULT", json.dumps({"lib": os.environ.get("GS_LIB_VARIANT", ""), "round": rnd, "point": pt,
                                            "ms_per_step": round(sum(ms) / len(ms), 3), "steps": ms,
                                            "digest": "%016x" % summ.digest(), "held": st["entries"],
                                            "builds": st["builds"], "refreshes": st["refreshes"]}), flush=True)
        return
    step()
    summ.sync()
    ms = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        step()
        summ.sync()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    st = summ.hot_index_stats()
    print("RESULT", json.dumps({"lib": os.environ.get("GS_LIB_VARIANT", ""), "label": a.label, "hot": a.hot,
                                "ms_per_step": round(sum(ms) / len(ms), 3), "steps": ms, "digest": "%016x" % summ.digest(),
                                "held": st["entries"], "builds": st["builds"], "refreshes": st["refreshes"]}))


if __name__ == "__main__":
    main()
