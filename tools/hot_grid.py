#!/usr/bin/env python3
"""One point of the hot index's grid on the flagship step (RMAT-26, 2^30 edges in 2^20-edge
batches, pipelining 3; reset + 1024 folds + label export per step): ms per step over --steps
steps after one warm-up step, and the digest of the final summary.

  GS_LIB_VARIANT=<name> python tools/hot_grid.py [--hot LOG2 FIRST EVERY] [--steps 4]

Without --hot the library's default rule runs (its size, refresh cadence and sample are the
compile-time switches GS_HOT_LOG2, GS_HOT_REFRESH_EVERY, GS_HOT_SAMPLE_LOG2 of gs_capi.cpp:
one `make variant` library per setting). The caller alternates the points
(profiles/hot_buckets_grid.txt)."""
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

    def step():
        summ.reset()
        for o in range(0, E, B):
            summ.fold_device(src[o:], dst[o:], n=B)
        summ.export_labels_device(out_v, out_l)

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
