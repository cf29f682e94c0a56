#!/usr/bin/env python3
"""CPU model of what the hot index covers on the flagship stream: table probes per edge for a
bucket layout and a way of counting (no GPU needed).

RMAT-26 micro-batches of 2^20 edges from oracle.rmat_edges, seed 0x5EED0026. Folds 64-67 are the
sample (the build follows the last of the counted folds and takes its candidates from it);
batches 500 and 900 are the test. Each bucket keeps its highest ranks {count, tag}. Every
candidate is assumed to be in the table and under the build's ancestor G (the grids show
129-131 K of 131,072 places held). Table probes per edge = one-hit edges + 2 x no-hit edges: two
hits need no table access, one hit needs the missed side's probe.

Read the table for differences between rows, not for absolute values: the fold's measured
requests per edge add the edge stream (0.125), finds, fallbacks and second-line probes.

  python tools/hot_cover.py [--quick]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED, SCALE, B = 0x5EED0026, 26, 1 << 20
MUL = np.uint64(0xD6E8FEB86659FD93)            # hot_pos (gs_device.hpp)
TAG = np.uint64(0x9E3779B97F4A7C15)            # hot_rank's tag (gs_hot_k.hip)
ROW_MUL = (np.uint64(0xC2B2AE3D27D4EB4F), np.uint64(0xA24BAED4963EE407))   # sketch_pos


def batch(i):
    import oracle
    s, d = oracle.rmat_edges(SEED, SCALE, i * B, B, True)
    return np.asarray(s).astype(np.uint64), np.asarray(d).astype(np.uint64)


def counts_of(ids, folds, rows, sketch_bits):
    """The count the build would rank each of `ids` by: exact (rows == 0), or the smallest of the
    rows' counters of a sketch of 2^sketch_bits counters per row."""
    ends = np.concatenate([np.concatenate(f) for f in folds])
    if rows == 0:
        u, c = np.unique(ends, return_counts=True)
        return c[np.searchsorted(u, ids)]
    est = None
    for r in range(rows):
        sh = np.uint64(64 - sketch_bits)
        tab = np.bincount(((ends * ROW_MUL[r]) >> sh).astype(np.int64), minlength=1 << sketch_bits)
        e = tab[((ids * ROW_MUL[r]) >> sh).astype(np.int64)]
        est = e if est is None else np.minimum(est, e)
    return est


def held_keys(sample, q, places, nfolds, rows, sketch_bits, all_candidates=False):
    folds = sample[len(sample) - nfolds:]
    cand = np.unique(np.concatenate([np.concatenate(f) for f in (folds if all_candidates else folds[-1:])]))
    cnt = counts_of(cand, folds, rows, sketch_bits).astype(np.uint64)
    rank = (cnt << np.uint64(32)) | ((cand * TAG) >> np.uint64(32))
    bucket = (cand * MUL) >> np.uint64(64 - q)
    order = np.lexsort((np.iinfo(np.uint64).max - rank, bucket))
    b = bucket[order]
    first = np.r_[0, np.flatnonzero(b[1:] != b[:-1]) + 1]
    place = np.arange(len(b)) - np.repeat(first, np.diff(np.r_[first, len(b)]))
    return np.sort(cand[order][place < places])


def probes_per_edge(held, tests):
    e = p = 0
    for s, d in tests:
        hs, hd = np.isin(s, held), np.isin(d, held)
        p += int((~hs).sum() + (~hd).sum())
        e += len(s)
    return p / e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one test batch only")
    a = ap.parse_args()
    sample = [batch(i) for i in range(64, 68)]
    tests = [batch(i) for i in ((500,) if a.quick else (500, 900))]
    rows = [  # name, log2 buckets, places, folds, sketch rows (0: exact), sketch bits, candidates from every fold
        ("2^16 x 2 | 1 fold, one row 2^21 (the parent)", 16, 2, 1, 1, 21, False),
        ("2^16 x 2 | 1 fold, one row 2^22", 16, 2, 1, 1, 22, False),
        ("2^16 x 2 | 1 fold, one row 2^23", 16, 2, 1, 1, 23, False),
        ("2^16 x 2 | 1 fold, two rows x 2^22", 16, 2, 1, 2, 22, False),
        ("2^16 x 2 | 1 fold, exact counts", 16, 2, 1, 0, 0, False),
        ("2^16 x 2 | 2 folds, one row 2^23", 16, 2, 2, 1, 23, False),
        ("2^16 x 2 | 2 folds, two rows x 2^22", 16, 2, 2, 2, 22, False),
        ("2^16 x 2 | 4 folds, one row 2^23", 16, 2, 4, 1, 23, False),
        ("2^16 x 2 | 4 folds, exact counts", 16, 2, 4, 0, 0, False),
        ("2^15 x 5 | 1 fold, one row 2^21", 15, 5, 1, 1, 21, False),
        ("2^15 x 5 | 1 fold, two rows x 2^22", 15, 5, 1, 2, 22, False),
        ("2^15 x 5 | 4 folds, two rows x 2^22", 15, 5, 4, 2, 22, False),
        ("2^15 x 5 | 4 folds, exact counts", 15, 5, 4, 0, 0, False),
        ("2^15 x 5 | 4 folds, exact counts, candidates from every fold", 15, 5, 4, 0, 0, True),
        ("2^15 x 4 | 1 fold, exact counts (no quotienting)", 15, 4, 1, 0, 0, False),
    ]
    print("| index in 1 MiB | counts from | keys held | table probes/edge |")
    print("|---|---|---|---|")
    for name, q, places, nfolds, r, bits, allc in rows:
        held = held_keys(sample, q, places, nfolds, r, bits, allc)
        layout, counts = name.split(" | ")
        print("| %s | %s | %d | %.3f |" % (layout, counts, len(held), probes_per_edge(held, tests)), flush=True)


if __name__ == "__main__":
    main()
