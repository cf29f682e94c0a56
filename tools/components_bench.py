"""Grouped component export (gs_export_components*) against the parent path, on an MI355X.

For each input -- config 2's final summary (RMAT-20, 2^24 edges) and the 2^24-edge prefix of
the RMAT-26 stream -- the summary is folded once, then three readers of the same information
are timed with a host clock around calls that end in their own synchronise, alternated in one
process after a warm-up:
  (a) components_device     the CSR into device arrays
  (b) components            the CSR into host arrays (gs_export_components)
  (c) parent                gs_export_labels to host + np.lexsort((v, label)), what
                            Summary.colouring() / labels() callers do today
and the outputs of (b) and (c) are compared for equality.

Kernel times come from a separate run under the profiler with no counters and no other
tracing (this script with --trace, which only runs (a)):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python tools/components_bench.py --trace --inputs rmat26p
  python tools/components_bench.py --kernel-stats DIR/.../run_kernel_stats.csv --rows N ...
--kernel-stats adds, per kernel, calls and average microseconds, and the per-pass rate of
k_sort_scatter and of a whole pass under the 32 B/row model (12 B read + 12 B written by
the scatter, 8 B read by the histogram), against the 6.29 TB/s streaming-copy ceiling.

There is no CPU fallback: without a GPU the script fails. Output: one JSON document.
Usage: python tools/components_bench.py [--reps 10] [--inputs rmat20,rmat26p] [--out FILE]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

INPUTS = {  # name: (scale, seed, edges) -- BASELINE configs 2 and 3's streams
    "rmat20": (20, 0x5EED0020, 1 << 24),
    "rmat26p": (26, 0x5EED0026, 1 << 24),
    "rmat26": (26, 0x5EED0026, 1 << 30),  # config 3's whole stream (32.8 M vertices); not in the default set
}
COPY_CEILING_GBS = 6290.0  # measured streaming copy (MI355X_MICROARCH.md)
PASS_BYTES_PER_ROW = 32
SCATTER_BYTES_PER_ROW = 24


def build_summary(gs, torch, name):
    scale, seed, edges = INPUTS[name]
    dev = torch.device("cuda", 0)
    batch = 1 << 20
    src = torch.empty(batch, dtype=torch.int64, device=dev)
    dst = torch.empty(batch, dtype=torch.int64, device=dev)
    s = gs.Summary("cc", device=0, capacity_hint=min(1 << scale, 1 << 25))
    for start in range(0, edges, batch):
        gs.gen_rmat(src, dst, start, batch, scale, seed, True)
        torch.cuda.synchronize()
        s.fold_device(src, dst)
        s.sync()
    return s


def parent_path(gs, s):
    """labels to host + the host sort by (label, vertex)."""
    import ctypes
    n = s.num_vertices()
    v = np.empty(n, np.int64)
    lab = np.empty(n, np.int64)
    got = ctypes.c_size_t()
    rc = gs.lib().gs_export_labels(s.handle, v.ctypes.data, lab.ctypes.data, n, ctypes.byref(got))
    if rc:
        raise gs.GSError(rc, gs.lib().gs_last_error().decode())
    t_copy = time.perf_counter()
    o = np.lexsort((v, lab))
    return v[o], lab[o], t_copy


def stats(xs):
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs), "reps": len(xs)}


def run_input(gs, torch, name, reps, trace):
    s = build_summary(gs, torch, name)
    nv = s.num_vertices()
    nc = s.num_components()
    dev = torch.device("cuda", 0)
    comp = torch.empty(nc, dtype=torch.int64, device=dev)
    offset = torch.empty(nc + 1, dtype=torch.int64, device=dev)
    member = torch.empty(nv, dtype=torch.int64, device=dev)
    sign = torch.empty(nv, dtype=torch.uint8, device=dev)
    out = {"input": name, "scale": INPUTS[name][0], "edges": INPUTS[name][2], "vertices": nv, "components": nc}
    if trace:
        for _ in range(3):
            s.components_device(comp, offset, member, sign)
        s.close()
        return out
    # warm-up: sizes every scratch buffer, pages the host arrays in
    s.components_device(comp, offset, member, sign)
    ok, hcomp, hoff, hmem, hsign = s.components()
    pv, pl, _ = parent_path(gs, s)
    out["host_equals_parent"] = bool(np.array_equal(hmem, pv) and
                                     np.array_equal(np.repeat(hcomp, np.diff(hoff.astype(np.int64))), pl))
    out["device_equals_host"] = bool(np.array_equal(member.cpu().numpy(), hmem) and
                                     np.array_equal(comp.cpu().numpy(), hcomp) and
                                     np.array_equal(offset.cpu().numpy().view(np.uint64), hoff))
    ta, tb, tc, tc_copy, tn = [], [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        s.components_device(comp, offset, member, sign)
        t1 = time.perf_counter()
        s.components()
        t2 = time.perf_counter()
        _, _, t_copy = parent_path(gs, s)
        t3 = time.perf_counter()
        s.num_components()
        t4 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
        tc.append(t3 - t2)
        tc_copy.append(t_copy - t2)
        tn.append(t4 - t3)
    out["components_device"] = stats(ta)
    out["components_host"] = stats(tb)
    out["parent_export_labels_lexsort"] = stats(tc)
    out["parent_export_labels_only"] = stats(tc_copy)
    out["num_components"] = stats(tn)
    out["host_speedup_over_parent"] = out["parent_export_labels_lexsort"]["median_ms"] / out["components_host"]["median_ms"]
    s.close()
    return out


def kernel_stats(path, rows):
    """Per-kernel calls / average from a rocprofv3 --stats kernel_stats.csv; rates for `rows` rows."""
    ks = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            r = {k.lower(): v for k, v in r.items()}
            name = r["name"].replace("void ", "").replace("(anonymous namespace)::", "")
            short = name.split("(")[0].split("::")[-1].strip()
            if not (short.startswith("k_sort") or short.startswith("k_comp") or short.startswith("k_export")):
                continue
            ks[short] = {"calls": int(r["calls"]), "avg_us": float(r["averagens"]) / 1e3,
                         "total_ms": float(r["totaldurationns"]) / 1e6}
    out = {"rows": rows, "kernels": ks, "copy_ceiling_gbs": COPY_CEILING_GBS}
    if "k_sort_scatter" in ks and rows:
        sc = ks["k_sort_scatter"]["avg_us"]
        out["scatter_gbs_at_24B_per_row"] = SCATTER_BYTES_PER_ROW * rows / (sc * 1e-6) / 1e9
        out["scatter_gbs_at_32B_per_row_model"] = PASS_BYTES_PER_ROW * rows / (sc * 1e-6) / 1e9
        per_pass = sc + ks.get("k_sort_hist", {}).get("avg_us", 0.0) + ks.get("k_sort_scan", {}).get("avg_us", 0.0)
        out["pass_us"] = per_pass
        out["pass_gbs_at_32B_per_row"] = PASS_BYTES_PER_ROW * rows / (per_pass * 1e-6) / 1e9
        out["pass_fraction_of_copy_ceiling"] = out["pass_gbs_at_32B_per_row"] / COPY_CEILING_GBS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inputs", default="rmat20,rmat26p")
    ap.add_argument("--trace", action="store_true", help="only run the device export (for a profiler run)")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a --trace run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--rows", type=int, default=0, help="rows of the traced input (its 'vertices')")
    ap.add_argument("--out")
    a = ap.parse_args()
    doc = {"tool": "components_bench"}
    if a.kernel_stats:
        prev = None
        if a.out and os.path.exists(a.out):  # merge into an earlier timing document
            with open(a.out) as f:
                prev = json.load(f)
        rows = a.rows or (prev["results"][-1]["vertices"] if prev else 0)  # the traced input is the last one timed
        doc["kernel_trace"] = kernel_stats(a.kernel_stats, rows)
        if prev:
            prev["kernel_trace"] = doc["kernel_trace"]
            doc = prev
    else:
        import torch
        import gsamd as gs
        gs.lib()
        if not torch.cuda.is_available():
            raise SystemExit("components_bench needs an MI355X: no GPU is visible")
        doc["device"] = torch.cuda.get_device_name(0)
        doc["reps"] = a.reps
        doc["sort_tile"] = gs.SORT_TILE
        doc["results"] = [run_input(gs, torch, n, a.reps, a.trace) for n in a.inputs.split(",")]
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
