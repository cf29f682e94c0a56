"""The figures of DESIGN.md section 6k (-> profiles/text_bench.json): the kernel time of the LONG and
EVENT parses beside the two-field parse of the same bytes (gs_parse_set_profiling events; RMAT-20
ids, 2^21 lines), the whole gs_parse_records_device call at 0 %, 1 % and 33 % comment lines (wall
clock around the synchronised call, 2^20 lines), and TextReader.fold_into of a 2^20-line text into
DegreeStream and Matching beside fold of the host arrays (wall clock, three runs each).
Run from the repository root on the GPU: python tools/text_bench.py [out.json]"""
import json, sys, time
import numpy as np
sys.path.insert(0, ".")
import torch
import gsamd as gs
import oracle

out = {}
N = 1 << 21
s, d = oracle.rmat_edges(0x5EED0014, 20, 0, N, True)
rng = np.random.default_rng(5)
ts = np.cumsum(rng.integers(0, 20, N))
ev = rng.integers(0, 2, N)
sl, dl, tl, el = s.tolist(), d.tolist(), ts.tolist(), ev.tolist()
T_long = b"".join(b"%d %d %d\n" % r for r in zip(sl, dl, tl))
T_event = b"".join(b"%d %d %s\n" % (a, b, b"+" if e else b"-") for a, b, e in zip(sl, dl, el))

def dev(text):
    return torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()

src = torch.zeros(N + N // 2 + 8, dtype=torch.int64, device="cuda")
dst = torch.zeros_like(src)
val = torch.zeros_like(src)
dele = torch.zeros(src.numel(), dtype=torch.uint8, device="cuda")

def kernel_us(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    gs.parse_set_profiling(True)
    for _ in range(reps):
        fn()
    us, n = gs.parse_profile()
    gs.parse_set_profiling(False)
    assert n == reps
    return us / n

def wall_us(fn, reps=15, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - a) * 1e6)
    return float(np.median(t)), float(min(t)), float(max(t))

for name, text, third, col in (("long", T_long, "long", val), ("event", T_event, "event", dele)):
    t = dev(text)
    two = kernel_us(lambda: gs.parse_edges_device(t, src, dst))
    three = kernel_us(lambda: gs.parse_records_device(t, src, dst, col, 0, third))
    out["kernel_" + name] = {"lines": N, "bytes": len(text), "two_field_us": two, "three_field_us": three,
                             "two_Glines_s": N / two / 1e3, "three_Glines_s": N / three / 1e3,
                             "two_GB_s": len(text) / two / 1e3, "three_GB_s": len(text) / three / 1e3}
    print(name, json.dumps(out["kernel_" + name]), flush=True)

# comment compaction: the whole call (parse, counts to the host, compaction, copy back), wall clock
lines = T_long.split(b"\n")[:-1][: 1 << 20]
for pct, every in ((0, 0), (1, 100), (33, 3)):
    ll = list(lines)
    if every:
        for k in range(0, len(ll), every):
            ll[k] = b"% comment"
    t = dev(b"\n".join(ll) + b"\n")
    off = wall_us(lambda: gs.parse_records_device(t, src, dst, val, 0, "long")) if pct == 0 else None
    on = wall_us(lambda: gs.parse_records_device(t, src, dst, val, 0, "long", False, True))
    out["comments_%d" % pct] = {"lines": len(ll), "flag_off_us": off, "flag_on_us": on}
    print("comments", pct, json.dumps(out["comments_%d" % pct]), flush=True)

# end to end: fold_into of a 2^20-line text beside fold of the host arrays
n = 1 << 20
w = rng.integers(1, 10 ** 6, n)
txt_ev = b"".join(b"%d %d %s\n" % (a, b, b"+" if e else b"-") for a, b, e in zip(sl[:n], dl[:n], el[:n]))
txt_w = b"".join(b"%d\t%d\t%d\n" % r for r in zip(sl[:n], dl[:n], w.tolist()))
dele_h = (1 - ev[:n]).astype(np.uint8)

def timed(fn, reps=3):
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return [round(x, 2) for x in t]

with gs.DegreeStream("all", vertex_hint=1 << 20) as D, gs.TextReader(third="event") as R:
    def f_text():
        D.reset(); R.fold_into(D, txt_ev); D.sync()
    def f_arr():
        D.reset(); D.fold(s[:n], d[:n], dele_h); D.sync()
    out["degstream_ms"] = {"text_bytes": len(txt_ev), "fold_into": timed(f_text), "fold_arrays": timed(f_arr)}
    print("degstream", json.dumps(out["degstream_ms"]), flush=True)
with gs.Matching(vertex_hint=1 << 20) as M, gs.TextReader(sep=gs.SEP_TAB, third="long") as R:
    def f_text():
        M.reset(); R.fold_into(M, txt_w); M.sync()
    def f_arr():
        M.reset(); M.fold(s[:n], d[:n], w); M.sync()
    out["matching_ms"] = {"text_bytes": len(txt_w), "fold_into": timed(f_text), "fold_arrays": timed(f_arr)}
    print("matching", json.dumps(out["matching_ms"]), flush=True)
with open(sys.argv[1] if len(sys.argv) > 1 else "profiles/text_bench.json", "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
