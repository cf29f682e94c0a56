"""bench.py --dump-outputs on CPU: the writer of the .npy files (dump_outputs). 64-bit ids
must survive the float64 files exactly, the rows must not depend on the order the library
emitted them in, and the sample of a long output must be the same from run to run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("gs_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load(d, col):
    hi = np.load(os.path.join(d, col + "_hi32.npy"))
    lo = np.load(os.path.join(d, col + "_lo32.npy"))
    assert hi.dtype == np.float64 and lo.dtype == np.float64
    return ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)).view(np.int64)


def test_plain_run_is_the_default(monkeypatch):
    """--full is off unless asked for, and a plain run writes nothing."""
    bench = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_rows_exact_and_independent_of_emission_order(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(7)
    v = np.unique(rng.integers(-(1 << 63), (1 << 63) - 1, 5000, dtype=np.int64))  # all 64 bits in use
    v = np.concatenate([v, np.array([-1, 0, (1 << 63) - 1, -(1 << 63), (1 << 53) + 1], np.int64)])
    v = np.unique(v)
    lab = v[::-1].copy()
    for k, perm in enumerate((np.arange(len(v)), rng.permutation(len(v)))):
        d = str(tmp_path / ("o%d" % k))
        bench.dump_outputs(d, {"vertex": v[perm], "label": lab[perm]}, scalars={"flag": 1.0})
        assert np.array_equal(_load(d, "vertex"), v)  # sorted by vertex, bit-exact
        assert np.array_equal(_load(d, "label"), lab)
        assert np.load(os.path.join(d, "rows.npy")).tolist() == [float(len(v))]
        assert np.load(os.path.join(d, "flag.npy")).tolist() == [1.0]


def test_long_output_keeps_a_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_ROWS", 64)
    n = 1000
    v = np.arange(n, dtype=np.int64) * 3 + (1 << 40)
    perm = np.random.default_rng(1).permutation(n)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, {"vertex": v, "label": v + 1})
    bench.dump_outputs(b, {"vertex": v[perm], "label": v[perm] + 1})
    va, vb = _load(a, "vertex"), _load(b, "vertex")
    assert len(va) == 64 and np.array_equal(va, vb)
    assert np.all(np.diff(va) >= 0) and np.isin(va, v).all()
    assert np.array_equal(_load(a, "label"), va + 1) and np.array_equal(_load(b, "label"), va + 1)
    assert np.load(os.path.join(a, "rows.npy")).tolist() == [float(n)]
    # unsorted outputs (a stream's own order) keep their order
    c = str(tmp_path / "c")
    bench.dump_outputs(c, {"src": v[perm]}, sort=False, rank=1, world=2)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, 64))
    hi = np.load(os.path.join(c, "src_hi32_rank1.npy"))
    lo = np.load(os.path.join(c, "src_lo32_rank1.npy"))
    got = ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)).view(np.int64)
    assert np.array_equal(got, v[perm][idx])
