"""GPU, end to end: text in, a summary out. The reference's pinned inputs taken in as its drivers
take them, as lines (DEGREES_DATA through DegreeStream, TRIANGLES_DATA through event-time windows
and Triangles), TextReader.fold_into of a text against fold of the same arrays for every handle
type, and WindowTriangles::runText of the C++ host mirror (tests/cpp/test_text.cpp)."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gelly-streaming_amd", "host", "bin")


def _pins(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.mark.parametrize("chunk_bytes", [0, 16])
@pytest.mark.parametrize("data,result", [("degrees_data", "degrees_result"), ("degrees_data_zero", "degrees_result_zero")])
def test_degree_pins_from_their_text(gs, data, result, chunk_bytes):
    """util/ExamplesTestData.java DEGREES_DATA -> every (degree,count) record DEGREES_RESULT lists,
    in order; with 16-byte chunks (two lines each) the records are read chunk by chunk."""
    pins = _pins("degree_pins.json")
    text = pins[data]["text"].encode()
    got, sizes = [], []

    def each(n):
        sizes.append(n)
        _, d, c = D.records()
        got.extend("(%d,%d)" % (a, b) for a, b in zip(d.tolist(), c.tolist()))

    with gs.DegreeStream("all", vertex_hint=16) as D, gs.TextReader(third="event", int32=True,
                                                                     chunk_bytes=chunk_bytes) as R:
        assert R.fold_into(D, text, each) == len(text.split(b"\n"))
    assert got == pins[result]["text"].split("\n")
    assert len(sizes) == (1 if chunk_bytes == 0 else (len(text.split(b"\n")) + 1) // 2)


def test_triangle_pin_from_its_text(gs):
    """TRIANGLES_DATA as "src trg timestamp" lines -> 400 ms windows -> (count, window.maxTimestamp())."""
    pins = _pins("triangle_pins.json")
    text = b"".join(b"%d %d %d\n" % tuple(e) for e in pins["triangles_data"]["edges"])
    size = pins["triangles_result"]["window_ms"]
    for chunk_bytes in (0, 40):
        rows = []
        with gs.Triangles(edge_hint=64) as T, gs.TextReader(third="long", chunk_bytes=chunk_bytes) as R:
            for w, src, dst, ts, n in R.windows(text, size):
                assert n > 0 and all(t // size == w for t in ts.cpu().tolist())
                rows.append([T.window(src.cpu().numpy(), dst.cpu().numpy()), (w + 1) * size - 1])
        assert sorted(rows) == sorted(pins["triangles_result"]["rows"]) == [[2, 399], [2, 1199], [3, 799]]


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.fixture(scope="module")
def rmat(oracle_mod):
    s, d = oracle_mod.rmat_edges(0x5EED0A10, 10, 0, 1 << 12, False)  # ids 0 .. 1023: repeated edges, triangles
    rng = np.random.default_rng(71)
    return s, d, rng.integers(1, 10 ** 6, len(s)), rng


def _text(s, d, third=None, sep=b" "):
    cols = [s.tolist(), d.tolist()] + ([list(third)] if third is not None else [])
    return b"".join(sep.join(b"%d" % x if not isinstance(x, bytes) else x for x in row) + b"\n" for row in zip(*cols))


CASES = {
    "Spanner": (lambda gs: gs.Spanner(k=3), lambda h: (h.count(), h.edges())),
    "Distinct": (lambda gs: gs.Distinct(), lambda h: (h.size(), h.vertices(), h.edges())),
    "TriangleStream": (lambda gs: gs.TriangleStream(), lambda h: (h.count(), h.local_counts())),
    "TriangleSampler": (lambda gs: gs.TriangleSampler(samples=256, vertices=1 << 10), lambda h: (h.estimate(), h.states())),
    "Summary": (lambda gs: gs.Summary("cc", capacity_hint=1 << 12), lambda h: h.labels()),
    "Triangles": (lambda gs: gs.Triangles(edge_hint=1 << 12), lambda h: (h.count(), h.local_counts())),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fold_into_equals_fold_of_the_arrays(gs, rmat, name):
    s, d, _, _ = rmat
    make, read = CASES[name]
    text = _text(s, d)
    with make(gs) as a, make(gs) as b, gs.TextReader(chunk_bytes=8192) as R:
        chunks = []
        assert R.fold_into(a, text, chunks.append) == len(s)
        assert len(chunks) > 3 and sum(chunks) == len(s)
        at = 0
        for n in chunks:  # the same cuts: a stream handle's per-fold results are the same too
            b.fold(s[at:at + n], d[at:at + n])
            at += n
        assert _same(read(a), read(b))


def test_matching_from_tab_separated_weights(gs, rmat):
    s, d, w, _ = rmat
    text = _text(s, d, w.tolist(), b"\t")
    with gs.Matching(vertex_hint=1 << 10) as a, gs.Matching(vertex_hint=1 << 10) as b:
        with gs.TextReader(sep=gs.SEP_TAB, third="long", chunk_bytes=8192) as R:
            chunks = []
            assert R.fold_into(a, text, chunks.append) == len(s) and len(chunks) > 3
        b.fold(s, d, w)
        assert _same(a.count(), b.count()) and _same(a.edges(), b.edges())
        with gs.TextReader(third="long") as R:  # the text is tab-separated: a whitespace reader splits it too
            a.reset()
            assert R.fold_into(a, text) == len(s) and _same(a.edges(), b.edges())


def test_degrees_with_deletions_from_events(gs, rmat):
    s, d, _, rng = rmat
    again = rng.permutation(len(s))[: len(s) // 4]
    es, ed = np.concatenate([s, s[again]]), np.concatenate([d, d[again]])
    dele = np.concatenate([np.zeros(len(s), np.uint8), np.ones(len(again), np.uint8)])
    text = _text(es, ed, [b"-" if x else b"+" for x in dele.tolist()])
    with gs.Degrees("all", capacity_hint=1 << 12) as a, gs.Degrees("all", capacity_hint=1 << 12) as b:
        with gs.TextReader(third="event", chunk_bytes=8192) as R:
            assert R.fold_into(a, text) == len(es)
        b.fold(es, ed, dele)
        assert _same(a.degrees(), b.degrees()) and _same(a.distribution(), b.distribution())
    with gs.DegreeStream("out") as a, gs.DegreeStream("out") as b, gs.TextReader() as R:  # no third field: additions
        assert R.fold_into(a, _text(s, d)) == len(s)
        b.fold(s, d)
        assert _same(a.degrees(), b.degrees())


def test_text_on_host_mirror():
    exe = os.path.join(BIN, "test_text")
    assert os.path.exists(exe), "host mirror not built (run __graft_entry__.build())"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("WindowTriangles.runText", "WindowTriangles.runText equals run", "WindowTriangles.runText tab and CRLF",
                 "WindowTriangles.runText small chunks", "WindowTriangles.runText empty",
                 "WindowTriangles.runText malformed line throws", "TextReader.events and comments"):
        assert "PASS " + name in r.stdout
    assert "0 failure(s)" in r.stdout
