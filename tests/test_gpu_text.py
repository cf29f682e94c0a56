"""GPU: the field-spec text parse (gs_parse_records_device), the window bounds
(gs_window_bounds_device) and the text reader (gs_text_*, gsamd.TextReader) of include/gs_ingest.h.
Expected values come from the tests' model of the reference drivers' Java rules
(tests/text_model.py), which tests/test_text_seq.py ties to csrc/gs_text_seq.hpp, the header the
kernels include."""
import numpy as np
import pytest

import text_model as tm

pytestmark = pytest.mark.gpu

TILE = 16384   # bytes per parse workgroup (csrc/gs_ingest.hip kTile)
OVER = 512     # bytes of the next tile it stages (kOver)
REACH = 192    # a line's '\n' is looked for in three 64-byte segments


def _device_text(text, offset=0):
    import torch
    buf = torch.zeros(len(text) + offset, dtype=torch.uint8, device="cuda")
    if text:
        buf[offset:] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    return buf[offset:]


def _gpu_records(gs, text, sep=0, third=None, int32=False, comments=False, offset=0):
    """as tm.parse_text: (src, dst, third column, n_lines, n_records, bad_line)"""
    import torch
    cap = text.count(b"\n") + 1
    src = torch.zeros(cap, dtype=torch.int64, device="cuda")
    dst = torch.zeros(cap, dtype=torch.int64, device="cuda")
    col = torch.zeros(cap, dtype=torch.uint8 if third == "event" else torch.int64, device="cuda")
    nl, nr, bad = gs.parse_records_device(_device_text(text, offset), src, dst, col if third else None, sep, third,
                                          int32, comments)
    torch.cuda.synchronize()
    return src.cpu().numpy()[:nr], dst.cpu().numpy()[:nr], col.cpu().numpy()[:nr], nl, nr, bad


def _check(gs, text, sep, third, int32=False, comments=False, offset=0, what=None):
    want = tm.parse_text(text, sep, third, int32, comments)
    got = _gpu_records(gs, text, sep, third, int32, comments, offset)
    assert got[3:] == want[3:], (what, got[3:], want[3:])
    for k in range(3):
        if not np.array_equal(got[k], want[k]):
            i = int(np.flatnonzero(got[k] != want[k])[0])
            raise AssertionError((what, "column", k, "record", i, int(got[k][i]), int(want[k][i])))


# ---------------------------------------------------------------- parity with the two-field parse
@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("seed,nlines,offset", [(1, 50, 0), (2, 20000, 0), (4, 20000, 1), (5, 20000, 7)])
def test_no_third_field_is_the_two_field_parse(gs, sep, seed, nlines, offset):
    import torch
    rng = np.random.default_rng(seed)
    text = tm.random_text2(rng, nlines, sep)
    cap = text.count(b"\n") + 1
    view = _device_text(text, offset)
    a = [torch.zeros(cap, dtype=torch.int64, device="cuda") for _ in range(4)]
    n0, b0 = gs.parse_edges_device(view, a[0], a[1], sep)
    nl, nr, bad = gs.parse_records_device(view, a[2], a[3], None, sep)
    torch.cuda.synchronize()
    assert (nl, nr, bad) == (n0, n0, b0)
    assert torch.equal(a[0], a[2]) and torch.equal(a[1], a[3])


# ---------------------------------------------------------------- random texts in every mode
@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("third,int32,comments", [m for m in tm.MODES if m != (None, False, False)])
def test_random_texts_match_the_model(gs, sep, third, int32, comments):
    rng = np.random.default_rng(2000 + 100 * sep + 10 * tm.MODES.index((third, int32, comments)))
    text = tm.random_text3(rng, 20000, sep, third or "long", comments)
    _check(gs, text, sep, third, int32, comments, what="mixed")
    # no malformed line: GS_OK, bad_line -1, every row compared
    clean = tm.clean_text3(rng, 4000, sep, third or "event")
    assert tm.parse_text(clean, sep, third, int32, comments)[3:] == (4000, 4000, -1)
    _check(gs, clean, sep, third, int32, comments, offset=3, what="clean, unaligned")


def test_edge_case_texts(gs):
    for text in (b"", b"\n", b"1 2 3", b"1 2 3\n", b"1 2 3\n\n", b"\n1 2 3", b"1 2 3\r", b"1 2 +\r\n3 4 -\r\n", b"%",
                 b"%\n", b"%\r\n%", b"1 2 \n", b"1 2  x\n", b"-2147483648 2147483647 -9223372036854775808\n"):
        for sep in (0, 1):
            for third, int32, comments in tm.MODES[1:]:
                _check(gs, text, sep, third, int32, comments, what=(text, sep, third, int32, comments))


# ---------------------------------------------------------------- tile edges
def _filler(n, k, s, third, comments):
    """a line of n bytes, its '\\n' included: zero-padded "0..01 2 f", every fifth a comment"""
    if comments and k % 5 == 0:
        return b"%" + s + b"c" * (n - 3) + b"\n"
    tail = b"1" + s + b"2" + s + (b"+" if third == "event" and k % 2 else b"7") + b"\n"
    return b"0" * (n - len(tail)) + tail


def _text_with_line_at(start, special, end, s, third, comments):
    """filler lines of 30-80 bytes up to byte `start`, where `special` (with its '\\n') begins, then
    filler up to `end` bytes (cut there: the last line may lack its '\\n')"""
    out, k = bytearray(), 0
    while start - len(out) > 80:
        k += 1
        out += _filler(30 + (k * 7) % 21, k, s, third, comments)
    if start > len(out):
        out += _filler(start - len(out), 1, s, third, False)  # 30..80 bytes
    assert len(out) == start
    out += special
    while len(out) < end:
        k += 1
        out += _filler(30 + (k * 7) % 21, k, s, third, comments)
    return bytes(out[:end]) if end >= start + len(special) else bytes(out)


def _edge_lines(s, third):
    """(name, line, byte of the line that is put on the tile edge)"""
    f = b"+" if third == "event" else b"123456789"
    head = b"11" + s + b"22" + s
    long3 = head + (b"0" * 400 + b"7" if third == "long" else b"+" + s + b"x" * 400)
    return [
        ("separator before field 2 is the tile's last byte; field 2 starts the next tile", head + f, len(head)),
        ("field 2 straddles the edge", head + f, len(head) + len(f) // 2),
        ("field 2 ends at the tile's last byte", head + f, len(head) + len(f)),
        ("newline is the tile's last byte", head + f, len(head) + len(f) + 1),
        ("newline is the next tile's first byte", head + f, len(head) + len(f)),
        ("field 1 straddles the edge", head + f, 4),
        ("a line of more than 192 bytes starts right before the edge", long3, 3),
        ("a long line's field 2 crosses the edge", long3, len(head) + 200),
        ("empty field 2, then junk", head + s + b"x", len(head)),
        ("no field 2", b"11" + s + b"22" + s, 5),
    ]


@pytest.mark.parametrize("comments", [False, True])
@pytest.mark.parametrize("sep", [0, 1])
def test_third_field_at_tile_edges(gs, sep, comments):
    """Three tiles of text; the third field, its separator, its end and the line's newline on
    either side of the edges at 16384 and 32768; a field 2 that ends inside and just past the 512
    over-staged bytes (the per-character path over global memory); texts that end without
    '\\n', with '\\r' and with '\\r\\n'."""
    s = b"\t" if sep == 1 else b" "
    total = 3 * TILE
    for third in ("long", "event"):
        for edge in (TILE, 2 * TILE):
            for name, line, at in _edge_lines(s, third):
                text = _text_with_line_at(edge - at, line + b"\n", total, s, third, comments)
                _check(gs, text, sep, third, False, comments, what=(name, edge, third))
            # field 2 ends inside / just past the over-staged bytes of the tile its line starts in
            for end_at in (edge + OVER - 3, edge + OVER, edge + OVER + 5):
                start = edge - 10
                body = b"1" + s + b"2" + s
                pad = end_at - start - len(body) - 1
                line = body + (b"0" * pad + b"7" if third == "long" else b"-" + s + b"y" * (pad - 1))
                assert start + len(line) == end_at and len(line) > REACH
                text = _text_with_line_at(start, line + b"\n", total, s, third, comments)
                _check(gs, text, sep, third, False, comments, what=("over-staged", edge, end_at, third))
        # the text's end: the last line without '\n', with '\r', with '\r\n', a comment, at an edge
        for tail in (b"5" + s + b"6" + s + b"77", b"5" + s + b"6" + s + b"+\r", b"5" + s + b"6" + s + b"8\r\n",
                     b"5" + s + b"6", b"5" + s + b"6" + s, b"%", b"%\r", b"%" + s + b"end\r\n"):
            for start in (2 * TILE - 2, 2 * TILE, 2 * TILE + 100):
                text = _text_with_line_at(start, tail, 0, s, third, comments)
                assert text.endswith(tail)
                _check(gs, text, sep, third, False, comments, what=("tail", tail, start, third))


# ---------------------------------------------------------------- comment lines
def test_no_comment_line_skips_the_compaction(gs):
    rng = np.random.default_rng(31)
    text = tm.clean_text3(rng, 5000, 0, "long")
    p0, c0 = gs.testing_text_stats()
    _check(gs, text, 0, "long", False, True, what="no comment line")
    p1, c1 = gs.testing_text_stats()
    assert (p1 - p0, c1 - c0) == (1, 0)
    _check(gs, b"% one\n" + text, 0, "long", False, True, what="one comment line")
    p2, c2 = gs.testing_text_stats()
    assert (p2 - p1, c2 - c1) == (1, 1)


def test_comment_lines(gs):
    rng = np.random.default_rng(32)
    # every line a comment: no record
    text = b"".join([b"%\n", b"% a b c\n", b"%\r\n"][k % 3] for k in range(4000))
    got = _gpu_records(gs, text, 0, "event", False, True)
    assert got[3:] == (4000, 0, -1)
    # about one third of the lines, over more than three compaction tiles (1024 lines each), the
    # comment lines up to 300 bytes long (the per-character path never parses them)
    lines = tm.clean_text3(rng, 5000, 0, "long").split(b"\n")[:-1]
    for k in range(0, len(lines), 3):
        lines[k] = b"% " + b"z" * int(rng.integers(0, 300))
    assert len(lines) > 3 * gs.TEXT_TILE
    text = b"\n".join(lines) + b"\n"
    _check(gs, text, 0, "long", False, True, what="a third")
    # bad_line counts the comment lines, the records do not
    lines[3001] = b"1 2 x"
    want = tm.parse_text(b"\n".join(lines), 0, "long", False, True)
    assert want[5] == 3001 and want[4] == 5000 - len(range(0, 5000, 3))
    _check(gs, b"\n".join(lines), 0, "long", False, True, what="bad_line")
    # without the flag the first comment line is the malformed one
    assert _gpu_records(gs, text, 0, "long")[5] == 0
    # a comment as the first and as the last line of a tile
    for third in (None, "event"):
        s = b" "
        for at, name in ((0, "first line of a tile"), (2, "last line of a tile")):
            text = _text_with_line_at(TILE - at, b"%\n", 2 * TILE + 77, s, third or "long", True)
            _check(gs, text, 0, third, True, True, what=(name, third))
        text = _text_with_line_at(TILE - 100, b"% " + b"q" * 250 + b"\n", 2 * TILE, s, third or "long", True)
        _check(gs, text, 0, third, True, True, what=("a comment of more than 192 bytes over the edge", third))


# ---------------------------------------------------------------- the reader: chunks
def _read_all(gs, reader, text):
    cols = [[], [], []]
    sizes = []
    for src, dst, third, n in reader.chunks(text):
        cols[0].append(src.cpu().numpy().copy())
        cols[1].append(dst.cpu().numpy().copy())
        cols[2].append(third.cpu().numpy().copy() if third is not None else np.zeros(n, np.int64))
        sizes.append(n)
    return [np.concatenate(c) if c else np.zeros(0, np.int64) for c in cols], sizes


@pytest.mark.parametrize("third,comments", [("long", False), ("event", True), (None, True)])
def test_reader_chunks_equal_one_parse(gs, third, comments):
    rng = np.random.default_rng(41)
    lines = tm.clean_text3(rng, 20000, 0, third or "long").split(b"\n")[:-1]
    if comments:
        for k in range(3, len(lines), 7):
            lines[k] = [b"%", b"% a comment", b"%\r", b"%\t" + b"w" * 200][k % 4]
    text = b"\n".join(lines) + b"\n"
    assert len(text) > 3 * 65536
    want = tm.parse_text(text, 0, third, False, comments)
    assert want[5] == -1
    with gs.TextReader(third=third, comments=comments, chunk_bytes=65536) as reader:
        for _ in range(2):  # a second open reuses the reader
            got, sizes = _read_all(gs, reader, text)
            assert len(sizes) >= 4 and sum(sizes) == want[4]
            for g, w in zip(got, want[:3]):
                assert np.array_equal(g, w)
            assert reader.position() == (want[3], want[4], -1)
        # a comment as the last line of one chunk and the first of the next
        if comments:
            lines = text.split(b"\n")[:-1]
            at, k = 0, 0
            while at + len(lines[k]) + 1 <= 65536:
                at += len(lines[k]) + 1
                k += 1
            lines[k - 1] = b"%" + b" " * (len(lines[k - 1]) - 1)  # the same lengths: the same cut
            lines[k] = b"%" + b" " * (len(lines[k]) - 1)
            text2 = b"\n".join(lines) + b"\n"
            want2 = tm.parse_text(text2, 0, third, False, comments)
            assert want2[3:] == (want[3], want[4] - 2 + (k - 1 in range(3, len(lines), 7)) + (k in range(3, len(lines), 7)), -1)
            got, sizes = _read_all(gs, reader, text2)
            assert sum(sizes) == want2[4] and all(np.array_equal(g, w) for g, w in zip(got, want2[:3]))


def test_reader_errors(gs):
    rng = np.random.default_rng(42)
    text = tm.clean_text3(rng, 13000, 0, "long")
    lines = text.split(b"\n")[:-1]
    k = 2 * 65536 // (len(text) // len(lines)) + 300  # a line inside the third chunk
    assert 2 * 65536 < sum(len(x) + 1 for x in lines[:k]) < 3 * 65536
    lines[k] = b"1 2 x"
    bad_text = b"\n".join(lines) + b"\n"
    with gs.TextReader(third="long", chunk_bytes=65536) as reader:
        delivered = 0
        with pytest.raises(gs.GSError) as e:
            for src, dst, val, n in reader.chunks(bad_text):
                delivered += 1
        assert e.value.code == gs.GS_ERR_PARSE and str(k) in str(e.value)
        assert delivered == 2 and reader.position()[2] == k
        # a line longer than a chunk
        with pytest.raises(gs.GSError) as e:
            list(reader.chunks(b"1 2 3\n" + b"1 2 " + b"0" * 70000 + b"\n"))
        assert e.value.code == gs.GS_ERR_INVALID
        # the reader still works
        got, sizes = _read_all(gs, reader, text)
        assert sum(sizes) == 13000
        assert list(reader.chunks(b"")) and reader.position() == (0, 0, -1)
        with pytest.raises(gs.GSError) as e:  # no open text
            reader._next()
        assert e.value.code == gs.GS_ERR_INVALID


# ---------------------------------------------------------------- windows
def _gpu_bounds(gs, ts, size):
    import torch
    t = torch.tensor(np.asarray(ts, np.int64), device="cuda")
    first = torch.zeros(len(ts), dtype=torch.int64, device="cuda")
    window = torch.zeros(len(ts), dtype=torch.int64, device="cuda")
    nw = gs.window_bounds_device(t, size, first, window)
    torch.cuda.synchronize()
    return first.cpu().numpy()[:nw], window.cpu().numpy()[:nw]


def test_window_bounds(gs):
    rng = np.random.default_rng(51)
    n = 3 * gs.TEXT_TILE + 77  # crosses three compaction tiles
    cases = [([5], 10), ([-5], 10), (np.full(n, 123), 1000), (np.arange(n) * 10, 10), (np.arange(n) * 10, 7),
             (np.repeat(np.arange(-40, 40), 41), 1), (rng.integers(-5000, 5000, n), 37),
             (np.sort(rng.integers(0, 10 ** 6, n)), 1000), ([-1, 0, 1, -99, -100, -101, 99, 100], 100),
             ([tm.I64_MIN, tm.I64_MIN + 1, -1, 0, tm.I64_MAX - 1, tm.I64_MAX], tm.I64_MAX)]
    for ts, size in cases:
        first, window = _gpu_bounds(gs, ts, size)
        wf, ww = tm.window_bounds(list(np.asarray(ts).tolist()), size)
        assert np.array_equal(first, wf) and np.array_equal(window, ww), (len(ts), size)
    # more windows than the arrays hold: the count is still the whole count
    import torch
    t = torch.arange(0, 100, dtype=torch.int64, device="cuda")
    small = torch.zeros(10, dtype=torch.int64, device="cuda")
    assert gs.window_bounds_device(t, 1, small, small.clone()) == 100


def test_reader_delivers_whole_windows(gs):
    """chunk_bytes = 65536 (about 4000 lines): windows inside a chunk, one that spans two chunks,
    one that spans more than three (the held-back records outgrow the columns), and the final
    partial window, delivered by the last call."""
    rng = np.random.default_rng(52)
    runs = [100] * 30 + [3500] + [50] * 20 + [15000] + [7] * 40 + [1234]
    ts = np.concatenate([np.full(r, 1000 * k + 3, np.int64) + rng.integers(0, 900, r) for k, r in enumerate(runs)])
    src = rng.integers(0, 10 ** 6, len(ts))
    dst = rng.integers(0, 10 ** 6, len(ts))
    text = b"".join(b"%d %d %d\n" % (a, b, t) for a, b, t in zip(src.tolist(), dst.tolist(), ts.tolist()))
    assert len(text) > 5 * 65536
    wf, ww = tm.window_bounds(ts.tolist(), 1000)
    assert len(wf) == len(runs)
    with gs.TextReader(third="long", chunk_bytes=65536) as reader:
        for _ in range(2):
            got = [(w, s.cpu().numpy().copy(), d.cpu().numpy().copy(), v.cpu().numpy().copy(), n)
                   for w, s, d, v, n in reader.windows(text, 1000)]
            assert [g[0] for g in got] == ww.tolist() and [g[4] for g in got] == runs
            assert np.array_equal(np.concatenate([g[1] for g in got]), src)
            assert np.array_equal(np.concatenate([g[2] for g in got]), dst)
            assert np.array_equal(np.concatenate([g[3] for g in got]), ts)
        # windows off again: plain chunks
        assert sum(n for _, _, _, n in reader.chunks(text)) == len(ts)
    with gs.TextReader(third="event") as reader:
        with pytest.raises(ValueError):
            next(reader.windows(text, 1000))
        assert gs.lib().gs_text_set_window(reader.handle, 10) == gs.GS_ERR_INVALID


# ---------------------------------------------------------------- look-back
def test_three_field_parse_under_the_lookback_fallback(gs, knobs):
    """The look-back is the two-field parse's, shared: with a timeout of 0 every tile that finds an
    unpublished predecessor counts the lines before it itself, and the three-field kernel's line
    numbers are still the model's."""
    rng = np.random.default_rng(61)
    knobs(parse_lb_timeout_us=0)
    text = tm.random_text3(rng, 30000, 0, "long", True)
    _check(gs, text, 0, "long", False, True, offset=1, what="timeout 0")
