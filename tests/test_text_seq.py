"""CPU: the rules of the field-spec text ingest (csrc/gs_text_seq.hpp, the header the parse kernels
include) in a stand-alone program built with the address and undefined-behaviour sanitizers
(tests/cpp/text_seq_sanitize.cpp): against the oracle's two-field parse, against the tests' own
model of Java's split / parseLong / parseInt (tests/text_model.py, which the GPU tests take their
expected values from), on the rule cases of include/gs_ingest.h spelled out, on window bounds, and
on the reference's pinned DEGREES_DATA text."""
import json
import os
import subprocess

import numpy as np
import pytest

import text_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIRD = {None: 0, "long": 1, "event": 2}


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    """run(args...) -> stdout of the sanitizer-built program; any sanitizer report fails."""
    d = tmp_path_factory.mktemp("text_seq")
    exe = str(d / "text_seq_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                            "-I" + os.path.join(ROOT, "gelly-streaming_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "text_seq_sanitize.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    # a preloaded library may precede the ASan runtime: do not treat that as an error
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    count = [0]

    def run(data, *args):
        count[0] += 1
        path = str(d / ("in%d" % count[0]))
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([exe, args[0], path] + [str(a) for a in args[1:]], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        return r.stdout
    return run


def _parse(san, text, sep, third, int32, comments):
    out = san(text, "parse", sep, THIRD[third], (1 if int32 else 0) | (2 if comments else 0)).splitlines()
    head = out[0].split()
    assert head[0::2] == ["lines", "records", "bad"]
    n_lines, n_records, bad = int(head[1]), int(head[3]), int(head[5])
    rows = np.array([[int(x) for x in ln.split()] for ln in out[1:]], np.int64).reshape(-1, 4)
    assert len(rows) == n_records
    col = rows[:, 3].astype(np.uint8) if third == "event" else rows[:, 2]
    return rows[:, 0], rows[:, 1], col, n_lines, n_records, bad


def _same(got, want, what):
    assert got[3:] == want[3:], (what, got[3:], want[3:])
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w), what


@pytest.mark.parametrize("sep", [0, 1])
def test_two_field_texts_agree_with_the_oracle(san, oracle_mod, sep):
    rng = np.random.default_rng(100 + sep)
    for nlines in (0, 1, 40, 3000):
        text = tm.random_text2(rng, nlines, sep)
        es, ed, en, eb = oracle_mod.parse_edges(text, sep)
        s, d, _, n, r, b = _parse(san, text, sep, None, False, False)
        assert (n, r, b) == (en, en, eb)
        assert np.array_equal(s, es) and np.array_equal(d, ed)
        # and the model, which the GPU tests trust, says the same
        _same(tm.parse_text(text, sep), (es, ed, np.zeros(en, np.int64), en, en, eb), (sep, nlines))


@pytest.mark.parametrize("sep", [0, 1])
@pytest.mark.parametrize("third,int32,comments", tm.MODES)
def test_three_field_texts_agree_with_the_model(san, sep, third, int32, comments):
    rng = np.random.default_rng(1000 + 100 * sep + 10 * THIRD[third] + 2 * int32 + comments)
    texts = [tm.random_text3(rng, 1500, sep, third or "long", comments),
             tm.random_text3(rng, 300, sep, third or "event", comments, p_bad=0.0), tm.random_text2(rng, 300, sep)]
    for text in texts:
        _same(_parse(san, text, sep, third, int32, comments), tm.parse_text(text, sep, third, int32, comments),
              (sep, third, int32, comments))


# the rule cases of include/gs_ingest.h: (text, sep, third, int32, comments) -> what the line gives:
# "bad", "skip", or the record (src, dst, third value)
RULES = [
    # fields 0 and 1, Integer.parseInt
    (b"2147483647 -2147483648", 0, None, True, False, (2147483647, -2147483648, 0)),
    (b"2147483648 1", 0, None, True, False, "bad"),
    (b"1 -2147483649", 0, None, True, False, "bad"),
    (b"2147483648 1", 0, None, False, False, (2147483648, 1, 0)),
    (b"1 2 9223372036854775807", 0, "long", True, False, (1, 2, 9223372036854775807)),  # a LONG field stays long
    (b"1 2 9223372036854775808", 0, "long", False, False, "bad"),
    (b"1 2 -9223372036854775808", 0, "long", False, False, (1, 2, -9223372036854775808)),
    (b"1 2 -9223372036854775809", 0, "long", False, False, "bad"),
    # existence and extent of field 2
    (b"1 2  x", 0, "event", False, False, (1, 2, 1)),  # an empty field 2: a deletion
    (b"1 2  x", 0, "long", False, False, "bad"),       # ... and no Long.parseLong argument
    (b"1 2 ", 0, "event", False, False, "bad"),        # none
    (b"1 2", 0, "event", False, False, "bad"),
    (b"1 2 ", 0, "long", False, False, "bad"),
    (b"1 2", 0, "long", False, False, "bad"),
    (b"1 2   ", 0, "event", False, False, "bad"),      # trailing empties only
    (b"1 2 5 junk", 0, "long", False, False, (1, 2, 5)),  # later fields are ignored
    (b"1 2 +5", 0, "long", False, False, (1, 2, 5)),
    (b"1 2 5\r", 0, "long", False, False, (1, 2, 5)),
    (b"1 2 5x", 0, "long", False, False, "bad"),
    (b"1\t2\t 5", 1, "long", False, False, "bad"),     # tab mode: the field is " 5"
    (b"1\t2\t5", 1, "long", False, False, (1, 2, 5)),
    (b"1 2 5", 1, "long", False, False, "bad"),
    # events
    (b"1 2 +", 0, "event", False, False, (1, 2, 0)),
    (b"1 2 -", 0, "event", False, False, (1, 2, 1)),
    (b"1 2 ++", 0, "event", False, False, (1, 2, 1)),
    (b"1 2 + -", 0, "event", False, False, (1, 2, 0)),
    (b"1 2 +\r", 0, "event", False, False, (1, 2, 0)),
    (b"1 2 anything", 0, "event", False, False, (1, 2, 1)),
    (b"1\t2\t\t+", 1, "event", False, False, (1, 2, 1)),
    (b"1\t2\t+ ", 1, "event", False, False, (1, 2, 1)),  # tab mode: the field is "+ "
    # comment lines
    (b"%", 0, None, False, True, "skip"),
    (b"% a comment", 0, "long", False, True, "skip"),
    (b"%\r", 0, "event", False, True, "skip"),
    (b"%\tx", 1, None, False, True, "skip"),
    (b"% x", 1, None, False, True, "bad"),   # tab mode: field 0 is "% x"
    (b"%foo", 0, None, False, True, "bad"),
    (b" % x", 0, None, False, True, "bad"),
    (b"%", 0, None, False, False, "bad"),    # without the flag a comment line is malformed
    (b"", 0, None, False, True, "bad"),
]


def test_rule_cases_give_the_listed_verdicts(san):
    for text, sep, third, int32, comments, want in RULES:
        for tail in (b"", b"\n") if text else (b"\n",):  # (the empty line exists only before a '\n')
            got = _parse(san, text + tail, sep, third, int32, comments)
            model = tm.parse_text(text + tail, sep, third, int32, comments)
            _same(got, model, text)
            s, d, col, n_lines, n_records, bad = got
            assert n_lines == 1, text
            if want == "skip":
                assert (n_records, bad) == (0, -1), text
            elif want == "bad":
                assert (n_records, bad) == (1, 0), text
            else:
                assert (n_records, bad) == (1, -1) and (int(s[0]), int(d[0]), int(col[0])) == want, text
    # comment lines count as lines: the malformed line's index counts them, the records do not
    text = b"% one\n1 2 5\n%\n3 4 x\n5 6 7\n"
    s, d, col, n_lines, n_records, bad = _parse(san, text, 0, "long", False, True)
    assert (n_lines, n_records, bad) == (5, 3, 3)
    assert s.tolist() == [1, 0, 5] and col.tolist() == [5, 0, 7]


def test_window_bounds(san):
    rng = np.random.default_rng(7)
    cases = [([5], 10), (list(range(0, 100, 3)), 10), ([7, 7, 7, 8, 9, 9, 10], 1), ([0, 399, 400, 401, 799, 800, 1199], 400),
             ([500, 100, 450, 40, 30, 900, 50], 100), ([-1, 0, 1, -99, -100, -101, 99, 100], 100),
             (rng.integers(-5000, 5000, 300).tolist(), 37), (np.sort(rng.integers(0, 10 ** 6, 500)).tolist(), 1000)]
    for ts, size in cases:
        out = san(b"".join(b"%d\n" % t for t in ts), "windows", size).splitlines()
        assert out[0].split()[0] == "windows"
        rows = np.array([[int(x) for x in ln.split()] for ln in out[1:]], np.int64).reshape(-1, 2)
        first, window = tm.window_bounds(ts, size)
        assert int(out[0].split()[1]) == len(first)
        assert np.array_equal(rows[:, 0], first) and np.array_equal(rows[:, 1], window), (ts, size)
    # truncating division: -1 and 1 share window 0 (Flink's floor would put -1 into window -1)
    assert tm.window_bounds([-1, 1], 100)[1].tolist() == [0]


def test_degree_pin_text_gives_its_six_events(san):
    """util/ExamplesTestData.java DEGREES_DATA, taken in as the reference takes it: as lines."""
    with open(os.path.join(ROOT, "tests", "golden", "degree_pins.json")) as f:
        pins = json.load(f)
    text = pins["degrees_data"]["text"].encode()
    s, d, dele, n_lines, n_records, bad = _parse(san, text, 0, "event", True, False)
    assert (n_lines, n_records, bad) == (6, 6, -1)
    assert list(zip(s.tolist(), d.tolist(), dele.tolist())) == [(1, 2, 0), (2, 3, 0), (1, 4, 0), (2, 3, 1), (3, 4, 0),
                                                                (1, 2, 1)]
    zero = pins["degrees_data_zero"]["text"].encode()
    got = _parse(san, zero, 0, "event", True, False)
    _same(got, tm.parse_text(zero, 0, "event", True), "degrees_data_zero")
    assert got[5] == -1 and got[4] == len(zero.strip().split(b"\n"))


def test_kernels_include_the_checked_header():
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_ingest.hip")) as f:
        text = f.read()
    assert '#include "gs_text_seq.hpp"' in text
    for fn in ("txt_is_comment(", "txt_event_field(", "txt_int32_ok(", "txt_window_opens(", "txt_window_of(",
               "txt_mode_third(", "txt_mode_int32(", "txt_mode_comment(", "txt_tiles(", "txt_row_first("):
        assert fn in text, fn
