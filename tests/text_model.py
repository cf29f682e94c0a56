"""The tests' own model of the field-spec text ingest (include/gs_ingest.h): Java's split,
Long.parseLong / Integer.parseInt and the reference drivers' third-field rules, written from the
Java semantics with Python's bytes and ints (no code shared with csrc/gs_text_seq.hpp, which
tests/test_text_seq.py ties to this model), and the generators of the texts the CPU and GPU tests
share. Not a test module."""
import re

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
WHITESPACE = b" \t\n\x0b\x0c\r"  # Java regex \s
_NUMBER = re.compile(rb"[+-]?[0-9]+\Z")

MODES = [(third, int32, comments) for third in (None, "long", "event") for int32 in (False, True)
         for comments in (False, True)]


def java_split(s, sep):
    """String.split(regex) with limit 0 on a one-character class: every separator cuts, trailing
    empty strings are dropped, a string without a separator is returned whole."""
    seps = b"\t" if sep == 1 else WHITESPACE
    parts, cur, cut = [], bytearray(), False
    for c in s:
        if c in seps:
            parts.append(bytes(cur))
            cur = bytearray()
            cut = True
        else:
            cur.append(c)
    if not cut:
        return [bytes(s)]
    parts.append(bytes(cur))
    while parts and parts[-1] == b"":
        parts.pop()
    return parts


def parse_number(f, lo, hi):
    """Long.parseLong / Integer.parseInt of ASCII input: the value, or None where Java throws."""
    if not _NUMBER.match(f):
        return None
    v = int(f)
    return v if lo <= v <= hi else None


def parse_line(line, sep, third, int32, comments):
    """"skip", None (malformed) or (src, dst, third value)."""
    if line.endswith(b"\r"):
        line = line[:-1]
    f = java_split(line, sep)
    if comments and f and f[0] == b"%":
        return "skip"
    if len(f) < 2:
        return None
    lo, hi = (I32_MIN, I32_MAX) if int32 else (I64_MIN, I64_MAX)
    a, b = parse_number(f[0], lo, hi), parse_number(f[1], lo, hi)
    if a is None or b is None:
        return None
    if third is None:
        return a, b, 0
    if len(f) < 3:
        return None
    if third == "long":
        v = parse_number(f[2], I64_MIN, I64_MAX)
        return None if v is None else (a, b, v)
    return a, b, 0 if f[2] == b"+" else 1


def lines_of(text):
    lines = bytes(text).split(b"\n")
    if lines[-1] == b"":  # no line after a final '\n', none in an empty text
        lines.pop()
    return lines


def parse_text(text, sep=0, third=None, int32=False, comments=False):
    """(src, dst, third column, n_lines, n_records, bad_line): a malformed line keeps a zero row."""
    src, dst, col, bad = [], [], [], -1
    lines = lines_of(text)
    for i, line in enumerate(lines):
        r = parse_line(line, sep, third, int32, comments)
        if r == "skip":
            continue
        if r is None:
            if bad < 0:
                bad = i
            r = (0, 0, 0)
        src.append(r[0])
        dst.append(r[1])
        col.append(r[2])
    dt = np.uint8 if third == "event" else np.int64
    return (np.array(src, np.int64), np.array(dst, np.int64), np.array(col, dt), len(lines), len(src), bad)


def window_of(ts, size):
    """C++ truncating division."""
    q = abs(int(ts)) // int(size)
    return -q if ts < 0 else q


def window_bounds(ts, size):
    """(first, window): the maximal runs of consecutive records with equal window id."""
    first, window = [], []
    for i, t in enumerate(ts):
        w = window_of(t, size)
        if i == 0 or w != window_of(ts[i - 1], size):
            first.append(i)
            window.append(w)
    return np.array(first, np.int64), np.array(window, np.int64)


# ---------------------------------------------------------------- generators
LIMITS = [b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809",
          b"2147483647", b"2147483648", b"-2147483648", b"-2147483649"]


def random_text2(rng, nlines, sep):
    """Two-field texts of the shape of tests/test_gpu_ingest.py's _random_text."""
    s = b"\t" if sep == 1 else b" "
    seps = [b" ", b"\t", b"\x0b", b"\x0c"] if sep == 0 else [b"\t"]
    good_vals = [0, 1, -1, 7, I64_MAX, I64_MIN, 123456789012345678]
    lines = []
    for _ in range(nlines):
        r = rng.random()
        a = int(rng.choice(good_vals)) if rng.random() < 0.2 else int(rng.integers(-(10 ** 12), 10 ** 12))
        b = int(rng.integers(-(10 ** 18), 10 ** 18))
        sp = seps[int(rng.integers(len(seps)))]
        if r < 0.80:
            ln = b"%d%s%d" % (a, sp, b)
        elif r < 0.85:
            ln = b"+%d%s%d" % (abs(a), sp, b)
        elif r < 0.88:
            ln = b"%d%s%d%s%s" % (a, sp, b, s, b"x" * int(rng.integers(1, 700)))
        elif r < 0.91:
            ln = b"%d%s%d\r" % (a, sp, b)
        elif r < 0.93:
            ln = b"%d%s%d%s" % (a, sp, b, sp)
        else:
            bad = [b"", b"%d" % a, s + b"%d%s%d" % (a, s, b), b"%d%s%s%d" % (a, s, s, b), b"%da%s%d" % (a, s, b),
                   b"9223372036854775808%s1" % s, b"-%s5" % s, b"1%s-9223372036854775809" % s]
            ln = bad[int(rng.integers(len(bad)))]
        lines.append(ln)
    text = b"\n".join(lines)
    if rng.random() < 0.5:
        text += b"\n"
    return text


def random_text3(rng, nlines, sep, third, comments=False, p_bad=0.08):
    """Three-field texts: valid values, '+' / '-' events, missing, empty, signed and '\\r'-ended
    third fields, trailing separators, third fields of 24-700 bytes (leading zeros, junk), the
    int64 and int32 limits and their neighbours in every field, and comment lines."""
    s = b"\t" if sep == 1 else b" "
    seps = [b" ", b"\t", b"\x0b", b"\x0c"] if sep == 0 else [b"\t"]

    def endpoint():
        r = rng.random()
        if r < 0.05:
            return LIMITS[int(rng.integers(len(LIMITS)))]
        if r < 0.6:
            return b"%d" % int(rng.integers(-(10 ** 9), 10 ** 9))
        return b"%d" % int(rng.integers(-(10 ** 12), 10 ** 12))

    def field3():
        r = rng.random()
        if third == "event" and r < 0.6:
            return [b"+", b"-"][int(rng.integers(2))]
        if r < 0.5:
            return b"%d" % int(rng.integers(-(10 ** 15), 10 ** 15))
        if r < 0.58:
            return LIMITS[int(rng.integers(len(LIMITS)))]
        if r < 0.64:
            return b"+%d" % int(rng.integers(0, 10 ** 10))
        if r < 0.70:  # 24 - 700 bytes: leading zeros (a valid long), or junk
            n = int(rng.integers(24, 700))
            return b"0" * (n - 3) + b"%03d" % int(rng.integers(1000)) if rng.random() < 0.5 else b"7" * (n - 1) + b"x"
        if r < 0.76:
            return [b"+", b"-", b"++", b"+x", b"x", b"+1", b"-0"][int(rng.integers(7))]
        return b"%d" % int(rng.integers(0, 2000))

    lines = []
    for _ in range(nlines):
        sp = seps[int(rng.integers(len(seps)))]
        sp2 = seps[int(rng.integers(len(seps)))]
        core = endpoint() + sp + endpoint()
        r = rng.random()
        if comments and r < 0.06:
            ln = [b"%", b"%" + s + b"a comment", b"%" + s, b"%\r", b"%foo", s + b"%" + s + b"x",
                  b"%" + s + b"y" * 300][int(rng.integers(7))]
        elif r < 1.0 - p_bad:
            ln = core + sp2 + field3()
            t = rng.random()
            if t < 0.05:
                ln += b"\r"
            elif t < 0.10:
                ln += sp2  # trailing separator
            elif t < 0.15:
                ln += sp2 + b"ignored" + sp2 + b"fields"
        else:
            ln = [core, core + sp2, core + sp2 + sp2, core + sp2 + sp2 + b"x", core + sp2 + b" 5", core + b"\r",
                  core + sp2 + b"\r", b"", endpoint(), sp + core + sp2 + b"1", core + b"x" + sp2 + b"1",
                  core + sp2 + b"12a", core + sp2 + b"-"][int(rng.integers(13))]
        lines.append(ln)
    text = b"\n".join(lines)
    if rng.random() < 0.5:
        text += b"\n"
    return text


def clean_text3(rng, nlines, sep, third, ts_step=0):
    """Well-formed three-field lines only (no malformed line, no comment)."""
    s = b"\t" if sep == 1 else b" "
    out, ts = [], 0
    for _ in range(nlines):
        a, b = int(rng.integers(0, 5000)), int(rng.integers(0, 5000))
        if third == "event":
            f = [b"+", b"-"][int(rng.integers(2))]
        elif ts_step:
            ts += int(rng.integers(0, ts_step))
            f = b"%d" % ts
        else:
            f = b"%d" % int(rng.integers(-(10 ** 15), 10 ** 15))
        out.append(b"%d%s%d%s%s\n" % (a, s, b, s, f))
    return b"".join(out)
