"""GPU: per-window change emission against an independent reference, at its edges
(include/gs_summary.h, gs_set_change_tracking / gs_take_changes_device / gs_take_changes;
csrc/gs_changes.cpp, csrc/gs_changes_k.hip and the list-restoring branch of gs_reset).

test_gpu_changes.py checks the (vertex, label) rows of the CC kind on the walk path. Here:
the parity column of all four emitting kernels, the walk/scan threshold on both sides,
the whole-table take after a rebuild and the exact take after it, gs_reset over the
vertex list with spliced member lists, rows that reach a tracked summary through
combine / deserialize / fold_parity / fold_text, extreme ids, and the capacity contracts.

The reference is never the code under test: oracle.cc_labels for labels, oracle.bip_truth
for the parity of plain-edge streams (parity = 1 - sign, as tests/test_gpu_partitioned.py
has it), and _ref_weighted below (a BFS) for streams that carry an explicit w."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1


# ---------------------------------------------------------------- references
def _ref_plain(oracle_mod, s, d, signed):
    """{v: label} (CC) or {v: (label, parity)} (signed) of a stream of plain edges."""
    s = np.asarray(s, np.int64)
    d = np.asarray(d, np.int64)
    v, lab = oracle_mod.cc_labels(s, d)
    labels = dict(zip(v.tolist(), lab.tolist()))
    if not signed:
        return labels
    ok, comp, tv, sign = oracle_mod.bip_truth(s, d)
    assert ok, "only bipartite prefixes are in scope"
    out = {a: (c, 1 - g) for a, c, g in zip(tv.tolist(), comp.tolist(), sign.tolist())}
    assert {a: x[0] for a, x in out.items()} == labels, "the two oracles disagree on labels"
    return out


def _ref_weighted(s, d, w, signed=True):
    """Plain reference for edges with a required parity w (1: different sides, 0: same
    side): BFS per component; label = the component's minimum id, parity(v) =
    colour(v) XOR colour(that minimum). At most 4096 edges."""
    assert len(s) <= 4096
    adj = {}
    for a, b, p in zip(np.asarray(s).tolist(), np.asarray(d).tolist(), np.asarray(w).tolist()):
        adj.setdefault(a, []).append((b, p))
        adj.setdefault(b, []).append((a, p))
    out = {}
    for start in adj:
        if start in out:
            continue
        colour = {start: 0}
        order = [start]
        for u in order:  # (grows while it is walked: breadth first)
            for x, p in adj[u]:
                c = colour[u] ^ p
                if x not in colour:
                    colour[x] = c
                    order.append(x)
                else:
                    assert colour[x] == c, "the reference stream is not bipartite"
        m = min(order)
        for u in order:
            out[u] = (m, colour[u] ^ colour[m]) if signed else m
    return out


def _label(x):
    return x[0] if isinstance(x, tuple) else x


# ---------------------------------------------------------------- takes
def _rows(v, lab, par):
    v = np.asarray(v).tolist()
    assert len(set(v)) == len(v), "a vertex emitted twice in one take"
    if par is None:
        return dict(zip(v, np.asarray(lab).tolist()))
    return dict(zip(v, zip(np.asarray(lab).tolist(), np.asarray(par).tolist())))


def _take(x, signed, how="device", cap=None):
    """One take as {v: label} or {v: (label, parity)}. how = "device":
    gs_take_changes_device into arrays of `cap` rows (default num_vertices() + 1) with a
    uint8 parity tensor for the signed kind, prefilled with 0xFF so that a row whose
    parity was not written cannot pass; "host": gs_take_changes."""
    if how == "host":
        out = x.take_changes_host(with_parity=signed)
        return _rows(out[0], out[1], out[2] if signed else None)
    import torch
    m = x.num_vertices() + 1 if cap is None else cap
    dev = torch.device("cuda", x.device)
    v = torch.empty(m, dtype=torch.int64, device=dev)
    lab = torch.empty(m, dtype=torch.int64, device=dev)
    par = torch.full((m,), 0xFF, dtype=torch.uint8, device=dev) if signed else None
    k = x.take_changes_device(v, lab, par)
    assert k <= m
    return _rows(v[:k].cpu().numpy(), lab[:k].cpu().numpy(), par[:k].cpu().numpy() if signed else None)


class _Sink:
    """A keyed sink and the checks of one take against the reference state `after`.

    The expected row set of a take is {v : v new, or label(v) changed} since the previous
    take. Labels are component minima, so a vertex's parity relative to its label changes
    only when its label changes: the row set of the signed kind is the same as the CC
    one, and it is computed from the labels alone. Every emitted row must equal the
    reference (label and, for the signed kind, parity), and the sink that applies the
    rows must equal the reference state.
    mode "exact": rows == changed set; "superset": changed set <= rows (the scan path's
    idempotent rows); "all": rows == every vertex (a whole-table take)."""

    def __init__(self):
        self.state = {}
        self.before = {}

    def clear(self):  # what gs_reset means for a sink: the summary is empty again
        self.state = {}
        self.before = {}

    def check(self, rows, after, mode="exact"):
        wrong = {k: (val, after.get(k)) for k, val in rows.items() if after.get(k) != val}
        assert not wrong, "rows that differ from the reference (emitted, expected): %r" % dict(list(wrong.items())[:8])
        changed = {k for k, val in after.items() if _label(self.before.get(k)) != _label(val)}
        if mode == "all":
            assert set(rows) == set(after), "a whole-table take emits every vertex once"
        else:
            assert changed <= set(rows), "a changed vertex was not emitted"
            if mode == "exact":
                assert set(rows) == changed, "unchanged vertices emitted"
        self.state.update(rows)
        assert self.state == after
        self.before = dict(after)
        return changed


def _windows(n, window):
    b = list(range(0, n, window)) + [n]
    return list(zip(b[:-1], b[1:]))


def _run_plain(gs, oracle_mod, kind, s, d, window, hint, mode="exact", how="device", setup=None, fold=None):
    """Plain edges window by window; the mode of a take after a window whose fold grew
    the table is "all" (the header: the first take after a rebuild emits every vertex)."""
    signed = kind == "signed"
    sink = _Sink()
    grown = kept = 0
    with gs.Summary(kind, capacity_hint=hint) as x:
        x.set_change_tracking(True)
        if setup:
            setup(x)
        for lo, hi in _windows(len(s), window):
            cap = x.table_capacity()
            (fold or (lambda y, a, b: y.fold(a, b)))(x, s[lo:hi], d[lo:hi])
            grew = x.table_capacity() != cap
            grown += grew
            kept += not grew
            sink.check(_take(x, signed, how), _ref_plain(oracle_mod, s[:hi], d[:hi], signed), "all" if grew else mode)
    return grown, kept


def _stream_a(oracle_mod):
    return oracle_mod.bip_edges(0x5EED0B1B, 11, 0, 1 << 14)


# ---------------------------------------------------------------- 1. signed kind, exact, with parity
@pytest.mark.parametrize("how", ["device", "host"])
def test_signed_rows_exact_with_parity(gs, oracle_mod, how):
    """k_emit_records (parity_to_root) and k_emit_new: every window's rows are exactly the
    changed set and carry the reference's label and parity; device and host takes each
    against the reference."""
    s, d = _stream_a(oracle_mod)
    grown, kept = _run_plain(gs, oracle_mod, "signed", s, d, 1 << 11, 1 << 14, how=how)
    assert grown == 0 and kept == 8  # hint 2^14: no rebuild, every take is on the walk path


@pytest.mark.parametrize("how", ["device", "host"])
def test_signed_merge_flips_a_component_by_value(gs, oracle_mod, how):
    """12 edges, negative ids, windows of 4. Window 2 hooks {10..13} under -5 through an
    edge that flips every parity of the component relative to its new minimum; window 3
    hooks {20,21,22} under -9 without a flip and {-5,-4,10..13} under -9 with one."""
    s = np.array([10, 11, 12, -5, -4, 20, 21, -9, -8, -9, 30, 31], np.int64)
    d = np.array([11, 12, 13, -4, 11, 21, 22, -8, 20, 13, 31, -9], np.int64)
    by_value = [
        {10: (10, 0), 11: (10, 1), 12: (10, 0), 13: (10, 1), -5: (-5, 0), -4: (-5, 1)},
        {10: (-5, 1), 11: (-5, 0), 12: (-5, 1), 13: (-5, 0), 20: (20, 0), 21: (20, 1), 22: (20, 0), -9: (-9, 0),
         -8: (-9, 1)},
        {-5: (-9, 1), -4: (-9, 0), 10: (-9, 0), 11: (-9, 1), 12: (-9, 0), 13: (-9, 1), 20: (-9, 0), 21: (-9, 1),
         22: (-9, 0), 30: (-9, 0), 31: (-9, 1)},
    ]
    sink = _Sink()
    with gs.Summary("signed", capacity_hint=64) as x:
        x.set_change_tracking(True)
        for wi, (lo, hi) in enumerate(_windows(12, 4)):
            x.fold(s[lo:hi], d[lo:hi])
            rows = _take(x, True, how)
            assert rows == by_value[wi]
            sink.check(rows, _ref_plain(oracle_mod, s[:hi], d[:hi], True))
        assert x.ok()


# ---------------------------------------------------------------- 2. parity on the scan and whole-table paths
def test_signed_parity_on_the_scan_path(gs, oracle_mod, knobs):
    """k_emit_scan (acc of find_ro): walk limit 8, so larger relabelled components go
    through the scan: a superset, no vertex twice, every row's parity the reference's."""
    knobs(changes_walk_max=8)
    s, d = _stream_a(oracle_mod)
    grown, _ = _run_plain(gs, oracle_mod, "signed", s, d, 1 << 11, 1 << 14, mode="superset")
    assert grown == 0


def test_signed_parity_on_the_whole_table_path(gs, oracle_mod):
    """Hint 16: the table is rebuilt during the stream and those takes emit the whole
    table (k_emit_scan with all = 1), parity included."""
    s, d = _stream_a(oracle_mod)
    grown, _ = _run_plain(gs, oracle_mod, "signed", s, d, 1 << 11, 16)
    assert grown >= 1


# ---------------------------------------------------------------- 3. the walk limit, both sides
K_ABSORB = 100
PATH_BASE = 10 ** 6


def _walk_limit_case(gs, oracle_mod, kind, m):
    """An absorbing component of 100 vertices (minimum id 0) and a path of m vertices from
    10^6 upwards, then the one edge that joins them: the path's root is hooked under 0 and
    its member list has exactly m entries. Returns the rows of the joining window."""
    signed = kind == "signed"
    s0 = np.concatenate([np.arange(K_ABSORB - 1), PATH_BASE + np.arange(m - 1)]).astype(np.int64)
    d0 = s0 + 1
    s1 = np.concatenate([s0, [K_ABSORB - 1]]).astype(np.int64)
    d1 = np.concatenate([d0, [PATH_BASE]]).astype(np.int64)
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=max(1 << 10, 2 * m)) as x:
        x.set_change_tracking(True)
        x.fold(s0, d0)
        sink.check(_take(x, signed), _ref_plain(oracle_mod, s0, d0, signed))
        cap = x.table_capacity()
        x.fold(s1[-1:], d1[-1:])
        assert x.table_capacity() == cap  # (a rebuild would make this a whole-table take)
        rows = _take(x, signed)
        after = _ref_plain(oracle_mod, s1, d1, signed)
        assert all(_label(val) == 0 for val in after.values())
        return rows, after, sink


@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_walk_limit_knob_both_sides(gs, oracle_mod, knobs, kind):
    """changes_walk_max = 8: a list of 8 is walked (exactly the 8 relabelled rows), a list
    of 9 goes to the scan (the 9 and the absorbing component's 100, each once)."""
    knobs(changes_walk_max=8)
    rows, after, sink = _walk_limit_case(gs, oracle_mod, kind, 8)
    assert len(rows) == 8
    sink.check(rows, after, "exact")
    rows, after, sink = _walk_limit_case(gs, oracle_mod, kind, 9)
    assert len(rows) == 9 + K_ABSORB
    sink.check(rows, after, "all")


@pytest.mark.parametrize("m", [1 << 16, (1 << 16) + 1])
def test_walk_limit_of_the_product_both_sides(gs, oracle_mod, m):
    """The product's limit of 2^16 (no knob): a list of 65536 is walked, one of 65537 is
    scanned."""
    rows, after, sink = _walk_limit_case(gs, oracle_mod, "cc", m)
    if m == 1 << 16:
        assert len(rows) == m
        sink.check(rows, after, "exact")
    else:
        assert len(rows) == m + K_ABSORB
        sink.check(rows, after, "all")


# ---------------------------------------------------------------- 4. rebuild, then exact again
def test_rebuild_take_is_the_whole_table_then_exact_again(gs, oracle_mod):
    """The take after a window whose fold grew the table has exactly num_vertices() rows,
    every vertex once with the oracle's label; the takes after windows without growth are
    exact again on the fresh lists (k_iota, k_relist, k_emit_new with emit = 0)."""
    s, d = oracle_mod.er_edges(0x5EED00E5, 14, 0, 1 << 15, True)
    sink = _Sink()
    kinds = []
    with gs.Summary("cc", capacity_hint=16) as x:
        x.set_change_tracking(True)
        for lo, hi in _windows(len(s), 1 << 12):
            cap = x.table_capacity()
            x.fold(s[lo:hi], d[lo:hi])
            grew = x.table_capacity() != cap
            kinds.append(grew)
            rows = _take(x, False)
            if grew:
                assert len(rows) == x.num_vertices()
            sink.check(rows, _ref_plain(oracle_mod, s[:hi], d[:hi], False), "all" if grew else "exact")
    assert any(kinds) and not all(kinds), kinds
    assert not kinds[-1] and True in kinds[:-1]  # an exact take after a whole-table one


# ---------------------------------------------------------------- 5. reset over the vertex list
def _grouping(cycle, nv=600, groups=40):
    """600 ids in 40 path components (a different grouping per cycle), then the edges
    that hook the components pairwise."""
    ids = (np.arange(nv, dtype=np.int64) * 7919 + 13)
    ids = np.random.RandomState(100 + cycle).permutation(ids).reshape(groups, nv // groups)
    s = ids[:, :-1].ravel()
    d = ids[:, 1:].ravel()
    hs = ids[0::2, -1]
    hd = ids[1::2, 0]
    return s, d, hs, hd


def _reset_cycles(gs, oracle_mod, kind, hint, sparse, toggle=False):
    signed = kind == "signed"
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=hint) as x:
        x.set_change_tracking(True)
        cap0 = x.table_capacity()
        for cycle in range(4):
            if cycle:
                x.reset()
                sink.clear()
            s, d, hs, hd = _grouping(cycle)
            cap = x.table_capacity()
            x.fold(s, d)
            grew = x.table_capacity() != cap
            sink.check(_take(x, signed), _ref_plain(oracle_mod, s, d, signed), "all" if grew else "exact")
            if toggle and cycle in (1, 2):
                # off and on again over a non-empty table: lists of the current forest
                # (k_relist) and the first take emits every vertex once
                x.set_change_tracking(False)
                x.set_change_tracking(True)
                rows = _take(x, signed)
                assert len(rows) == x.num_vertices() == 600
                sink.check(rows, _ref_plain(oracle_mod, s, d, signed), "all")
            s2 = np.concatenate([s, hs])
            d2 = np.concatenate([d, hd])
            cap = x.table_capacity()
            x.fold(hs, hd)
            grew = x.table_capacity() != cap
            sink.check(_take(x, signed), _ref_plain(oracle_mod, s2, d2, signed), "all" if grew else "exact")
        if sparse:  # 600 vertices in >= 2^16 slots: every reset went by the vertex list
            assert x.table_capacity() == cap0 >= 1 << 16


@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_reset_by_the_vertex_list_restores_the_member_lists(gs, oracle_mod, kind):
    """A sparse table (reset restores only the listed slots and their nxt entries): lists
    spliced before the reset must not leak into the walks after it. Four takes around
    each of three resets, all exact."""
    _reset_cycles(gs, oracle_mod, kind, 1 << 16, sparse=True)


def test_reset_of_a_dense_table_restores_the_member_lists(gs, oracle_mod):
    """The same cycles over a table too dense for the listed reset (the full-init branch)."""
    _reset_cycles(gs, oracle_mod, "cc", 256, sparse=False)


def test_reset_cycles_with_tracking_switched_off_and_on(gs, oracle_mod):
    _reset_cycles(gs, oracle_mod, "cc", 1 << 16, sparse=True, toggle=True)


# ---------------------------------------------------------------- 6. other doors into a tracked summary
def _path(ids):
    ids = np.asarray(ids, np.int64)
    return ids[:-1], ids[1:]


def _cat(*parts):
    return np.concatenate([np.asarray(p, np.int64) for p in parts])


@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_door_combine_bridges_two_components(gs, oracle_mod, kind):
    signed = kind == "signed"
    ts, td = (_cat(a, b, c) for a, b, c in zip(*[_path(range(0, 10)), _path(range(100, 110)), _path(range(200, 205))]))
    os_, od = np.array([9, 100, 400], np.int64), np.array([100, 300, 401], np.int64)
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=256) as x, gs.Summary(kind, capacity_hint=256) as other:
        x.set_change_tracking(True)
        x.fold(ts, td)
        sink.check(_take(x, signed), _ref_plain(oracle_mod, ts, td, signed))
        other.fold(os_, od)
        x.combine(other)
        rows = _take(x, signed)
        changed = sink.check(rows, _ref_plain(oracle_mod, _cat(ts, os_), _cat(td, od), signed))
        assert changed == set(range(100, 110)) | {300, 400, 401}
        x.fold([204], [401])  # the lists after the combined rows: {400, 401} is walked
        rows = _take(x, signed)
        sink.check(rows, _ref_plain(oracle_mod, _cat(ts, os_, [204]), _cat(td, od, [401]), signed))
        assert set(rows) == {400, 401}


def _consistent_weighted(seed, nv, ne, lo=0):
    """Random edges over nv ids with w = colour(a) XOR colour(b) of a hidden colouring:
    mixed w, cycles, always bipartite in the signed sense."""
    r = np.random.RandomState(seed)
    ids = lo + r.permutation(4 * nv)[:nv].astype(np.int64) * 3 - nv
    colour = r.randint(0, 2, nv)
    a = r.randint(0, nv, ne)
    b = (a + 1 + r.randint(0, nv - 1, ne)) % nv  # no self-loops
    return ids[a], ids[b], (colour[a] ^ colour[b]).astype(np.uint8)


def test_door_combine_exported_device_signed(gs, oracle_mod):
    """Rows (v, label, parity) exported from another signed summary whose parities are
    not all 1, folded into a tracked one that overlaps it."""
    import torch
    s, d, w = _consistent_weighted(11, 300, 900)
    ts, td, tw = s[:400], d[:400], w[:400]
    os_, od, ow = s[400:], d[400:], w[400:]
    sink = _Sink()
    with gs.Summary("signed", capacity_hint=2048) as x, gs.Summary("signed", capacity_hint=2048) as other:
        x.set_change_tracking(True)
        x.fold_parity(ts, td, tw)
        sink.check(_take(x, True), _ref_weighted(ts, td, tw))
        other.fold_parity(os_, od, ow)
        m = other.num_vertices()
        dev = torch.device("cuda", other.device)
        ev = torch.empty(m, dtype=torch.int64, device=dev)
        el = torch.empty(m, dtype=torch.int64, device=dev)
        ep = torch.empty(m, dtype=torch.uint8, device=dev)
        assert other.export_labels_device(ev, el, ep) == m
        other.sync()
        x.combine_exported_device(ev, el, ep, m)
        changed = sink.check(_take(x, True), _ref_weighted(s, d, w))
        assert changed, "the exported rows change nothing: the stream is too small"
        assert x.ok()


@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_door_deserialize_on_a_tracked_handle(gs, oracle_mod, kind):
    """gs_deserialize is a reset plus a fold of the image's rows. A reset empties the
    summary, so a sink empties with it (that is what gs_reset means); the take after the
    deserialize then brings a sink cleared at that moment to exactly the image's labels."""
    signed = kind == "signed"
    s, d = oracle_mod.bip_edges(0x5EED0B1C, 8, 0, 1 << 10)
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=4096) as src, gs.Summary(kind, capacity_hint=4096) as x:
        src.fold(s, d)
        image = src.serialize()
        x.set_change_tracking(True)
        x.fold(s[:300] + 5000, d[:300] + 5000)  # other vertices, with spliced lists
        sink.check(_take(x, signed), _ref_plain(oracle_mod, s[:300] + 5000, d[:300] + 5000, signed))
        x.fold(s[300:600] + 5000, d[300:600] + 5000)  # pending changes die with the reset
        x.deserialize(image)
        sink.clear()
        sink.check(_take(x, signed), _ref_plain(oracle_mod, s, d, signed), "all")
        s2, d2 = oracle_mod.bip_edges(0x5EED0B1C, 8, 1 << 10, 1 << 9)
        x.fold(s2, d2)
        sink.check(_take(x, signed), _ref_plain(oracle_mod, _cat(s, s2), _cat(d, d2), signed))


def test_door_fold_parity_mixed_w(gs, oracle_mod):
    s, d, w = _consistent_weighted(12, 300, 800)
    sink = _Sink()
    with gs.Summary("signed", capacity_hint=2048) as x:
        x.set_change_tracking(True)
        for lo, hi in _windows(len(s), 100):
            x.fold_parity(s[lo:hi], d[lo:hi], w[lo:hi])
            sink.check(_take(x, True), _ref_weighted(s[:hi], d[:hi], w[:hi]))
        assert x.ok() and 0 < int(w.sum()) < len(w)


@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_door_fold_text(gs, oracle_mod, kind):
    signed = kind == "signed"
    s, d = oracle_mod.bip_edges(0x5EED0B1D, 9, 0, 2500)
    text = bytes(oracle_mod.format_edges(s[500:], d[500:]))
    assert text.count(b"\n") == 2000
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=4096) as x:
        x.set_change_tracking(True)
        x.fold(s[:500], d[:500])
        sink.check(_take(x, signed), _ref_plain(oracle_mod, s[:500], d[:500], signed))
        assert x.fold_text(text) == 2000
        sink.check(_take(x, signed), _ref_plain(oracle_mod, s, d, signed))


def test_tracked_folds_with_pipelining(gs, oracle_mod):
    """set_pipelining(3) is overridden by a tracked fold (it takes the handle stream)."""
    import torch
    s, d = _stream_a(oracle_mod)

    def fold(x, a, b):  # several device folds per window, as a pipelined caller issues them
        ta, tb = torch.from_numpy(a).cuda(x.device), torch.from_numpy(b).cuda(x.device)
        torch.cuda.synchronize(x.device)
        for lo, hi in _windows(len(a), 512):
            x.fold_device(ta[lo:hi], tb[lo:hi])
        x.sync()  # (ta, tb are read until the folds are done)

    _run_plain(gs, oracle_mod, "cc", s, d, 1 << 11, 1 << 14, setup=lambda x: x.set_pipelining(3), fold=fold)


def test_tracked_folds_with_the_window_server_on(gs, oracle_mod):
    s, d = oracle_mod.bip_edges(0x5EED0B1E, 9, 0, 1 << 12)
    _run_plain(gs, oracle_mod, "signed", s, d, 256, 1 << 12, setup=lambda x: x.set_window_server(True))


def test_tracked_folds_with_batch_dedup(gs, oracle_mod):
    """Every edge ten times in its window: the dedup pre-pass drops the repeats and the
    rows are those of the plain stream."""
    s, d = oracle_mod.bip_edges(0x5EED0B1F, 9, 0, 1 << 11)
    s10 = np.tile(s.reshape(-1, 256), 10).ravel()  # windows of 2560 = 10 x the same 256 edges
    d10 = np.tile(d.reshape(-1, 256), 10).ravel()
    assert np.array_equal(s10[:256], s10[256:512]) and np.array_equal(s10[2560:2816], s[256:512])
    _run_plain(gs, oracle_mod, "signed", s10, d10, 2560, 1 << 12, setup=lambda x: x.set_batch_dedup(True))


# ---------------------------------------------------------------- 7. ids and shapes
_EXTREME = [  # windows of (src, dst)
    ([5, 1 << 40, 5, 9, 10, -7], [1 << 40, I64_MAX, 9, 10, 11, -3]),
    ([-3, 20, 100], [20, 21, 101]),
    ([I64_MIN, -7], [11, 100]),  # INT64_MIN joins the largest component: all of it relabels
    ([-7], [I64_MAX]),           # and then absorbs a second one while it is an old root
    ([I64_MIN, 77], [1 << 40, 21]),  # (an odd distance apart: still bipartite)
]


@pytest.mark.parametrize("kind", ["cc", "signed"])
@pytest.mark.parametrize("route", ["walk", "scan", "table"])
def test_extreme_ids_on_every_route(gs, oracle_mod, knobs, kind, route):
    """INT64_MIN (the reserved slot r0, always a final root), INT64_MAX, negatives and
    2^40. walk: exact rows. scan (walk limit 2): the rows of a window are every old vertex
    under a flagged root plus the new ones -- computed here from the reference, so a
    scan that loses INT64_MIN's own row is seen. table: tracking enabled after the first
    window, and switched off and on again after the third, so two takes are whole-table
    ones, the second with INT64_MIN present."""
    signed = kind == "signed"
    if route == "scan":
        knobs(changes_walk_max=2)
    sink = _Sink()
    s = np.empty(0, np.int64)
    d = np.empty(0, np.int64)
    with gs.Summary(kind, capacity_hint=256) as x:
        if route != "table":
            x.set_change_tracking(True)
        for wi, (ws, wd) in enumerate(_EXTREME):
            x.fold(np.array(ws, np.int64), np.array(wd, np.int64))
            s, d = _cat(s, ws), _cat(d, wd)
            after = _ref_plain(oracle_mod, s, d, signed)
            mode = "exact"
            if route == "table" and wi in (0, 3):
                if wi == 3:
                    x.set_change_tracking(False)
                x.set_change_tracking(True)
                mode = "all"
            before = dict(sink.before)
            rows = _take(x, signed)
            if route == "scan":
                # old components (>= 1 old vertex) whose label changed, by their size before
                sizes = {}
                for val in before.values():
                    sizes[_label(val)] = sizes.get(_label(val), 0) + 1
                big = {_label(after[k]) for k, val in before.items()
                       if _label(after[k]) != _label(val) and sizes[_label(val)] > 2}
                expect = {k for k, val in after.items()
                          if k not in before or _label(before[k]) != _label(val) or _label(val) in big}
                assert set(rows) == expect
                mode = "superset"
            sink.check(rows, after, mode)
        assert x.find(I64_MAX) == I64_MIN and x.find(1 << 40) == I64_MIN


def test_self_loops(gs, oracle_mod):
    """The records kernel skips a == b; a vertex seen only through a self-loop is new
    (k_emit_new), one on an existing vertex changes nothing."""
    wins = [([1, 7], [2, 7]), ([2], [2]), ([9], [9]), ([7, 9], [9, 9]), ([3, 3], [3, 1])]
    expect = [{1: 1, 2: 1, 7: 7}, {}, {9: 9}, {9: 7}, {3: 1}]
    sink = _Sink()
    s = np.empty(0, np.int64)
    d = np.empty(0, np.int64)
    with gs.Summary("cc", capacity_hint=64) as x:
        x.set_change_tracking(True)
        for (ws, wd), want in zip(wins, expect):
            x.fold(ws, wd)
            s, d = _cat(s, ws), _cat(d, wd)
            rows = _take(x, False)
            assert rows == want
            sink.check(rows, _ref_plain(oracle_mod, s, d, False))


@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_hook_chain_through_a_new_vertex(gs, oracle_mod, kind):
    """X = 50 (old root of {50, 51, 52}) under F = 30 (new in this window) under L = 1
    (old root of {1, 2}), both edges in one window: the `fresh` branch skips F's walk and
    still splices, and X's members are emitted with L's key."""
    signed = kind == "signed"
    s = np.array([50, 51, 1, 50, 30], np.int64)
    d = np.array([51, 52, 2, 30, 1], np.int64)
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=64) as x:
        x.set_change_tracking(True)
        x.fold(s[:3], d[:3])
        sink.check(_take(x, signed), _ref_plain(oracle_mod, s[:3], d[:3], signed))
        x.fold(s[3:], d[3:])
        rows = _take(x, signed)
        want = {50: (1, 0), 51: (1, 1), 52: (1, 0), 30: (1, 1)}
        assert rows == (want if signed else {k: val[0] for k, val in want.items()})
        sink.check(rows, _ref_plain(oracle_mod, s, d, signed))
        x.fold([52], [60])  # the spliced list of 1 is intact: only the new vertex
        assert _take(x, signed) == ({60: (1, 1)} if signed else {60: 1})


@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_takes_without_changes_are_empty(gs, oracle_mod, kind):
    signed = kind == "signed"
    s, d = oracle_mod.bip_edges(0x5EED0B20, 7, 0, 1 << 10)
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=1 << 14) as x:
        x.set_change_tracking(True)
        assert _take(x, signed) == {}  # nothing folded yet
        x.fold(s, d)
        cap = x.table_capacity()
        after = _ref_plain(oracle_mod, s, d, signed)
        sink.check(_take(x, signed), after)
        assert _take(x, signed) == {}  # two takes with no fold between them
        assert _take(x, signed, "host") == {}
        x.fold(s[::-1].copy(), d[::-1].copy())  # only edges that are already connected
        assert _take(x, signed) == {}
        x.fold(d[:64], s[:64])
        assert _take(x, signed, "host") == {}
        assert x.table_capacity() == cap  # (a rebuild would make a take the whole table)
        v, lab = x.labels()
        assert dict(zip(v.tolist(), lab.tolist())) == {k: _label(val) for k, val in after.items()}


# ---------------------------------------------------------------- 8. capacity contracts
@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_take_capacity_below_the_vertex_count_loses_nothing(gs, oracle_mod, kind):
    """cap == num_vertices() - 1 is refused with GS_ERR_INVALID before any side effect:
    the next take, with exactly num_vertices() rows, delivers the window's complete and
    exact change set."""
    signed = kind == "signed"
    s, d = oracle_mod.bip_edges(0x5EED0B21, 8, 0, 1 << 10)
    sink = _Sink()
    with gs.Summary(kind, capacity_hint=2048) as x:
        x.set_change_tracking(True)
        x.fold(s[:512], d[:512])
        nv = x.num_vertices()
        sink.check(_take(x, signed, cap=nv), _ref_plain(oracle_mod, s[:512], d[:512], signed))
        x.fold(s[512:], d[512:])
        nv = x.num_vertices()
        for _ in range(2):
            with pytest.raises(gs.GSError) as e:
                _take(x, signed, cap=nv - 1)
            assert e.value.code == gs.GS_ERR_INVALID
        changed = sink.check(_take(x, signed, cap=nv), _ref_plain(oracle_mod, s, d, signed))
        assert 0 < len(changed) < nv  # hooks and new vertices, and not simply everything


def test_delta_capacity_refuses_a_fold_before_any_effect(gs, oracle_mod):
    """Tracked folds between two takes are bounded by the delta list (gs_delta_capacity
    rows; the refusal names the edge bound). Folds of 2^20 edges are accepted up to the
    bound; the fold that would exceed it fails with GS_ERR_CAPACITY and leaves no trace;
    after a take it is accepted."""
    import re
    n = 1 << 20
    s, d = oracle_mod.er_edges(0x5EED00E6, 12, 0, n, True)
    s2, d2 = oracle_mod.er_edges(0x5EED00E7, 12, 0, n, True)
    s2, d2 = s2 ^ (1 << 50), d2 ^ (1 << 50)  # other vertices: an effect of the refused fold would show
    with gs.Summary("cc", capacity_hint=1 << 14) as probe:  # how many 2^20-edge folds fit between two takes
        probe.set_change_tracking(True)
        rows_cap = probe.delta_capacity()
        fit = 0
        err = None
        while err is None and fit * n <= rows_cap:
            try:
                probe.fold(s, d)
                fit += 1
            except gs.GSError as e:
                err = e
        assert err is not None and err.code == gs.GS_ERR_CAPACITY, "no refusal within delta_capacity() edges"
        bound = int(re.search(r"at most (\d+) folded edges", str(err)).group(1))
        assert n <= bound <= rows_cap           # at most one record per folded edge
        assert fit * n <= bound < (fit + 1) * n  # refused only because it would pass the bound
    sink = _Sink()
    with gs.Summary("cc", capacity_hint=1 << 14) as x:
        x.set_change_tracking(True)
        for i in range(fit):
            if i == fit - 1:
                # one call of 2^21 edges (two staging chunks, the first of which alone
                # would fit) is refused as a whole: no vertex of its first chunk arrives
                nv = x.num_vertices()
                with pytest.raises(gs.GSError) as e:
                    x.fold(_cat(s2, s), _cat(d2, d))
                assert e.value.code == gs.GS_ERR_CAPACITY
                assert x.num_vertices() == nv
            x.fold(s, d)
        with pytest.raises(gs.GSError) as e:
            x.fold(s2, d2)
        assert e.value.code == gs.GS_ERR_CAPACITY
        after = _ref_plain(oracle_mod, s, d, False)
        assert x.num_vertices() == len(after)
        sink.check(_take(x, False), after)
        assert _take(x, False) == {}
        x.fold(s2, d2)  # the refused fold, after the take
        final = _ref_plain(oracle_mod, _cat(s, s2), _cat(d, d2), False)
        changed = sink.check(_take(x, False), final)
        assert changed == set(final) - set(after)
        v, lab = x.labels()
        assert dict(zip(v.tolist(), lab.tolist())) == final
