"""GPU: the grouped component export (gs_num_components, gs_export_components_device,
gs_export_components) against the oracle -- the authority -- and against the parent path
(labels() / colouring() followed by np.lexsort). Every output is an integer: comparisons
are exact."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
SENTINEL = -0x5A5A5A5A5A5A5A5B


def _pins():
    with open(os.path.join(GOLD, "reference_pins.json")) as f:
        return json.load(f)


def _expand(comp, offset):
    return np.repeat(comp, np.diff(offset.astype(np.int64)))


def _device_export(s, cap_v, cap_c, with_sign=True):
    """components_device into fresh torch tensors; numpy (comp, offset, member, sign)."""
    import torch
    dev = torch.device("cuda", s.device)
    comp = torch.full((cap_c,), SENTINEL, dtype=torch.int64, device=dev)
    offset = torch.full((cap_c + 1,), SENTINEL, dtype=torch.int64, device=dev)
    member = torch.full((cap_v,), SENTINEL, dtype=torch.int64, device=dev)
    sign = torch.full((cap_v,), 0xA5, dtype=torch.uint8, device=dev) if with_sign else None
    nv, nc = s.components_device(comp, offset, member, sign)
    return (comp[:nc].cpu().numpy(), offset[:nc + 1].cpu().numpy().view(np.uint64), member[:nv].cpu().numpy(),
            sign[:nv].cpu().numpy() if with_sign else None)


def _check_structure(comp, offset, member):
    assert len(offset) == len(comp) + 1
    assert int(offset[0]) == 0 and int(offset[-1]) == len(member)
    assert np.all(np.diff(offset.astype(np.int64)) > 0), "an empty component"
    assert np.all(comp[1:] > comp[:-1]), "comp is not strictly ascending in signed order"
    if len(comp):
        assert np.array_equal(member[offset[:-1].astype(np.int64)], comp), "a component does not start at its minimum"


def _check_cc(s, oracle_mod, src, dst):
    """Host and device forms of a 'cc' summary equal the oracle and the parent path."""
    ov, olab = oracle_mod.cc_labels(src, dst)
    o = np.lexsort((ov, olab))
    ok, comp, offset, member, sign = s.components()
    assert ok
    _check_structure(comp, offset, member)
    assert np.array_equal(member, ov[o]), "members differ from the oracle"
    assert np.array_equal(_expand(comp, offset), olab[o]), "labels differ from the oracle"
    assert not sign.any()  # no colouring in a DisjointSet
    pv, pl = s.labels()  # the parent path: unordered rows sorted on the host
    po = np.lexsort((pv, pl))
    assert np.array_equal(member, pv[po]) and np.array_equal(_expand(comp, offset), pl[po])
    assert s.num_components() == len(comp) == len(np.unique(olab))
    dcomp, doffset, dmember, dsign = _device_export(s, len(member), len(comp))
    assert np.array_equal(dcomp, comp) and np.array_equal(doffset, offset)
    assert np.array_equal(dmember, member) and np.array_equal(dsign, sign)
    return comp, offset, member


def _check_signed(s, oracle_mod, src, dst):
    ook, ocomp, ov, osign = oracle_mod.bip_truth(src, dst)  # sorted by (comp, v)
    assert ook
    ok, comp, offset, member, sign = s.components()
    assert ok
    _check_structure(comp, offset, member)
    assert np.array_equal(member, ov) and np.array_equal(_expand(comp, offset), ocomp)
    assert np.array_equal(sign, osign), "signs differ from the oracle at %d vertices" % int((sign != osign).sum())
    pok, pcomp, pv, psign = s.colouring()  # the parent path
    assert pok and np.array_equal(member, pv) and np.array_equal(_expand(comp, offset), pcomp)
    assert np.array_equal(sign, psign)
    assert s.num_components() == len(comp)
    dcomp, doffset, dmember, dsign = _device_export(s, len(member), len(comp))
    assert np.array_equal(dcomp, comp) and np.array_equal(doffset, offset)
    assert np.array_equal(dmember, member) and np.array_equal(dsign, sign)
    return comp, offset, member, sign


def _csr_cc_string(comp, offset, member):
    return "{" + ", ".join("%d=[%s]" % (c, ", ".join(str(x) for x in member[int(a):int(b)].tolist()))
                           for c, a, b in zip(comp.tolist(), offset[:-1].tolist(), offset[1:].tolist())) + "}"


def _csr_candidates_string(ok, comp, offset, member, sign):
    if not ok:
        return "(false,{})"
    parts = []
    for c, a, b in zip(comp.tolist(), offset[:-1].tolist(), offset[1:].tolist()):
        inner = ", ".join("%d=(%d,%s)" % (x, x, "true" if g else "false")
                          for x, g in zip(member[int(a):int(b)].tolist(), sign[int(a):int(b)].tolist()))
        parts.append("%d={%s}" % (c, inner))
    return "(true,{" + ", ".join(parts) + "})"


# ------------------------------------------------------------- case 1: reference pins
def test_pin_connected_components(gs, oracle_mod):
    p = _pins()["cc_test"]
    s, d = map(np.array, zip(*p["edges"]))
    with gs.Summary("cc", capacity_hint=16) as ds:
        ds.fold(s, d)
        comp, offset, member = _check_cc(ds, oracle_mod, s, d)
        assert comp.tolist() == [1, 6, 8]
        assert offset.tolist() == [0, 4, 6, 8]
        assert member.tolist() == [1, 2, 3, 5, 6, 7, 8, 9]
        text = _csr_cc_string(comp, offset, member)
        assert text == oracle_mod.canonical_cc_string(*ds.labels())
        assert oracle_mod.cc_test_parser([text]) == p["expected_lines"]


def test_pin_bipartite(gs, oracle_mod):
    p = _pins()["bip_test_bipartite"]
    s, d = map(np.array, zip(*p["edges"]))
    with gs.Summary("signed", capacity_hint=16) as c:
        c.fold(s, d)
        comp, offset, member, sign = _check_signed(c, oracle_mod, s, d)
        assert _csr_candidates_string(True, comp, offset, member, sign) == p["expected"][0]


def test_pin_non_bipartite(gs):
    p = _pins()["bip_test_non_bipartite"]
    s, d = map(np.array, zip(*p["edges"]))
    with gs.Summary("signed", capacity_hint=16) as c:
        c.fold(s, d)
        ok, comp, offset, member, sign = c.components()
        assert not ok and len(comp) == 0 and len(member) == 0 and len(sign) == 0
        assert offset.tolist() == [0]
        assert c.num_components() == 0
        dcomp, doffset, dmember, _ = _device_export(c, 8, 8)
        assert len(dcomp) == 0 and len(dmember) == 0 and doffset.tolist() == [0]
        assert _csr_candidates_string(ok, comp, offset, member, sign) == p["expected"][0]


def test_pin_disjointset(gs):
    p = _pins()["disjointset_test"]
    with gs.Summary("cc", capacity_hint=16) as ds, gs.Summary("cc", capacity_hint=16) as ds2:
        s, d = map(np.array, zip(*p["setup_unions"]))
        ds.fold(s, d)
        s, d = map(np.array, zip(*p["merge_unions"]))
        ds2.fold(s, d)
        ds2.combine(ds)
        assert ds2.num_components() == p["expected_roots_after_merge"] == 2
        ok, comp, offset, member, sign = ds2.components()
        assert len(member) == p["expected_matches_after_merge"] == 18
        assert comp.tolist() == [0, 1]
        _check_structure(comp, offset, member)


# ------------------------------------------------------------- case 2: empty and truncation
@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_empty_summary(gs, kind):
    with gs.Summary(kind, capacity_hint=16) as s:
        assert s.num_components() == 0
        ok, comp, offset, member, sign = s.components()
        assert ok and len(comp) == 0 and len(member) == 0 and offset.tolist() == [0]
        dcomp, doffset, dmember, _ = _device_export(s, 4, 4)
        assert len(dcomp) == 0 and len(dmember) == 0 and doffset.tolist() == [0]


def test_truncation_leaves_the_buffers_untouched(gs):
    import torch
    L = gs.lib()
    src = np.arange(0, 300, dtype=np.int64)
    dst = src // 3 * 3  # 100 components of 3
    with gs.Summary("cc", capacity_hint=64) as s:
        s.fold(src, dst)
        nv, nc = 300, 100
        dev = torch.device("cuda", 0)
        for cap_v, cap_c in ((nv - 1, nc), (nv, nc - 1)):
            comp = torch.full((nc,), SENTINEL, dtype=torch.int64, device=dev)
            offset = torch.full((nc + 1,), SENTINEL, dtype=torch.int64, device=dev)
            member = torch.full((nv,), SENTINEL, dtype=torch.int64, device=dev)
            sign = torch.full((nv,), 0xA5, dtype=torch.uint8, device=dev)
            gv, gc = ctypes.c_size_t(0), ctypes.c_size_t(0)
            rc = L.gs_export_components_device(s.handle, comp.data_ptr(), offset.data_ptr(), member.data_ptr(),
                                               sign.data_ptr(), cap_v, cap_c, ctypes.byref(gv), ctypes.byref(gc))
            assert rc == gs.GS_ERR_TRUNCATED
            assert (gv.value, gc.value) == (nv, nc)
            torch.cuda.synchronize()
            assert bool((comp == SENTINEL).all()) and bool((offset == SENTINEL).all())
            assert bool((member == SENTINEL).all()) and bool((sign == 0xA5).all())
            # the host form
            hcomp = np.full(nc, SENTINEL, np.int64)
            hoff = np.full(nc + 1, 77, np.uint64)
            hmem = np.full(nv, SENTINEL, np.int64)
            hsign = np.full(nv, 0xA5, np.uint8)
            rc = L.gs_export_components(s.handle, hcomp.ctypes.data, hoff.ctypes.data, hmem.ctypes.data,
                                        hsign.ctypes.data, cap_v, cap_c, ctypes.byref(gv), ctypes.byref(gc))
            assert rc == gs.GS_ERR_TRUNCATED and (gv.value, gc.value) == (nv, nc)
            assert (hcomp == SENTINEL).all() and (hoff == 77).all() and (hmem == SENTINEL).all() and (hsign == 0xA5).all()
        # exact capacities succeed; null counts are rejected with a live handle too
        dcomp, doffset, dmember, _ = _device_export(s, nv, nc)
        assert dcomp.tolist() == list(range(0, 300, 3)) and dmember.tolist() == list(range(300))
        assert doffset.tolist() == list(range(0, 301, 3))
        gv = ctypes.c_size_t(0)
        assert L.gs_num_components(s.handle, None) == gs.GS_ERR_INVALID
        for fn in (L.gs_export_components_device, L.gs_export_components):
            assert fn(s.handle, None, None, None, None, 0, 0, None, ctypes.byref(gv)) == gs.GS_ERR_INVALID
            assert fn(s.handle, None, None, None, None, 0, 0, ctypes.byref(gv), None) == gs.GS_ERR_INVALID


# ------------------------------------------------------------- case 3: signed order, the reserved slot
@pytest.mark.parametrize("kind", ["cc", "signed"])
def test_signed_order_and_reserved_slot(gs, oracle_mod, kind):
    ids = [I64_MIN, I64_MIN + 1, -(1 << 40), -1, 0, 1, 1 << 40, I64_MAX - 1, I64_MAX]
    joined = [(I64_MIN, I64_MAX), (-1, 1), (0, 0)]
    loops = [(x, x) for x in ids if x not in (I64_MIN, I64_MAX, -1, 1, 0)]
    src, dst = map(lambda t: np.array(t, dtype=np.int64), zip(*(joined + loops)))
    with gs.Summary(kind, capacity_hint=16) as s:
        s.fold(src, dst)
        if kind == "cc":
            comp, offset, member = _check_cc(s, oracle_mod, src, dst)
        else:
            comp, offset, member, sign = _check_signed(s, oracle_mod, src, dst)
            assert sign[:2].tolist() == [1, 0]  # INT64_MAX is on the other side of INT64_MIN
        assert comp[0] == I64_MIN
        assert member[int(offset[0]):int(offset[1])].tolist() == [I64_MIN, I64_MAX]
        assert comp.tolist() == [I64_MIN, I64_MIN + 1, -(1 << 40), -1, 0, 1 << 40, I64_MAX - 1]
        assert np.all(comp[1:] > comp[:-1])


# ------------------------------------------------------------- case 4: sizes around every boundary
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, (1 << 14) + 3, "tile-1", "tile", "tile+1"]


def _cut_path(ids):
    """A path over ids cut into components of lengths 1, 2, 3, ...; singletons are self-loops."""
    src, dst = [], []
    a, k = 0, 1
    while a < len(ids):
        b = min(a + k, len(ids))
        if b - a == 1:
            src.append(ids[a:b])
            dst.append(ids[a:b])
        else:
            src.append(ids[a:b - 1])
            dst.append(ids[a + 1:b])
        a, k = b, k + 1
    return np.concatenate(src), np.concatenate(dst)


@pytest.mark.parametrize("dense", [False, True], ids=["random-ids", "dense-ids"])
@pytest.mark.parametrize("size", SIZES)
def test_sizes_around_every_boundary(gs, oracle_mod, size, dense):
    """random 64-bit ids run all 16 digit passes; ids 0..n-1 run the pass-skip path (at most
    two low digits of the vertex sort differ). "tile" is the scatter kernel's tile."""
    n = size if isinstance(size, int) else gs.SORT_TILE + {"tile-1": -1, "tile": 0, "tile+1": 1}[size]
    rng = np.random.default_rng(n)
    if dense:
        ids = rng.permutation(n).astype(np.int64)
    else:
        ids = np.unique(rng.integers(I64_MIN, I64_MAX, size=2 * n + 8, dtype=np.int64, endpoint=True))
        ids = rng.permutation(ids)[:n]
    assert len(ids) == n
    src, dst = _cut_path(ids)
    with gs.Summary("cc", capacity_hint=max(16, n)) as s:
        s.fold(src, dst)
        comp, offset, member = _check_cc(s, oracle_mod, src, dst)
        assert len(member) == n


def test_scan_carries_across_chunks(gs):
    """More than 4,096 scatter tiles: k_sort_scan walks each digit row of the histogram table
    in several 4,096-entry chunks with a carry (and the tail's scan of the head counts too).
    The smallest such size is 2,048 * 4,096 rows, too many for the oracle and a host sort within
    a test's time, so the expectation is analytic: ids -n/2 .. n/2 in triples joined to their
    first id, compared on the device."""
    import torch
    n = gs.SORT_TILE * 4096 + 3 * gs.SORT_TILE + 5
    dev = torch.device("cuda", 0)
    ids = torch.arange(n, dtype=torch.int64, device=dev) - n // 2
    first = ids - torch.arange(n, dtype=torch.int64, device=dev) % 3
    nc = (n + 2) // 3
    perm = torch.randperm(n, device=dev)
    src, dst = ids[perm].contiguous(), first[perm].contiguous()
    torch.cuda.synchronize()
    with gs.Summary("cc", capacity_hint=n) as s:
        s.fold_device(src, dst)
        assert s.num_components() == nc
        comp = torch.empty(nc, dtype=torch.int64, device=dev)
        offset = torch.empty(nc + 1, dtype=torch.int64, device=dev)
        member = torch.empty(n, dtype=torch.int64, device=dev)
        assert s.components_device(comp, offset, member) == (n, nc)
        torch.cuda.synchronize()
        assert bool(torch.equal(member, ids)), "members are not the ids in ascending order"
        assert bool(torch.equal(comp, ids[::3]))
        assert bool(torch.equal(offset[:-1], torch.arange(0, n, 3, dtype=torch.int64, device=dev)))
        assert int(offset[-1]) == n


# ------------------------------------------------------------- case 5: a mix of components
def _mixed_stream():
    n = (1 << 17) + 1
    rng = np.random.default_rng(0xC0A5)
    ids = rng.integers(I64_MIN, I64_MAX, size=n, dtype=np.int64, endpoint=True)
    m = int(0.6 * n)
    src = rng.choice(ids, m)
    dst = rng.choice(ids, m)
    fresh = np.setdiff1d(rng.integers(I64_MIN, I64_MAX, size=1100, dtype=np.int64, endpoint=True), ids)[:1000]
    assert len(fresh) == 1000
    side = rng.integers(0, 2, size=n).astype(bool)
    return ids, src, dst, rng.permutation(fresh), side


def _fold_batches(s, src, dst, batch=4096):
    for i in range(0, len(src), batch):
        s.fold(src[i:i + batch], dst[i:i + batch])


def test_mixed_components_cc(gs, oracle_mod):
    """The generator's shape is asserted from the oracle's result so that a changed generator
    cannot hollow the case out. (The oracle counts 45,777 negative ids among the 91,607
    vertices of this generator; the other five figures are the ones the case was specified
    with.)"""
    ids, src, dst, fresh, _ = _mixed_stream()
    ov, olab = oracle_mod.cc_labels(src, dst)
    _, sizes = np.unique(olab, return_counts=True)
    assert len(ov) == 91607 and len(sizes) == 13443 and sizes.max() == 40599
    assert int((sizes == 2).sum()) == 7120 and int((sizes >= 3).sum()) == 6323
    assert int((ov < 0).sum()) == 45777
    src = np.concatenate([src, fresh])
    dst = np.concatenate([dst, fresh])
    with gs.Summary("cc", capacity_hint=1 << 8) as s:
        _fold_batches(s, src, dst)
        comp, offset, member = _check_cc(s, oracle_mod, src, dst)
        assert len(member) == 92607 and len(comp) == 14443


def test_mixed_components_signed(gs, oracle_mod):
    ids, src, dst, fresh, side = _mixed_stream()
    order = np.argsort(ids, kind="stable")
    s_side = side[order][np.searchsorted(ids[order], src)]
    d_side = side[order][np.searchsorted(ids[order], dst)]
    cross = s_side != d_side
    src = np.concatenate([src[cross], fresh])
    dst = np.concatenate([dst[cross], fresh])
    assert 30000 < int(cross.sum()) < 50000  # about half of the 78,643 edges cross
    with gs.Summary("signed", capacity_hint=1 << 8) as s:
        _fold_batches(s, src, dst)
        comp, offset, member, sign = _check_signed(s, oracle_mod, src, dst)
        assert 0 < int(sign.sum()) < len(sign)


# ------------------------------------------------------------- case 6: read-only and repeatable
def test_export_is_read_only_and_repeatable(gs, oracle_mod):
    import torch
    rng = np.random.default_rng(6)
    src = rng.integers(-(1 << 13), 1 << 13, size=5 * 4096, dtype=np.int64)
    dst = rng.integers(-(1 << 13), 1 << 13, size=5 * 4096, dtype=np.int64)
    k = 3 * 4096
    with gs.Summary("cc", capacity_hint=1 << 10) as s:
        _fold_batches(s, src[:k], dst[:k])
        before = s.digest()
        first = s.components()
        assert s.digest() == before
        dev1 = _device_export(s, len(first[3]), len(first[1]))
        assert s.digest() == before
        second = s.components()
        for a, b in zip(first[1:], second[1:]):
            assert np.array_equal(a, b)
        for a, b in zip(first[1:], dev1):
            assert np.array_equal(a, b)
        _check_cc(s, oracle_mod, src[:k], dst[:k])
        # one more fold of 4,096 edges
        s.fold(src[k:k + 4096], dst[k:k + 4096])
        k += 4096
        _check_cc(s, oracle_mod, src[:k], dst[:k])
        # pipelined device folds queued immediately before the export (join_lanes orders them)
        dev = torch.device("cuda", 0)
        ts = torch.from_numpy(src[k:]).to(dev)
        td = torch.from_numpy(dst[k:]).to(dev)
        torch.cuda.synchronize()
        s.set_pipelining(3)
        for i in range(0, 4096, 1024):
            s.fold_device(ts[i:i + 1024], td[i:i + 1024])
        ok, comp, offset, member, sign = s.components()
        ov, olab = oracle_mod.cc_labels(src, dst)
        o = np.lexsort((ov, olab))
        assert np.array_equal(member, ov[o]) and np.array_equal(_expand(comp, offset), olab[o])
        for i in range(0, 4096, 1024):  # the same folds again (idempotent), then the device form
            s.fold_device(ts[i:i + 1024], td[i:i + 1024])
        dcomp, doffset, dmember, _ = _device_export(s, len(member), len(comp))
        assert np.array_equal(dcomp, comp) and np.array_equal(doffset, offset) and np.array_equal(dmember, member)
        s.sync()


# ------------------------------------------------------------- case 7: HBM accounting
def test_scratch_is_counted_and_released(gs):
    n = 5000
    src = np.arange(n, dtype=np.int64)
    dst = src // 7 * 7
    gc.collect()  # (no summary of an earlier test is released while this one counts)
    start = gs.hbm_bytes()
    s = gs.Summary("cc", capacity_hint=n)
    try:
        assert gs.hbm_bytes() - start == gs.create_bytes("cc", n)  # nothing of the export is allocated yet
        s.fold(src, dst)
        s.labels()  # (sizes the unordered export scratch, as the parent path does)
        held = gs.hbm_bytes()
        dcomp, doffset, dmember, _ = _device_export(s, n, n)
        assert len(dmember) == n and len(dcomp) == (n + 6) // 7
        first = gs.hbm_bytes()
        # two (key, payload) buffers of 12 bytes a row and a 256-row histogram table, with headroom
        assert 2 * 12 * n <= first - held <= 4 * 12 * n + (1 << 16)
        _device_export(s, n, n)
        assert gs.hbm_bytes() == first
        s.components()  # the host form adds its staging once
        host = gs.hbm_bytes()
        assert first < host <= first + 2 * (8 + 1 + 16) * n + 64
        s.components()
        assert gs.hbm_bytes() == host
    finally:
        s.close()
    assert gs.hbm_bytes() == start


# ------------------------------------------------------------- case 8: every first-use group
def _first_use_round(gs, kind):
    """One summary through every resource set that a call creates on first use, then closed:
    the result equals a fresh summary's of the same edges, and no device byte stays behind."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0xF1257)

    def edges(n):  # even -> odd ids below 4,096: bipartite, so the signed verdict holds
        return 2 * rng.integers(0, 2048, size=n, dtype=np.int64), 2 * rng.integers(0, 2048, size=n, dtype=np.int64) + 1

    lanes, big, prof, win, other = edges(4000), edges((1 << 18) + 1), edges(100), edges(64), edges(500)
    text_s, text_d = np.array([1, 3, 5], dtype=np.int64), np.array([2, 4, 6], dtype=np.int64)
    gc.collect()  # (no summary of an earlier test is released while this one counts)
    start = gs.hbm_bytes()
    s, t = gs.Summary(kind, capacity_hint=4096), gs.Summary(kind, capacity_hint=4096)
    try:
        # pipelining lanes
        ts, td = torch.from_numpy(lanes[0]).to(dev), torch.from_numpy(lanes[1]).to(dev)
        ws, wd = torch.from_numpy(win[0]).to(dev), torch.from_numpy(win[1]).to(dev)
        rec = torch.empty((64, 3), dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.set_pipelining(4)
        for i in range(0, 4000, 1000):
            s.fold_device(ts[i:i + 1000], td[i:i + 1000])
        # pinned host staging: the smallest host fold that is copied through it
        s.fold(*big)
        # text ingest
        assert s.fold_text(b"1 2\n3 4\n5 6\n") == 3
        # profiling
        s.set_profiling(True)
        s.fold(*prof)
        launches, ms = s.kernel_stats("fold")
        assert launches >= 1 and ms > 0
        s.set_profiling(False)
        # window server
        s.set_delta_tracking(True)
        s.set_window_server(True)
        assert s.fold_take(ws, wd, 64, rec, 64, cnt) <= 64
        assert s.window_server_stats()["windows"] == 1
        # combine scratch (the source's), host staging of components
        t.fold(*other)
        s.combine(t)
        ok, comp, offset, member, sign = s.components()
        assert ok and len(member) == s.num_vertices()
        parts = (lanes, big, (text_s, text_d), prof, win, other)
        src, dst = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        with gs.Summary(kind, capacity_hint=4096) as fresh:
            fresh.fold(src[:1 << 17], dst[:1 << 17])  # (plain folds, each a direct copy)
            fresh.fold(src[1 << 17:], dst[1 << 17:])
            if kind == "cc":
                for a, b in zip(s.labels(), fresh.labels()):
                    assert np.array_equal(a, b)
            else:
                got, want = s.colouring(), fresh.colouring()
                assert got[0] is True and want[0] is True
                for a, b in zip(got[1:], want[1:]):
                    assert np.array_equal(a, b)
    finally:
        s.close()
        t.close()
    assert gs.hbm_bytes() == start


def test_every_first_use_group_is_released(gs):
    """Twice in one process: a handle whose destroy left a stream or an event behind shows up as
    a HIP error at a later create. (That a closed summary returns its component staging is
    test_scratch_is_counted_and_released's; here every other set is in play as well.)"""
    for _ in range(2):
        for kind in ("cc", "signed"):
            _first_use_round(gs, kind)
