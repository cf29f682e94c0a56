"""CPU: the removal entry points of the triangle summary exist, are declared, exported and bound,
and reject bad arguments before touching a device. No compute calls here (the results are
checked on the GPU in test_gpu_triangle_removal.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_triangle_remove", "gs_triangle_remove_device", "gs_triangle_expire", "gs_triangle_set_refresh")
TESTING = {"gs_testing_triangle_remove_stats": r"\(void\* t, uint64_t\* out\);",
           "gs_testing_triangle_remove_phases": r"\(void\* t, uint64_t\* out\);",
           "gs_testing_triangle_set_fold": r"\(void\* t, uint64_t value\);"}


def test_names_are_declared_exported_and_bound(gs):
    with open(os.path.join(ROOT, "include", "gs_summary.h")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "include", "gs_testing.h")) as f:
        testing = f.read()
    L = gs.lib()
    dll = ctypes.CDLL(gs.LIB_PATH)
    for n in NAMES:
        assert n in gs.EXPORTED_SYMBOLS
        assert not re.search(r"\d", n)
        assert hasattr(dll, n)
        assert re.search(r"\bint %s\(gs_triangles \w+[,)]" % n, text), n
        assert getattr(L, n).argtypes, n
    for n, args in TESTING.items():
        assert n in gs.EXPORTED_SYMBOLS
        assert hasattr(dll, n)
        assert re.search(r"\bint %s%s" % (n, args), testing), n
        assert getattr(L, n).argtypes, n


def test_bad_arguments_are_rejected_before_any_device_call(gs):
    L = gs.lib()
    w = (ctypes.c_uint64 * 8)()
    calls = (
        lambda: L.gs_triangle_remove(None, None, None, 0),
        lambda: L.gs_triangle_remove_device(None, None, None, 0, 1),
        lambda: L.gs_triangle_expire(None, 1),
        lambda: L.gs_triangle_set_refresh(None, 1),
        lambda: L.gs_testing_triangle_remove_stats(None, w),
        lambda: L.gs_testing_triangle_remove_phases(None, w),
        lambda: L.gs_testing_triangle_set_fold(None, 1),
    )
    for c in calls:
        assert c() == gs.GS_ERR_INVALID
        assert b"null" in L.gs_last_error()
    # expire(h, 0): the argument is refused whatever the handle is
    assert L.gs_triangle_expire(None, 0) == gs.GS_ERR_INVALID
    assert b"folds must be >= 1" in L.gs_last_error()


def test_python_class_has_the_methods(gs):
    """The removal lives on gsamd.SlidingTriangles, a Triangles with every method of it: the
    public surface of Triangles itself is pinned by test_python_surface.py and stays."""
    import inspect
    cls = gs.SlidingTriangles
    assert issubclass(cls, gs.Triangles) and cls._PREFIX == "gs_triangle"
    for m in ("remove", "remove_device", "expire", "slide", "remove_stats", "fold", "fold_device", "count",
              "local_counts", "find_device", "window", "reset", "stats", "bins"):
        assert callable(getattr(cls, m)), m
    assert inspect.signature(cls.__init__).parameters["refresh"].default is False
    assert str(inspect.signature(cls.__init__)) == "(self, device=0, edge_hint=1048576, refresh=False)"
    p = inspect.signature(cls.remove_device).parameters
    assert [p["n"].default, p["stride"].default, p["after"].default] == [None, 1, None]
    assert list(inspect.signature(cls.slide).parameters)[1:] == ["src", "dst", "panes"]


def test_the_removal_reuses_the_count_kernels():
    """One walk, one set of count kernels: the fold and the removal differ by the Mark they pass."""
    with open(os.path.join(ROOT, "gelly-streaming_amd", "csrc", "gs_triangle_k.hip")) as f:
        text = f.read()
    assert len(re.findall(r"\buint32_t tri_walk\(", text)) == 1
    assert len(re.findall(r"void k_tri_count\(", text)) == 1 and len(re.findall(r"void k_tri_count_lds\(", text)) == 1
    assert "TriFoldMark{" in text and "TriDyingMark{" in text
