"""CPU-side checks of the mesh-evaluation stage's C ABI and Python surface (include/gsr_mesh_eval.h): the header is plain C99, the
library exports what it declares and _lib binds it in a table of its own, the workspace sizes follow the stated formulas, every
argument is refused in the documented order before anything is enqueued, and the Python validators raise before the library is
touched."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

from abi_helpers import A, OnDevice, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_mesh_eval.h")
NAMES = {"gsr_nearest_workspace_bytes", "gsr_nearest", "gsr_surface_sample_workspace_bytes", "gsr_surface_sample_count", "gsr_surface_sample_emit"}
INF = float("inf")


def test_mesh_eval_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_mesh_eval.h"\n'
                                'typedef char block[GSR_NEAREST_BLOCK_POINTS >= 64 && GSR_NEAREST_BLOCK_POINTS % 64 == 0 ? 1 : -1];\n'
                                'typedef char most[GSR_NEAREST_MAX_POINTS == 134217728 && GSR_SURFACE_SAMPLE_MAX_TRIANGLES == 134217728 ? 1 : -1];\n'
                                'typedef char each[GSR_SURFACE_SAMPLE_MAX_PER_TRIANGLE == 1048576 && GSR_SURFACE_SAMPLE_MAX_SAMPLES == 134217728 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  size_t (*w)(int64_t, int64_t) = gsr_nearest_workspace_bytes;\n'
                                '  int (*f)(int64_t, const float *, int64_t, const float *, float, float *, int32_t *, void *, size_t, void *) = gsr_nearest;\n'
                                '  size_t (*v)(int64_t) = gsr_surface_sample_workspace_bytes;\n'
                                '  int (*c)(int64_t, const float *, float, uint32_t, int32_t *, void *, size_t, void *) = gsr_surface_sample_count;\n'
                                '  int (*e)(int64_t, const float *, const int32_t *, uint32_t, int64_t, float *, int32_t *, void *) = gsr_surface_sample_emit;\n'
                                '  (void)w; (void)f; (void)v; (void)c; (void)e; return 0; }\n')


def test_mesh_eval_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.MESH_EVAL_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "MESH_EVAL_EXPORTS"]
    assert len(tables) >= 18                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_mesh_eval.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "nearest" not in gsr_h.lower() and "surface_sample" not in gsr_h
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_nearest" in ln or "gsr_surface" in ln} == declared      # exactly the declared names
    hdr = open(HDR).read()
    assert f"#define GSR_NEAREST_BLOCK_POINTS {_lib.NEAREST_BLOCK_POINTS} " in hdr
    for macro, value in (("GSR_NEAREST_MAX_POINTS", _lib.NEAREST_MAX_POINTS), ("GSR_SURFACE_SAMPLE_MAX_TRIANGLES", _lib.SURFACE_SAMPLE_MAX_TRIANGLES),
                         ("GSR_SURFACE_SAMPLE_MAX_SAMPLES", _lib.SURFACE_SAMPLE_MAX_SAMPLES)):
        assert f"#define {macro} (1 << 27)\n" in hdr and value == 1 << 27, macro
    assert "#define GSR_SURFACE_SAMPLE_MAX_PER_TRIANGLE (1 << 20)\n" in hdr and _lib.SURFACE_SAMPLE_MAX_PER_TRIANGLE == 1 << 20
    import mesh_eval_reference as R
    assert R.MAX_PER_TRIANGLE == _lib.SURFACE_SAMPLE_MAX_PER_TRIANGLE                     # the yardstick's clamp is the header's


def _up(x):
    return -(-x // 256) * 256


def _nearest_bytes(m, n):
    """The formula in the header's comment."""
    per_set = lambda x: 2 * _up(8 * x) + _up(16 * x) + _up(32 * -(-x // 256))
    h = 256 * -(-max(m, n) // 1024)
    return _up(32 * 2049) + per_set(m) + per_set(n) + 2 * _up(4 * h) + _up(4 * (-(-h // 1024) + 4))


def _sample_bytes(t):
    return _up(4 * (t + 1)) + _up(4 * (-(-(t + 1) // 1024) + 4))


def test_workspace_bytes_follow_the_stated_formulas(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    assert _lib.NEAREST_BLOCK_POINTS == 256                                              # (the formula above is written for it)
    sizes = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4097, 100_000, 1_000_000, (1 << 27) - 1, 1 << 27)
    for m in sizes:
        for n in (1, 257, 1025, 1_000_000, 1 << 27):
            b = int(L.gsr_nearest_workspace_bytes(m, n))
            assert b == _nearest_bytes(m, n) and b % 256 == 0, (m, n)
    for bad in (0, -1, -(1 << 40), (1 << 27) + 1, 1 << 40):
        assert int(L.gsr_nearest_workspace_bytes(bad, 1000)) == int(L.gsr_nearest_workspace_bytes(1000, bad)) == 0, bad
    last = 0
    for t in sizes:
        b = int(L.gsr_surface_sample_workspace_bytes(t))
        assert b == _sample_bytes(t) and b % 256 == 0 and b >= last, t
        last = b
    for bad in (0, -1, (1 << 27) + 1, 1 << 40):
        assert int(L.gsr_surface_sample_workspace_bytes(bad)) == 0, bad


def test_nearest_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN,
    GSR_E_WORKSPACE, in that order."""
    _lib = sub("_lib")
    L = _lib.lib()
    M, N = 1000, 700
    wsb = int(L.gsr_nearest_workspace_bytes(M, N))
    assert wsb > 0

    def call(m=M, q=A, n=N, r=A, cap=INF, d=A, i=A, ws=A, b=wsb):
        return L.gsr_nearest(m, q, n, r, cap, d, i, ws, b, None)

    for k in ("q", "r", "d", "ws"):
        assert call(**{k: None}) == _lib.GSR_E_NULL, k
        assert call(**{k: None}, m=0, b=0) == call(**{k: None}, i=A + 4) == call(**{k: None}, cap=-1.0) == _lib.GSR_E_NULL, k   # NULL before everything else
    for bad in (0, -1, (1 << 27) + 1, 1 << 40):
        for k in ("m", "n"):
            assert call(**{k: bad}) == _lib.GSR_E_DIMS, (k, bad)
            assert call(**{k: bad}, q=A + 4, b=0) == call(**{k: bad}, i=None) == _lib.GSR_E_DIMS, (k, bad)                        # ... before alignment
    for cap in (-1.0, -1e-30, -INF, float("nan")):
        assert call(cap=cap) == call(cap=cap, r=A + 8, b=0) == _lib.GSR_E_DIMS, cap
    for k in ("q", "r", "d", "i", "ws"):
        assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, k
        assert call(**{k: A + 4}, b=wsb - 1) == _lib.GSR_E_ALIGN, k                       # alignment before the workspace
    assert call(b=wsb - 1) == call(b=0) == _lib.GSR_E_WORKSPACE
    for cap in (0.0, 1.5, INF):
        assert call(cap=cap, i=None, b=wsb - 1) == _lib.GSR_E_WORKSPACE                   # (index may be NULL, the cap 0 or inf: not errors)
    assert call(m=1 << 27, b=wsb) == call(n=1 << 27, b=wsb) == _lib.GSR_E_WORKSPACE       # the largest counts are sizes like any other


def test_sampler_arguments_are_checked_in_order_before_any_hip_call(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    T = 1000
    wsb = int(L.gsr_surface_sample_workspace_bytes(T))
    assert wsb > 0

    def count(t=T, tri=A, density=10.0, seed=3, off=A, ws=A, b=wsb):
        return L.gsr_surface_sample_count(t, tri, density, seed, off, ws, b, None)

    def emit(t=T, tri=A, off=A, seed=3, cap=100, pts=A, idx=A):
        return L.gsr_surface_sample_emit(t, tri, off, seed, cap, pts, idx, None)

    for k in ("tri", "off", "ws"):
        assert count(**{k: None}) == count(**{k: None}, t=0, b=0) == count(**{k: None}, density=0.0) == _lib.GSR_E_NULL, k
    for t in (0, -1, (1 << 27) + 1, 1 << 40):
        assert count(t=t) == count(t=t, tri=A + 4, b=0) == _lib.GSR_E_DIMS, t
        assert emit(t=t) == emit(t=t, pts=A + 4) == _lib.GSR_E_DIMS, t
    for density in (0.0, -1.0, INF, float("nan")):
        assert count(density=density) == count(density=density, off=A + 4, b=0) == _lib.GSR_E_DIMS, density
    for k in ("tri", "off", "ws"):
        assert count(**{k: A + 4}) == count(**{k: A + 8}, b=wsb - 1) == _lib.GSR_E_ALIGN, k
    assert count(b=wsb - 1) == count(b=0) == _lib.GSR_E_WORKSPACE
    assert count(t=1 << 27) == _lib.GSR_E_WORKSPACE
    for k in ("tri", "off", "pts"):
        assert emit(**{k: None}) == emit(**{k: None}, t=0) == emit(**{k: None}, cap=0) == _lib.GSR_E_NULL, k
    for cap in (0, -1, (1 << 27) + 1, 1 << 40):
        assert emit(cap=cap) == emit(cap=cap, idx=A + 4) == emit(cap=cap, idx=None) == _lib.GSR_E_DIMS, cap
    for k in ("tri", "off", "pts", "idx"):
        assert emit(**{k: A + 4}) == emit(**{k: A + 8}) == _lib.GSR_E_ALIGN, k


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, me = sub("_lib"), sub("mesh_eval")
    assert list(inspect.signature(me.nearest).parameters) == ["queries", "refs", "max_dist", "want_indices", "out", "max_dist2"]
    assert list(inspect.signature(me.sample_mesh).parameters) == ["triangles", "density", "samples", "seed", "device"]
    assert list(inspect.signature(me.evaluate).parameters) == ["pred_points", "gt_points", "thresholds", "max_dist", "bounds"]
    assert inspect.signature(me.nearest).parameters["max_dist"].default == INF
    assert inspect.signature(me.sample_mesh).parameters["seed"].default == 0

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    dev = lambda t: t.as_subclass(OnDevice)
    good, refs = dev(torch.zeros(5, 3)), dev(torch.zeros(7, 3))
    for bad, what in ((np.zeros((5, 3), np.float32), "torch tensor"), (torch.zeros(5, 3), "GPU"), (dev(torch.zeros(5, 3, dtype=torch.float64)), "float32"),
                      (dev(torch.zeros(15)), r"shape \(N, 3\)"), (dev(torch.zeros(5, 4)), r"shape \(N, 3\)"), (dev(torch.zeros(0, 3)), "N >= 1"),
                      (dev(torch.zeros(5, 6)[:, ::2]), "contiguous"), (dev(torch.zeros(3, 5).t()), "contiguous")):
        with pytest.raises(ValueError, match="queries.*" + what):
            me.nearest(bad, refs)
        with pytest.raises(ValueError, match="refs.*" + what):
            me.nearest(good, bad)
    for bad in (-1.0, float("nan"), -INF, "far"):
        with pytest.raises(ValueError, match="max_dist"):
            me.nearest(good, refs, max_dist=bad)
        with pytest.raises(ValueError, match="max_dist2"):
            me.nearest(good, refs, max_dist2=bad)
    with pytest.raises(ValueError, match="not both"):
        me.nearest(good, refs, max_dist=1.0, max_dist2=1.0)
    assert me.cap2(INF) == INF and me.cap2(0.0) == 0.0 and me.cap2(None, 0.046875) == 0.046875 and me.cap2(0.1) == float(np.float32(0.1 * 0.1))
    assert me.cap2(1e30) == INF                                                           # beyond float32: every reference is a candidate
    for bad in (torch.zeros(5), dev(torch.zeros(4)), dev(torch.zeros(5, 1)), dev(torch.zeros(5, dtype=torch.float64)), dev(torch.zeros(10)[::2]),
                np.zeros(5, np.float32), (dev(torch.zeros(5)), dev(torch.zeros(5, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="dist2"):
            me.nearest(good, refs, out=bad)
    ok_d, ok_i = dev(torch.zeros(5)), dev(torch.zeros(5, dtype=torch.int32))
    for bad in (ok_d, (ok_d,), (ok_d, ok_i, ok_i)):
        with pytest.raises(ValueError, match="pair"):
            me.nearest(good, refs, want_indices=True, out=bad)
    for bad in (dev(torch.zeros(5)), dev(torch.zeros(5, dtype=torch.int64)), dev(torch.zeros(4, dtype=torch.int32)), torch.zeros(5, dtype=torch.int32),
                dev(torch.zeros(5, 1, dtype=torch.int32))):
        with pytest.raises(ValueError, match="indices"):
            me.nearest(good, refs, want_indices=True, out=(ok_d, bad))
    # the sampler
    tri = dev(torch.zeros(4, 3, 3))
    for bad, what in (([[[0.0] * 3] * 3], "torch tensor or a numpy array"), (np.zeros((4, 3, 3)), "float32"), (np.zeros((4, 9), np.float32), r"\(T, 3, 3\)"),
                      (dev(torch.zeros(0, 3, 3)), "T >= 1"), (np.zeros((4, 3, 2), np.float32), r"\(T, 3, 3\)")):
        with pytest.raises(ValueError, match=what):
            me.sample_mesh(bad, density=1.0)
    for kw in ({}, {"density": 1.0, "samples": 10}):
        with pytest.raises(ValueError, match="exactly one of density and samples"):
            me.sample_mesh(tri, **kw)
    for bad in (0.0, -1.0, INF, float("nan"), "dense"):
        with pytest.raises(ValueError, match="density"):
            me.sample_mesh(tri, density=bad)
    for bad in (0, -5, 2.5, (1 << 27) + 1, True):
        with pytest.raises(ValueError, match="samples must be an integer"):
            me.sample_mesh(tri, samples=bad)
    for bad in (-1, 1 << 32, 0.5, True, None):
        with pytest.raises(ValueError, match="seed must be an integer"):
            me.sample_mesh(tri, density=1.0, seed=bad)
    # evaluate
    host = torch.zeros(5, 3)
    for kw, what in (({"thresholds": ()}, "thresholds"), ({"thresholds": (0.1, 0.0)}, "thresholds"), ({"thresholds": (INF,)}, "thresholds"),
                     ({"thresholds": 0.1}, "thresholds"), ({"max_dist": 0.0}, "max_dist"), ({"max_dist": -1.0}, "max_dist"),
                     ({"bounds": (0, 1)}, "bounds"), ({"bounds": ((0, 0, 0), (1, 1, -1))}, "bounds"), ({"bounds": ((0, 0, 0),)}, "bounds")):
        with pytest.raises(ValueError, match=what):
            me.evaluate(host, host, **kw)
    for bad, what in ((np.zeros((5, 3)), "float32"), (torch.zeros(5, 2), r"shape \(N, 3\)"), ([[0.0, 0.0, 0.0]], "torch tensor")):
        with pytest.raises(ValueError, match="pred_points.*" + what):
            me.evaluate(bad, host)
        with pytest.raises(ValueError, match="gt_points.*" + what):
            me.evaluate(host, bad)
    # valid arguments pass the checks
    for call in (lambda: me.nearest(good, refs), lambda: me.nearest(good, refs, max_dist=0.5, out=ok_d), lambda: me.nearest(good, refs, max_dist2=0.0),
                 lambda: me.nearest(good, refs, want_indices=True, out=(ok_d, ok_i)), lambda: me.sample_mesh(tri, density=2.0, seed=(1 << 32) - 1),
                 lambda: me.sample_mesh(np.zeros((4, 3, 3), np.float32), samples=100)):
        with pytest.raises(AssertionError, match="library was touched"):
            call()
