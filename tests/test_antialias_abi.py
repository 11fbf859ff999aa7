"""CPU-side checks of the antialiased mode's C ABI and Python surface (include/gsr_antialias.h): the header is plain C99, the
library exports what it declares and _lib binds it, every argument of each new entry point is refused in the documented order
before anything is enqueued, `rasterize_mode` is validated before the library is touched, backward() refuses an untagged or stale
frame, and the trainer parses its flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import compile_c99_probe, declared_names, fake_call_setup, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_antialias.h")
NAMES = {"gsr_forward_count_aa", "gsr_forward_capacity_aa", "gsr_backward_aa", "gsr_backward_geom_aa", "gsr_backward_camera_aa"}


def test_antialias_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_antialias.h"\n'
                                'int main(void) {\n'
                                '  float h = GSR_AA_BLUR, fl = GSR_AA_RATIO_FLOOR;\n'
                                '  int (*a)(const GsrScene *, const GsrCamera *, const GsrGeom *, void *, size_t, int64_t *, float *, void *) = gsr_forward_count_aa;\n'
                                '  int (*b)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrBinning *, const GsrImage *, void *, size_t,\n'
                                '           void *, size_t, int64_t, float *, void *) = gsr_forward_capacity_aa;\n'
                                '  int (*c)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrBinning *, const GsrImage *,\n'
                                '           const GsrPixelGrads *, const GsrGrads *, float *, void *, size_t, uint32_t, const float *, void *) = gsr_backward_aa;\n'
                                '  int (*d)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrGrads *, float *, void *, size_t, const float *,\n'
                                '           void *) = gsr_backward_geom_aa;\n'
                                '  int (*e)(const GsrScene *, const GsrCamera *, const GsrGeom *, float *, const void *, size_t, void *, size_t,\n'
                                '           const float *, void *) = gsr_backward_camera_aa;\n'
                                '  (void)h; (void)fl; (void)a; (void)b; (void)c; (void)d; (void)e; return 0; }\n')


def test_antialias_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.ANTIALIAS_EXPORTS) == declared
    for other in (_lib.EXPORTS, _lib.CAPACITY_EXPORTS, _lib.LOSS_EXPORTS, _lib.AUX_EXPORTS, _lib.CAMERA_EXPORTS, _lib.DENSIFY_STATS_EXPORTS):
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_antialias.h" in doc and "aa_scale" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "aa_scale" not in gsr_h
    assert _lib.lib().gsr_abi_version() == 7
    # the CPU twin of the ABI does not get them
    cpu = os.path.join(ROOT, "oracle", "libgsr_cpu.so")
    if os.path.exists(cpu):
        for name in declared:
            assert not hasattr(C.CDLL(cpu), name), name


def test_forward_aa_arguments_are_checked_before_any_hip_call(libpath):
    """Fake 16-byte-aligned pointers: every case returns before anything is dereferenced or enqueued.  The order is the namesake's,
    with aa_scale's alignment among its alignment checks."""
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    geom = _lib.GsrGeom(A, A, A, A, A, A, A, A, A, A, None)
    gws = int(L.gsr_geom_workspace_bytes(N))
    D = C.c_int64(7)

    def count(aa=A, sc=scene, g=geom, ws=A, wsb=gws, out=D):
        return L.gsr_forward_count_aa(C.byref(sc) if sc is not None else None, C.byref(cam), C.byref(g) if g is not None else None, ws, wsb,
                                      C.byref(out) if out is not None else None, aa, None)

    for aa in (A, None):                                                  # NULL is the classic call: the same refusals
        assert count(aa, sc=None) == _lib.GSR_E_NULL
        assert count(aa, sc=_lib.GsrScene(N, A, A, A, A, A, 4, 1.0, 1)) == _lib.GSR_E_DIMS
        assert count(aa, sc=_lib.GsrScene(N, A, A, A, None, A, 3, 1.0, 1)) == _lib.GSR_E_NULL      # scene->opacity
        assert count(aa, out=None) == _lib.GSR_E_NULL
        assert count(aa, g=_lib.GsrGeom(None, A, A, A, A, A, A, A, A, A, None)) == _lib.GSR_E_NULL
        assert count(aa, g=_lib.GsrGeom(A + 4, A, A, A, A, A, A, A, A, A, None)) == _lib.GSR_E_ALIGN
        assert count(aa, ws=None) == _lib.GSR_E_WORKSPACE
        assert count(aa, wsb=gws - 1) == _lib.GSR_E_WORKSPACE
    assert count(A + 4) == _lib.GSR_E_ALIGN
    assert count(A + 4, wsb=gws - 1) == _lib.GSR_E_ALIGN                  # alignment before the workspace
    assert count(A + 4, g=_lib.GsrGeom(None, A, A, A, A, A, A, A, A, A, None)) == _lib.GSR_E_NULL   # NULL before alignment
    assert count(A + 4, sc=_lib.GsrScene(0, None, None, None, None, None, 3, 1.0, 1)) == _lib.GSR_OK and D.value == 0   # N = 0: not looked at

    K = 100
    img = _lib.GsrImage(A, A, A, A)
    bws = int(L.gsr_binning_workspace_bytes(N, K, W, H))

    def cap(aa=A, hint=K, b=None, im=img, g=geom, gb=gws, bb=bws):
        b = b or _lib.GsrBinning(K, A, A, A, A, None, 0)
        return L.gsr_forward_capacity_aa(C.byref(scene), C.byref(cam), C.byref(g), C.byref(b), C.byref(im), A, gb, A, bb, hint, aa, None)

    for aa in (A, None):
        assert cap(aa, im=_lib.GsrImage(None, A, A, A)) == _lib.GSR_E_NULL
        assert cap(aa, b=_lib.GsrBinning(-1, A, A, A, A, None, 0)) == _lib.GSR_E_OVERFLOW
        assert cap(aa, hint=-1) == _lib.GSR_E_OVERFLOW
        assert cap(aa, b=_lib.GsrBinning(K, None, A, A, A, None, 0)) == _lib.GSR_E_NULL
        assert cap(aa, b=_lib.GsrBinning(K, A + 4, A, A, A, None, 0)) == _lib.GSR_E_ALIGN
        assert cap(aa, gb=gws - 1) == _lib.GSR_E_WORKSPACE
        assert cap(aa, bb=bws - 1) == _lib.GSR_E_WORKSPACE
    assert cap(A + 8) == _lib.GSR_E_ALIGN
    assert cap(A + 8, bb=bws - 1) == _lib.GSR_E_ALIGN
    assert cap(A + 8, b=_lib.GsrBinning(K, None, A, A, A, None, 0)) == _lib.GSR_E_NULL


def test_backward_aa_arguments_are_checked_before_any_hip_call(libpath):
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    wsb = int(L.gsr_backward_workspace_bytes(N, 100, W, H))
    img = _lib.GsrImage(None, None, A, A)
    geom = _lib.GsrGeom(A, None, None, A, None, A, A, A, A, A, None)
    PG = _lib.GsrPixelGrads
    ok_gr = _lib.GsrGrads(A, A, A, A, A, None, None, None, None)

    def whole(aa=A, pg=PG(A, None, None), flags=0, D=100, ws=A, b=wsb, gr=ok_gr, inv=None, g=geom, sc=scene):
        bn = _lib.GsrBinning(D, A, A, None, None, None, 0)
        return L.gsr_backward_aa(C.byref(sc), C.byref(cam), C.byref(g), C.byref(bn), C.byref(img), C.byref(pg) if pg is not None else None,
                                 C.byref(gr), inv, ws, b, flags, aa, None)

    def half(aa=A, ws=A, b=wsb, gr=ok_gr, inv=None, g=geom, sc=scene):
        return L.gsr_backward_geom_aa(C.byref(sc), C.byref(cam), C.byref(g), C.byref(gr), inv, ws, b, aa, None)

    for aa in (A, None):
        for flags in (2, 0x80000000):
            assert whole(aa, flags=flags) == _lib.GSR_E_DIMS              # unknown bits, before anything else
        assert whole(aa, pg=None) == _lib.GSR_E_NULL
        assert whole(aa, pg=PG(None, None, None)) == _lib.GSR_E_NULL
        assert whole(aa, pg=PG(A + 4, None, None)) == _lib.GSR_E_ALIGN
        assert whole(aa, D=-1) == _lib.GSR_E_OVERFLOW
        for fn in (whole, half):
            assert fn(aa, sc=_lib.GsrScene(N, A, A, A, None, A, 3, 1.0, 1)) == _lib.GSR_E_NULL     # scene->opacity: the AA kernel reads it
            assert fn(aa, gr=_lib.GsrGrads(None, A, A, A, A, None, None, None, None)) == _lib.GSR_E_NULL
            assert fn(aa, g=_lib.GsrGeom(None, None, None, A, None, A, A, A, A, A, None)) == _lib.GSR_E_NULL
            assert fn(aa, gr=_lib.GsrGrads(A, A, A + 4, A, A, None, None, None, None)) == _lib.GSR_E_ALIGN
            assert fn(aa, inv=A + 4) == _lib.GSR_E_ALIGN
            assert fn(aa, ws=A + 4) == _lib.GSR_E_ALIGN
            assert fn(aa, ws=None) == _lib.GSR_E_WORKSPACE
            assert fn(aa, b=wsb - 1) == _lib.GSR_E_WORKSPACE
            assert fn(aa, sc=_lib.GsrScene(0, None, None, None, None, None, 3, 1.0, 1)) == _lib.GSR_OK
    for fn in (whole, half):
        assert fn(A + 4) == _lib.GSR_E_ALIGN
        assert fn(A + 4, b=wsb - 1) == _lib.GSR_E_ALIGN                   # alignment before the workspace
        assert fn(A + 4, gr=_lib.GsrGrads(None, A, A, A, A, None, None, None, None)) == _lib.GSR_E_NULL
    assert whole(A + 4, D=-1) == _lib.GSR_E_ALIGN                         # ... and before the overflow
    assert whole(A + 4, flags=2) == _lib.GSR_E_DIMS


def test_backward_camera_aa_arguments_are_checked_before_any_hip_call(libpath):
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    wsb = int(L.gsr_backward_workspace_bytes(N, 0, W, H))
    scb = int(L.gsr_backward_camera_scratch_bytes(N))
    geom = _lib.GsrGeom(A, None, None, None, None, None, None, None, A, None, None)

    def call(aa=A, sc=scene, g=geom, out=A, ws=A, b=wsb, scr=A, sb=scb):
        return L.gsr_backward_camera_aa(C.byref(sc), C.byref(cam), C.byref(g) if g is not None else None, out, ws, b, scr, sb, aa, None)

    for aa in (A, None):
        assert call(aa, sc=_lib.GsrScene(N, A, A, A, None, A, 3, 1.0, 1)) == _lib.GSR_E_NULL       # scene->opacity
        assert call(aa, sc=_lib.GsrScene(-1, A, A, A, A, A, 3, 1.0, 1)) == _lib.GSR_E_DIMS
        assert call(aa, out=None) == _lib.GSR_E_NULL
        assert call(aa, out=A + 4) == _lib.GSR_E_ALIGN
        assert call(aa, g=None) == _lib.GSR_E_NULL
        assert call(aa, g=_lib.GsrGeom(A, None, None, None, None, None, None, None, None, None, None)) == _lib.GSR_E_NULL
        assert call(aa, ws=None) == _lib.GSR_E_WORKSPACE
        assert call(aa, b=wsb - 1) == _lib.GSR_E_WORKSPACE
        assert call(aa, sb=scb - 1) == _lib.GSR_E_WORKSPACE
    assert call(A + 4) == _lib.GSR_E_ALIGN
    assert call(A + 4, b=wsb - 1) == _lib.GSR_E_ALIGN
    assert call(A + 4, out=None) == _lib.GSR_E_NULL


# ---- the Python surface ----
def test_rasterize_mode_is_validated_before_the_library_is_touched(monkeypatch):
    _lib, forward, backward = sub("_lib"), sub("forward"), sub("backward")
    import inspect
    for fn in (forward.render_gaussians, backward.backward):
        p = inspect.signature(fn).parameters["rasterize_mode"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "classic"
    assert _lib.RASTERIZE_MODES == ("classic", "antialiased")

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    z = np.zeros((4, 3), np.float32)
    for bad in ("antialias", "Antialiased", None, True, 1, ""):
        with pytest.raises(ValueError, match="rasterize_mode"):
            forward.render_gaussians(np.zeros(3, np.float32), z, rasterize_mode=bad)
        with pytest.raises(ValueError, match="rasterize_mode"):
            backward.backward(np.zeros(3, np.float32), z, np.zeros((8, 8, 3), np.float32), rasterize_mode=bad)
    # the reference's keyword stays accepted and ignored (quirk Q7): it reaches the library as any classic call does
    with pytest.raises(AssertionError, match="library was touched"):
        forward.render_gaussians(np.zeros(3, np.float32), z, antialiasing=True)


def test_backward_refuses_an_untagged_or_stale_frame(monkeypatch):
    """Tag states that Python can see and C cannot: a classic frame or a re-packed copy handed to the antialiased backward, a
    write into the records or the opacity since the render, another opacity tensor, and an antialiased frame handed to the classic
    backward.  Each raises before the library or the GPU is touched."""
    _lib, backward = sub("_lib"), sub("backward")

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    import weakref
    N = 6
    z, bg, dpix = np.zeros((N, 3), np.float32), np.zeros(3, np.float32), np.zeros((8, 8, 3), np.float32)
    call = lambda co, op, mode, **kw: backward.backward(bg, z, dpix, opacity=op, conic_opacity=co, rasterize_mode=mode, **kw)
    records = torch.zeros(N, 16)
    co, op = records[:, 2:6], torch.full((N,), 0.5)
    with pytest.raises(ValueError, match="not a copy of it and not a classic frame"):
        call(co, op, "antialiased")                                        # a classic frame: no tag
    with pytest.raises(ValueError, match="not a copy of it and not a classic frame"):
        call(None, op, "antialiased", geom_buffer={"conic_opacity": co})   # ... found through the geom buffer too
    co._gsr_aa_scale = (torch.ones(N), weakref.ref(op), op._version, co._version, None)
    with pytest.raises(ValueError, match="not a copy of it and not a classic frame"):
        call(co.contiguous(), op, "antialiased")                           # a re-packed copy carries no tag
    with pytest.raises(ValueError, match="pass the same mode"):
        call(co, op, "classic")                                            # an antialiased frame, classic backward
    with pytest.raises(ValueError, match="pass the same mode"):
        backward.backward(bg, z, dpix, opacity=op, geom_buffer={"conic_opacity": co})
    with pytest.raises(ValueError, match="not the tensor this frame was rendered from"):
        call(co, op.clone(), "antialiased")                                # another opacity tensor
    with pytest.raises(AssertionError, match="library was touched"):
        call(co, op, "antialiased")                                        # the valid tag passes the checks
    op.mul_(0.5)
    with pytest.raises(ValueError, match="written in place since"):
        call(co, op, "antialiased")                                        # opacity written since
    co._gsr_aa_scale = (torch.ones(N), weakref.ref(op), op._version, co._version, None)
    records[0, 0] = 1.0                                                    # a write into the records: the view shares their counter
    with pytest.raises(ValueError, match="written in place after the render"):
        call(co, op, "antialiased")


def _train(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_the_rasterize_mode_flag():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--rasterize-mode" in p.stdout and "antialiased" in p.stdout
    p = _train("--rasterize-mode", "mip")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    # a valid mode is parsed before the other arguments are judged: the refusal below is theirs
    p = _train("--rasterize-mode", "antialiased", "--lambda-dssim", "2")
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr
