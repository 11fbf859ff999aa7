"""CPU-side checks of the depth-distortion stage's C ABI and Python surface (include/gsr_distortion.h): the header is plain C99, the
library exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented order before
anything is enqueued, the Python validators raise before the library is touched, and the trainer parses its flags."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import A, OnDevice, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, pkg, sub

HDR = os.path.join(ROOT, "include", "gsr_distortion.h")
NAMES = {"gsr_distortion_forward", "gsr_distortion_backward"}


def test_distortion_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include <stddef.h>\n#include "gsr_distortion.h"\n'
                                'typedef char first[offsetof(GsrDistortionFrame, W) == 0 && offsetof(GsrDistortionFrame, N) == 8 ? 1 : -1];\n'
                                'typedef char same[offsetof(GsrDistortionFrame, block_masks) == offsetof(GsrFeaturesFrame, block_masks) ? 1 : -1];\n'
                                'typedef char more[offsetof(GsrDistortionFrame, inv_depth) == sizeof(GsrFeaturesFrame) ? 1 : -1];\n'
                                'typedef char size[sizeof(GsrDistortionFrame) == 104 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  int (*f)(const GsrDistortionFrame *, float *, float *, void *) = gsr_distortion_forward;\n'
                                '  int (*b)(const GsrDistortionFrame *, const float *, const float *, float *, void *) = gsr_distortion_backward;\n'
                                '  (void)f; (void)b; return 0; }\n')


def test_distortion_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.DISTORTION_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "DISTORTION_EXPORTS"]
    assert len(tables) >= 16                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_distortion.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "distortion" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_distortion" in ln} == declared   # exactly the declared names
    hdr = open(HDR).read()
    assert C.sizeof(_lib.GsrDistortionFrame) == 104
    names = [f[0] for f in _lib.GsrDistortionFrame._fields_]
    assert names[:12] == [f[0] for f in _lib.GsrFeaturesFrame._fields_] and names[12:] == ["inv_depth", "inv_depth_stride"]
    for word in ("inv_depth_stride", "A S", "(A, mu, S, 0)", "total - P", "may differ from run to run", "No workspace is", "near/far",
                 "pixels 0-31 in order", "3, 4, 6, 7, 9, 10 and 11"):
        assert word in hdr, word


def test_distortion_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN, in
    that order, for both entry points; the argument order is held by which fake pointer a refusal answers to."""
    _lib = sub("_lib")
    L = _lib.lib()

    def frame(**kw):
        f = dict(W=40, H=30, N=100, D=500, xy=A, xy_stride=16, conic_opacity=A + 8, conic_opacity_stride=16, point_list=A, ranges=A, n_contrib=A,
                 block_masks=None, inv_depth=A + 36, inv_depth_stride=16)
        f.update(kw)
        return _lib.GsrDistortionFrame(*(f[k] for k, _ in _lib.GsrDistortionFrame._fields_))

    def fwd(a=A, b=A, c=A, fr=True, **kw):                       # (c: the backward's third array; the forward has two)
        return L.gsr_distortion_forward(C.byref(frame(**kw)) if fr else None, a, b, None)

    def bwd(a=A, b=A, c=A, fr=True, **kw):
        return L.gsr_distortion_backward(C.byref(frame(**kw)) if fr else None, a, b, c, None)

    for call, arrays in ((fwd, ("a", "b")), (bwd, ("a", "b", "c"))):
        assert call(fr=False) == _lib.GSR_E_NULL
        for k in ("xy", "conic_opacity", "ranges", "n_contrib", "point_list", "inv_depth"):
            assert call(**{k: None}) == _lib.GSR_E_NULL, k
            assert call(**{k: None}, a=A + 4) == call(**{k: None}, W=0) == _lib.GSR_E_NULL, k          # NULL before everything else
        for k in arrays:
            assert call(**{k: None}) == call(**{k: None}, W=0) == _lib.GSR_E_NULL, k
        bad_dims = [dict(W=0), dict(H=0), dict(W=-1), dict(W=32769), dict(H=32769), dict(N=0), dict(N=1 << 31), dict(D=-1), dict(D=(1 << 30) + 1),
                    dict(xy_stride=1), dict(conic_opacity_stride=3), dict(inv_depth_stride=0)]
        for kw in bad_dims:
            assert call(**kw) == _lib.GSR_E_DIMS, kw
            assert call(**kw, a=A + 4) == call(**kw, ranges=A + 2) == _lib.GSR_E_DIMS, kw              # ... before alignment
        for k in ("xy", "conic_opacity", "point_list", "ranges", "n_contrib", "inv_depth"):
            assert call(**{k: A + 2}) == call(**{k: A + 1}) == _lib.GSR_E_ALIGN, k
        for k in arrays:
            assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, k
        assert call(point_list=None, D=0, W=0) == _lib.GSR_E_DIMS                                      # (a frame with D = 0 needs no list)


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, dist, loss, bwd = sub("_lib"), sub("distortion"), sub("loss"), sub("backward")
    gsr = pkg()
    assert list(inspect.signature(dist.render_distortion).parameters) == ["buffers", "image_height", "image_width", "out", "use_block_masks"]
    assert list(inspect.signature(loss.distortion_loss_and_gradients).parameters) == ["dist", "mask", "weight"]
    for fn in (gsr.backward,):
        params = inspect.signature(fn).parameters
        for k in ("dL_ddistortion", "distortion_moments"):
            assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None
    assert "distortion" in gsr.__all__

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    dev = lambda t: t.as_subclass(OnDevice)
    N, H, W, D = 7, 20, 33, 50
    tiles = 3 * 2
    i32 = torch.int32
    records = dev(torch.zeros(N, 16))

    def bufs(**kw):
        b = {"points_xy_image": records[:, 0:2], "conic_opacity": records[:, 2:6], "point_list": dev(torch.zeros(D, dtype=i32)),
             "ranges": dev(torch.zeros(tiles, 2, dtype=i32)), "n_contrib": dev(torch.zeros(H, W, dtype=i32)), "depths": dev(torch.ones(N))}
        b.update(kw)
        return b
    for bad_b, what in ((bufs(ranges=dev(torch.zeros(tiles + 1, 2, dtype=i32))), "ranges"), (bufs(n_contrib=dev(torch.zeros(W, H, dtype=i32))), "n_contrib"),
                        (bufs(point_list=dev(torch.zeros(D, dtype=torch.int64))), "point_list"), (bufs(points_xy_image=dev(torch.zeros(N, 3))), "points_xy_image"),
                        (bufs(conic_opacity=dev(torch.zeros(N + 1, 4))), "disagree"), (bufs(depths=dev(torch.ones(N + 1))), "depths"),
                        (bufs(depths=torch.ones(N)), "depths"), (bufs(depths=None), "depths"), (None, "buffers must be the dict")):
        with pytest.raises(ValueError, match=what):
            dist.render_distortion(bad_b, H, W)
    for h, w in ((H + 16, W), (H, W + 16), (0, W), (H, 0), (float(H), W), (True, W)):
        with pytest.raises(ValueError):
            dist.render_distortion(bufs(), h, w)
    good = (dev(torch.zeros(H, W)), dev(torch.zeros(H, W, 4)))
    for bad in (good[0], (good[0],), (good[1], good[0]), (torch.zeros(H, W), good[1]), (good[0], dev(torch.zeros(H, W, 3))),
                (dev(torch.zeros(H, W, dtype=torch.float64)), good[1])):
        with pytest.raises(ValueError, match="out"):
            dist.render_distortion(bufs(), H, W, out=bad)
    with pytest.raises(AssertionError, match="library was touched"):            # valid arguments pass the checks
        dist.render_distortion(bufs(), H, W)
    with pytest.raises(AssertionError, match="library was touched"):
        dist.render_distortion(bufs(), H, W, out=good, use_block_masks=False)
    # the loss is plain torch: nothing to touch, but its arguments are judged
    d = dev(torch.full((H, W), 2.0))
    lo, g = loss.distortion_loss_and_gradients(d, weight=3.0)
    assert tuple(g.shape) == (H, W) and abs(float(g[0, 0]) - 3.0 / (W * H)) < 1e-9 and abs(float(lo) - 6.0) < 1e-5
    mask = np.zeros((H, W), np.float32)
    mask[:5] = 1
    with pytest.raises(ValueError, match="mask"):
        loss.distortion_loss_and_gradients(d, mask=mask[:4])
    for bad in (np.zeros((H, W), np.float32), torch.zeros(H, W), dev(torch.zeros(H, W, 1)), dev(torch.zeros(H, W, dtype=torch.float64))):
        with pytest.raises(ValueError, match="dist must be"):
            loss.distortion_loss_and_gradients(bad)
    with pytest.raises(ValueError, match="weight"):
        loss.distortion_loss_and_gradients(d, weight=float("nan"))
    # backward(): both keywords or neither, refused before anything else is looked at
    for kw in (dict(dL_ddistortion=d), dict(distortion_moments=good[1])):
        with pytest.raises(ValueError, match="dL_ddistortion and distortion_moments together"):
            gsr.backward(None, None, None, **kw)
        with pytest.raises(ValueError, match="dL_ddistortion and distortion_moments together"):
            gsr.backward_view({}, {}, None, {}, None, **kw)


def test_trainer_parses_the_distortion_flags():
    train = os.path.join(ROOT, "examples", "train.py")
    p = subprocess.run([sys.executable, train, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--lambda-dist", "--dist-from-iter", "--report-distortion"):
        assert flag in p.stdout, flag
    for bad, msg in ((["--lambda-dist", "-1"], "--lambda-dist must be >= 0"), (["--dist-from-iter", "-3"], "--dist-from-iter must be >= 0")):
        p = subprocess.run([sys.executable, train] + bad, capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and msg in p.stderr, p.stderr[-500:]
