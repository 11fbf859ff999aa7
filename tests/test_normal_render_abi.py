"""CPU-side checks of the normal-rendering stage's C ABI and Python surface (include/gsr_normal_render.h): the header is plain C99, the
library exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented order before
anything is enqueued, the Python validators raise before the library is touched, backward() takes its three keywords together or
not at all, and the trainer parses its flags."""
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

HDR = os.path.join(ROOT, "include", "gsr_normal_render.h")
NAMES = {"gsr_gaussian_normals", "gsr_gaussian_normals_backward", "gsr_normal_render_forward", "gsr_normal_render_backward",
         "gsr_normal_consistency_loss"}


def test_normal_render_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include <stddef.h>\n#include "gsr_normal_render.h"\n'
                                'int main(void) {\n'
                                '  int (*a)(int64_t, const float *, const float *, const float *, const float *, float *, void *) = gsr_gaussian_normals;\n'
                                '  int (*b)(int64_t, const float *, const float *, const float *, const float *, const float *, float *, void *)'
                                ' = gsr_gaussian_normals_backward;\n'
                                '  int (*c)(const GsrFeaturesFrame *, const float *, float *, void *) = gsr_normal_render_forward;\n'
                                '  int (*d)(const GsrFeaturesFrame *, const float *, const float *, const float *, float *, float *, void *)'
                                ' = gsr_normal_render_backward;\n'
                                '  int (*e)(const float *, const float *, const float *, const float *, int32_t, int32_t, float, float *, float *, float *,'
                                ' void *, size_t, void *) = gsr_normal_consistency_loss;\n'
                                '  float t = GSR_NORMAL_RENDER_MIN_LENGTH + GSR_NORMAL_RENDER_MIN_AXIS2;\n'
                                '  (void)a; (void)b; (void)c; (void)d; (void)e; (void)t; return 0; }\n')


def test_normal_render_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.NORMAL_RENDER_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "NORMAL_RENDER_EXPORTS"]
    assert len(tables) >= 17                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_normal_render.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "normal_render" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    mine = {ln.split()[-1] for ln in exported.splitlines() if any(w in ln for w in ("gsr_normal_render", "gsr_gaussian_normals", "gsr_normal_consistency"))}
    assert mine == declared                                                              # exactly the declared names
    hdr = open(HDR).read()
    for word in ("strict <", "sigma3d.h", "1e-24f", "held constant", "left out of the camera gradient", "bit for bit gsr_features_forward at C = 3",
                 "total - P", "eps32 |total|", "pixels 0-31 in order", "3, 4, 6, 7, 9 and 10", "CLEARS dL_dnormals", "may differ from run to run",
                 "GSR_NORMAL_RENDER_MIN_LENGTH", "the same bits every call", "gsr_normals_workspace_bytes"):
        assert word in hdr, word
    assert _lib.NORMAL_RENDER_MIN_LENGTH == 1e-3 and _lib.NORMAL_RENDER_MIN_AXIS2 == 1e-24


def test_normal_render_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN (and
    GSR_E_WORKSPACE last), in that order, for all five entry points; the argument order is held by which fake pointer a refusal
    answers to.  Only `viewmatrix` is real memory: it is a host array, read by the DIMS check."""
    _lib = sub("_lib")
    L = _lib.lib()
    view = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    bad_view = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    bad_view[5] = float("nan")

    # (a), (b)
    def normals(N=100, s=A, q=A, p=A, v=view, out=A, g=A, bwd=False):
        if bwd:
            return L.gsr_gaussian_normals_backward(N, s, q, p, v, g, out, None)
        return L.gsr_gaussian_normals(N, s, q, p, v, out, None)

    for bwd, arrays in ((False, ("s", "q", "p", "out")), (True, ("s", "q", "p", "g", "out"))):
        for k in arrays + ("v",):
            assert normals(bwd=bwd, **{k: None}) == normals(bwd=bwd, **{k: None}, N=0) == _lib.GSR_E_NULL, k
            assert normals(bwd=bwd, **{k: None}, **({"s": A + 4} if k != "s" else {"q": A + 4})) == _lib.GSR_E_NULL, k
        for kw in (dict(N=0), dict(N=-1), dict(N=1 << 31), dict(v=bad_view)):
            assert normals(bwd=bwd, **kw) == normals(bwd=bwd, **kw, s=A + 4) == _lib.GSR_E_DIMS, kw
        for k in arrays:
            assert normals(bwd=bwd, **{k: A + 4}) == normals(bwd=bwd, **{k: A + 8}) == _lib.GSR_E_ALIGN, k

    # (c), (d)
    def frame(**kw):
        f = dict(W=40, H=30, N=100, D=500, xy=A, xy_stride=16, conic_opacity=A + 8, conic_opacity_stride=16, point_list=A, ranges=A, n_contrib=A,
                 block_masks=None)
        f.update(kw)
        return _lib.GsrFeaturesFrame(*(f[k] for k, _ in _lib.GsrFeaturesFrame._fields_))

    def fwd(a=A, b=A, c=A, d=A, e=A, fr=True, **kw):             # (c, d, e: the backward's further arrays; the forward has two)
        return L.gsr_normal_render_forward(C.byref(frame(**kw)) if fr else None, a, b, None)

    def bwd(a=A, b=A, c=A, d=A, e=A, fr=True, **kw):
        return L.gsr_normal_render_backward(C.byref(frame(**kw)) if fr else None, a, b, c, d, e, None)

    for call, arrays in ((fwd, ("a", "b")), (bwd, ("a", "b", "c", "d", "e"))):
        assert call(fr=False) == _lib.GSR_E_NULL
        for k in ("xy", "conic_opacity", "ranges", "n_contrib", "point_list"):
            assert call(**{k: None}) == _lib.GSR_E_NULL, k
            assert call(**{k: None}, a=A + 4) == call(**{k: None}, W=0) == _lib.GSR_E_NULL, k          # NULL before everything else
        for k in arrays:
            assert call(**{k: None}) == call(**{k: None}, W=0) == _lib.GSR_E_NULL, k
        bad_dims = [dict(W=0), dict(H=0), dict(W=-1), dict(W=32769), dict(H=32769), dict(N=0), dict(N=1 << 31), dict(D=-1), dict(D=(1 << 30) + 1),
                    dict(xy_stride=1), dict(conic_opacity_stride=3)]
        for kw in bad_dims:
            assert call(**kw) == _lib.GSR_E_DIMS, kw
            assert call(**kw, a=A + 4) == call(**kw, ranges=A + 2) == _lib.GSR_E_DIMS, kw              # ... before alignment
        for k in ("xy", "conic_opacity", "point_list", "ranges", "n_contrib"):
            assert call(**{k: A + 2}) == call(**{k: A + 1}) == _lib.GSR_E_ALIGN, k
        for k in arrays:
            assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, k
        assert call(point_list=None, D=0, W=0) == _lib.GSR_E_DIMS                                      # (a frame with D = 0 needs no list)

    # (e)
    W, H = 40, 30
    need = int(L.gsr_normals_workspace_bytes(W, H))
    assert need > 0

    def loss(N=A, nd=A, valid=A, m=None, W=W, H=H, weight=1.0, gN=A, gnd=A, sums=A, ws=A, nbytes=need):
        return L.gsr_normal_consistency_loss(N, nd, valid, m, W, H, weight, gN, gnd, sums, ws, nbytes, None)

    for k in ("N", "nd", "valid", "gN", "gnd", "sums", "ws"):
        assert loss(**{k: None}) == loss(**{k: None}, W=0) == loss(**{k: None}, nbytes=0) == _lib.GSR_E_NULL, k
    for kw in (dict(W=0), dict(H=0), dict(W=-1), dict(W=1 << 15, H=1 << 15), dict(weight=float("nan")), dict(weight=float("inf"))):
        assert loss(**kw) == loss(**kw, gN=A + 4) == loss(**kw, nbytes=0) == _lib.GSR_E_DIMS, kw
    for k in ("N", "nd", "valid", "m", "gN", "gnd", "ws"):
        assert loss(**{k: A + 4}) == loss(**{k: A + 4}, nbytes=0) == _lib.GSR_E_ALIGN, k
    assert loss(sums=A + 2) == _lib.GSR_E_ALIGN and loss(m=A, nbytes=need - 1) == _lib.GSR_E_WORKSPACE    # (sums: any slot of a float array)


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, nr, loss, bwd = sub("_lib"), sub("normal_render"), sub("loss"), sub("backward")
    gsr = pkg()
    assert list(inspect.signature(nr.gaussian_normals).parameters) == ["scales", "rotations", "means", "camera", "out"]
    assert list(inspect.signature(nr.render_normals).parameters) == ["normals", "buffers", "image_height", "image_width", "out", "use_block_masks"]
    assert list(inspect.signature(loss.normal_consistency_loss_and_gradients).parameters)[:6] == ["normal_image", "depth", "final_Ts", "camera", "mask",
                                                                                                   "weight"]
    # the four keywords are taken by name through backward()'s catch-all (tests/test_normals_abi.py holds that no parameter of the
    # signature has "normal" in its name): keyword-only by construction, these four names with these defaults and no others
    params = inspect.signature(gsr.backward).parameters
    assert [p.kind for p in params.values()].count(inspect.Parameter.VAR_KEYWORD) == 1 and not [p for p in params if "normal" in p]
    assert nr.STAGE_KEYWORDS == {"dL_dnormal_image": None, "gaussian_normals": None, "normal_image": None, "normal_param_grad": True}
    assert nr.stage_keywords({}) == (None, None, None, True) and nr.stage_keywords({"normal_param_grad": False, "normal_image": 3}) == (None, None, 3, False)
    for bad in ("dL_dnormals_image", "normal_images", "gaussian_normal", "anything"):
        with pytest.raises(TypeError, match=f"unexpected keyword argument '{bad}'"):
            gsr.backward(None, None, None, **{bad: 1})
    assert "normal_render" in gsr.__all__

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    dev = lambda t: t.as_subclass(OnDevice)
    N, H, W, D = 7, 20, 33, 50
    tiles = 3 * 2
    i32 = torch.int32
    records = dev(torch.zeros(N, 16))
    cam = {"world_to_camera": np.eye(4, dtype=np.float32), "tan_fovx": 0.5, "tan_fovy": 0.4, "width": W, "height": H}
    s, q, p = dev(torch.ones(N, 3)), dev(torch.ones(N, 4)), dev(torch.zeros(N, 3))

    # gaussian_normals
    for bad, what in (((torch.ones(N, 3), q, p), "scales"), ((dev(torch.ones(N, 4)), q, p), "scales"), ((s, dev(torch.ones(N, 3)), p), "rotations"),
                      ((s, q, dev(torch.zeros(N + 1, 3))), "disagree"), ((s, dev(torch.ones(N, 4, dtype=torch.float64)), p), "rotations")):
        with pytest.raises(ValueError, match=what):
            nr.gaussian_normals(*bad, cam)
    for bad_cam in ({}, {"world_to_camera": np.eye(3)}, np.full((4, 4), np.nan), "view"):
        with pytest.raises(ValueError, match="view matrix|world_to_camera"):
            nr.gaussian_normals(s, q, p, bad_cam)
    with pytest.raises(ValueError, match="out"):
        nr.gaussian_normals(s, q, p, cam, out=dev(torch.zeros(N, 4)))
    with pytest.raises(AssertionError, match="library was touched"):
        nr.gaussian_normals(s, q, p, cam)
    with pytest.raises(AssertionError, match="library was touched"):
        nr.gaussian_normals(s, q, p, np.eye(4), out=dev(torch.zeros(N, 3)))
    with pytest.raises(ValueError, match="dL_dnormals"):
        nr.gaussian_normals_backward(dev(torch.zeros(N, 4)), s, q, p, cam)
    with pytest.raises(AssertionError, match="library was touched"):
        nr.gaussian_normals_backward(dev(torch.zeros(N, 3)), s, q, p, cam)

    # render_normals
    def bufs(**kw):
        b = {"points_xy_image": records[:, 0:2], "conic_opacity": records[:, 2:6], "point_list": dev(torch.zeros(D, dtype=i32)),
             "ranges": dev(torch.zeros(tiles, 2, dtype=i32)), "n_contrib": dev(torch.zeros(H, W, dtype=i32))}
        b.update(kw)
        return b
    n = dev(torch.zeros(N, 3))
    for bad_b, what in ((bufs(ranges=dev(torch.zeros(tiles + 1, 2, dtype=i32))), "ranges"), (bufs(n_contrib=dev(torch.zeros(W, H, dtype=i32))), "n_contrib"),
                        (bufs(point_list=dev(torch.zeros(D, dtype=torch.int64))), "point_list"), (None, "buffers must be the dict")):
        with pytest.raises(ValueError, match=what):
            nr.render_normals(n, bad_b, H, W)
    for bad_n in (torch.zeros(N, 3), dev(torch.zeros(N + 1, 3)), dev(torch.zeros(N, 4)), dev(torch.zeros(N, 3, dtype=torch.float64)), dev(torch.zeros(3, N)).T):
        with pytest.raises(ValueError, match="normals must be"):
            nr.render_normals(bad_n, bufs(), H, W)
    for h, w in ((H + 16, W), (H, W + 16), (0, W), (float(H), W), (True, W)):
        with pytest.raises(ValueError):
            nr.render_normals(n, bufs(), h, w)
    for bad in (dev(torch.zeros(H, W)), torch.zeros(H, W, 3), dev(torch.zeros(H, W, 4)), dev(torch.zeros(H, W, 3, dtype=torch.float64))):
        with pytest.raises(ValueError, match="out"):
            nr.render_normals(n, bufs(), H, W, out=bad)
    with pytest.raises(AssertionError, match="library was touched"):
        nr.render_normals(n, bufs(), H, W, out=dev(torch.zeros(H, W, 3)), use_block_masks=False)

    # the loss
    nimg, depth, T = dev(torch.zeros(H, W, 3)), dev(torch.ones(H, W)), dev(torch.zeros(H, W))
    for args, kw, what in (((torch.zeros(H, W, 3), depth, T, cam), {}, "normal_image"), ((dev(torch.zeros(H, W)), depth, T, cam), {}, "normal_image"),
                           ((nimg, dev(torch.ones(W, H)), T, cam), {}, "depth"), ((nimg, depth, dev(torch.ones(H, W + 1)), cam), {}, "final_Ts"),
                           ((nimg, depth, T, {"width": W}), {}, "camera"), ((nimg, depth, T, cam), dict(mask=np.ones((H, 2), np.float32)), "mask"),
                           ((nimg, depth, T, cam), dict(weight=float("nan")), "weight"), ((nimg, depth, T, cam), dict(loss_out=dev(torch.zeros(3))), "loss_out")):
        with pytest.raises(ValueError, match=what):
            loss.normal_consistency_loss_and_gradients(*args, **kw)
    with pytest.raises(AssertionError, match="library was touched"):
        loss.normal_consistency_loss_and_gradients(nimg, depth, T, cam, weight=0.05)

    # backward(): the three keywords together or not at all, refused before anything else is looked at
    triple = dict(dL_dnormal_image=nimg, gaussian_normals=n, normal_image=nimg)
    for drop in triple:
        for kw in ({k: v for k, v in triple.items() if k != drop}, {drop: triple[drop]}):
            with pytest.raises(ValueError, match="dL_dnormal_image, gaussian_normals and normal_image together"):
                gsr.backward(None, None, None, **kw)
            with pytest.raises(ValueError, match="dL_dnormal_image, gaussian_normals and normal_image together"):
                gsr.backward_view({}, {}, None, {}, None, **kw)


def test_trainer_parses_the_normal_consistency_flags():
    train = os.path.join(ROOT, "examples", "train.py")
    p = subprocess.run([sys.executable, train, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--lambda-normal-consistency", "--normal-consistency-from-iter", "--report-normal-consistency"):
        assert flag in p.stdout, flag
    for bad, msg in ((["--lambda-normal-consistency", "-1"], "--lambda-normal-consistency must be >= 0"),
                     (["--normal-consistency-from-iter", "-3"], "--normal-consistency-from-iter must be >= 0")):
        p = subprocess.run([sys.executable, train] + bad, capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and msg in p.stderr, p.stderr[-500:]
