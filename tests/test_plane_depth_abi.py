"""CPU-side checks of the plane-depth stage's C ABI and Python surface (include/gsr_plane_depth.h): the header is plain C99, the
library exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented order before
anything is enqueued, the Python validators raise before the library is touched, backward()'s signature holds the facts the stage
promised, and the tools parse their flags."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest
import torch

from abi_helpers import A, OnDevice, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, pkg, sub

HDR = os.path.join(ROOT, "include", "gsr_plane_depth.h")
NAMES = {"gsr_plane_slopes", "gsr_plane_slopes_backward", "gsr_plane_depth_forward", "gsr_plane_depth_backward"}


def test_plane_depth_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include <stddef.h>\n#include "gsr_plane_depth.h"\n'
                                'typedef char size[sizeof(GsrDistortionFrame) == 104 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  int (*a)(int64_t, const float *, const float *, const float *, const float *, float, float, int32_t, int32_t, float *, void *)'
                                ' = gsr_plane_slopes;\n'
                                '  int (*d)(int64_t, const float *, const float *, const float *, const float *, float, float, int32_t, int32_t, const float *,'
                                ' float *, float *, void *) = gsr_plane_slopes_backward;\n'
                                '  int (*f)(const GsrDistortionFrame *, const float *, float *, void *) = gsr_plane_depth_forward;\n'
                                '  int (*b)(const GsrDistortionFrame *, const float *, const float *, const float *, float *, float *, void *)'
                                ' = gsr_plane_depth_backward;\n'
                                '  float c = GSR_PLANE_DEPTH_MIN_COS + GSR_PLANE_DEPTH_MAX_FLATNESS + GSR_PLANE_DEPTH_NEAR + GSR_PLANE_DEPTH_MAX_RATIO;\n'
                                '  (void)a; (void)d; (void)f; (void)b; (void)c; return 0; }\n')


def test_plane_depth_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.PLANE_DEPTH_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "PLANE_DEPTH_EXPORTS"]
    assert len(tables) >= 20                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_plane_depth.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "plane" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "plane" in ln} == declared          # exactly the declared names
    hdr = open(HDR).read()
    assert "typedef struct" not in hdr                                                            # the frame is gsr_distortion.h's
    for word in ("GsrDistortionFrame", "fma(-gx, dx, fma(-gy, dy, invd))", "invd * 0.25f", "GSR_PLANE_DEPTH_MIN_COS", "GSR_PLANE_DEPTH_MAX_FLATNESS",
                 "GSR_PLANE_DEPTH_NEAR", "GSR_PLANE_DEPTH_MAX_RATIO", "no atomics", "touches no other accumulator column", "CLEARS", "total-minus-prefix",
                 "left out of the camera gradient", "pixels", "may differ from run", "Stale or foreign buffers", "GSR_E_NULL", "GSR_E_DIMS",
                 "GSR_E_ALIGN", "GSR_E_HIP"):
        assert word in hdr, word
    assert hdr.index("GSR_E_NULL ") < hdr.index("GSR_E_DIMS ") < hdr.index("GSR_E_ALIGN ") < hdr.index("GSR_E_HIP ")
    for name, value in (("MIN_COS", 0.1), ("MAX_FLATNESS", 0.5), ("NEAR", 0.2), ("MAX_RATIO", 4.0)):
        assert getattr(_lib, "PLANE_DEPTH_" + name) == value and f"#define GSR_PLANE_DEPTH_{name} {value}f" in hdr


def test_plane_depth_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN, in
    that order, for all four entry points; the argument order is held by which fake pointer a refusal answers to."""
    _lib = sub("_lib")
    L = _lib.lib()

    def frame(**kw):
        f = dict(W=40, H=30, N=100, D=500, xy=A, xy_stride=16, conic_opacity=A + 8, conic_opacity_stride=16, point_list=A, ranges=A, n_contrib=A,
                 block_masks=None, inv_depth=A + 36, inv_depth_stride=16)
        f.update(kw)
        return _lib.GsrDistortionFrame(*(f[k] for k, _ in _lib.GsrDistortionFrame._fields_))

    def fwd(a=A, b=A, c=A, d=A, e=A, fr=True, **kw):                  # (c, d, e: the backward's further arrays; the forward has two)
        return L.gsr_plane_depth_forward(C.byref(frame(**kw)) if fr else None, a, b, None)

    def bwd(a=A, b=A, c=A, d=A, e=A, fr=True, **kw):
        return L.gsr_plane_depth_backward(C.byref(frame(**kw)) if fr else None, a, b, c, d, e, None)

    for call, arrays in ((fwd, ("a", "b")), (bwd, ("a", "b", "c", "d", "e"))):
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

    good_view = (C.c_float * 16)(*[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])

    def view_of(bad_at=None, value=float("nan")):
        v = (C.c_float * 16)(*good_view)
        if bad_at is not None:
            v[bad_at] = value
        return v

    def slopes(N=100, n=A, s=A, p=A, view=good_view, tx=0.5, ty=0.4, W=40, H=30, out=A):
        return L.gsr_plane_slopes(N, n, s, p, view, tx, ty, W, H, out, None)

    def slopes_bwd(N=100, n=A, s=A, p=A, view=good_view, tx=0.5, ty=0.4, W=40, H=30, out=A, mom=A, dmean=A):
        return L.gsr_plane_slopes_backward(N, n, s, p, view, tx, ty, W, H, mom, dmean, out, None)

    for call, arrays in ((slopes, ("n", "s", "p", "out")), (slopes_bwd, ("n", "s", "p", "out", "mom", "dmean"))):
        for k in arrays + ("view",):
            assert call(**{k: None}) == call(**{k: None}, N=0) == _lib.GSR_E_NULL, k
            if k != "n":
                assert call(**{k: None}, n=A + 4) == _lib.GSR_E_NULL, k                                # NULL before everything else
        for kw in (dict(N=0), dict(N=-1), dict(N=1 << 31), dict(view=view_of(5)), dict(view=view_of(15, float("inf"))), dict(tx=0.0), dict(ty=-1.0),
                   dict(tx=float("nan")), dict(ty=float("inf")), dict(W=0), dict(H=0), dict(W=32769), dict(H=-3)):
            assert call(**kw) == _lib.GSR_E_DIMS, kw
            assert call(**kw, n=A + 4) == _lib.GSR_E_DIMS, kw                                          # ... before alignment
        for k in arrays:
            assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, k


def test_backward_signature_holds_the_promised_facts():
    gsr = pkg()
    nr, pd, tsdf = sub("normal_render"), sub("plane_depth"), sub("tsdf")
    params = inspect.signature(gsr.backward).parameters
    names = list(params)
    for k in ("dL_dplane_depth", "plane_slopes", "plane_depth_image"):
        assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None
        assert names.index(k) < names.index("rendered_stage")                                          # in front of the catch-all
    assert params["plane_param_grad"].kind is inspect.Parameter.KEYWORD_ONLY and params["plane_param_grad"].default is True
    assert names.index("plane_param_grad") < names.index("rendered_stage")
    assert params["rendered_stage"].kind is inspect.Parameter.VAR_KEYWORD and names[-1] == "rendered_stage"
    assert not [n for n in names if any(w in n for w in ("normal", "tsdf", "mesh"))]                   # the substrings existing tests hold the signature by
    assert "gaussian_normals" not in names                                                             # ... it keeps arriving through the catch-all
    assert nr.STAGE_KEYWORDS == {"dL_dnormal_image": None, "gaussian_normals": None, "normal_image": None, "normal_param_grad": True}
    assert "plane_depth" in gsr.__all__ and gsr.plane_depth is pd
    assert list(inspect.signature(pd.plane_slopes).parameters) == ["normals", "scales", "means", "camera", "out"]
    assert list(inspect.signature(pd.render_plane_depth).parameters) == ["slopes", "buffers", "image_height", "image_width", "out", "use_block_masks"]
    fv = inspect.signature(tsdf.fuse_views).parameters
    assert fv["plane_depth"].default is False and fv["depth_mode"].default == "expected" and tsdf.DEPTH_MODES == ("expected", "median")


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, pd, tsdf = sub("_lib"), sub("plane_depth"), sub("tsdf")
    gsr = pkg()

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    dev = lambda t: t.as_subclass(OnDevice)
    N, H, W, D = 8, 20, 33, 50
    tiles = 3 * 2
    i32 = torch.int32
    records = dev(torch.zeros(N, 16))
    cam = {"world_to_camera": torch.eye(4), "tan_fovx": 0.5, "tan_fovy": 0.4, "width": W, "height": H}
    n, s, p = dev(torch.zeros(N, 3)), dev(torch.ones(N, 3)), dev(torch.zeros(N, 3))

    def bufs(**kw):
        b = {"points_xy_image": records[:, 0:2], "conic_opacity": records[:, 2:6], "point_list": dev(torch.zeros(D, dtype=i32)),
             "ranges": dev(torch.zeros(tiles, 2, dtype=i32)), "n_contrib": dev(torch.zeros(H, W, dtype=i32)), "depths": dev(torch.ones(N))}
        b.update(kw)
        return b
    # plane_slopes
    for bad, what in (((torch.zeros(N, 3), s, p, cam), "normals"), ((n, dev(torch.ones(N, 2)), p, cam), "scales"), ((n, s, dev(torch.zeros(N + 1, 3)), cam), "disagree"),
                      ((n.double(), s, p, cam), "normals"), ((n, s, p, dict(cam, tan_fovx=0.0)), "tan_fovx"), ((n, s, p, dict(cam, width=0)), "width"),
                      ((n, s, p, {k: v for k, v in cam.items() if k != "world_to_camera"}), "world_to_camera"),
                      ((n, s, p, dict(cam, world_to_camera=torch.full((4, 4), float("nan")))), "finite")):
        with pytest.raises(ValueError, match=what):
            pd.plane_slopes(*bad)
    for bad in (dev(torch.zeros(N, 3)), torch.zeros(N, 2), dev(torch.zeros(N, 2, dtype=torch.float64)), dev(torch.zeros(N + 1, 2))):
        with pytest.raises(ValueError, match="out"):
            pd.plane_slopes(n, s, p, cam, out=bad)
    with pytest.raises(AssertionError, match="library was touched"):            # valid arguments pass the checks
        pd.plane_slopes(n, s, p, cam, out=dev(torch.zeros(N, 2)))
    with pytest.raises(ValueError, match="dL_dplane_moments"):
        pd.plane_slopes_backward(dev(torch.zeros(N, 2)), n, s, p, cam)
    with pytest.raises(AssertionError, match="library was touched"):
        pd.plane_slopes_backward(dev(torch.zeros(N, 3)), n, s, p, cam)
    # render_plane_depth
    sl = dev(torch.zeros(N, 2))
    for bad_b, what in ((bufs(ranges=dev(torch.zeros(tiles + 1, 2, dtype=i32))), "ranges"), (bufs(n_contrib=dev(torch.zeros(W, H, dtype=i32))), "n_contrib"),
                        (bufs(point_list=dev(torch.zeros(D, dtype=torch.int64))), "point_list"), (bufs(depths=dev(torch.ones(N + 1))), "depths"),
                        (bufs(depths=None), "depths"), (None, "buffers must be the dict")):
        with pytest.raises(ValueError, match=what):
            pd.render_plane_depth(sl, bad_b, H, W)
    for bad in (dev(torch.zeros(N, 3)), dev(torch.zeros(N + 1, 2)), torch.zeros(N, 2), dev(torch.zeros(N, 2, dtype=torch.float64)), dev(torch.zeros(N, 4))[:, :2], None):
        with pytest.raises(ValueError, match="slopes"):
            pd.render_plane_depth(bad, bufs(), H, W)
    for h, w in ((H + 16, W), (H, W + 16), (0, W), (H, 0)):
        with pytest.raises(ValueError):
            pd.render_plane_depth(sl, bufs(), h, w)
    for bad in (dev(torch.zeros(H, W, 1)), torch.zeros(H, W), dev(torch.zeros(W, H)), dev(torch.zeros(H, W, dtype=torch.float64))):
        with pytest.raises(ValueError, match="out"):
            pd.render_plane_depth(sl, bufs(), H, W, out=bad)
    with pytest.raises(AssertionError, match="library was touched"):
        pd.render_plane_depth(sl, bufs(), H, W, out=dev(torch.zeros(H, W)), use_block_masks=False)
    # backward(): the three keywords all or none, and they need gaussian_normals; refused before anything else is looked at
    img = dev(torch.zeros(H, W))
    full = dict(dL_dplane_depth=img, plane_slopes=sl, plane_depth_image=img)
    for drop in full:
        kw = {k: v for k, v in full.items() if k != drop}
        for one in (kw, {k: v for k, v in list(kw.items())[:1]}):
            with pytest.raises(ValueError, match="dL_dplane_depth, plane_slopes and plane_depth_image together"):
                gsr.backward(None, None, None, **one, gaussian_normals=n)
            with pytest.raises(ValueError, match="dL_dplane_depth, plane_slopes and plane_depth_image together"):
                gsr.backward_view({}, {}, None, {}, None, **one)
    with pytest.raises(ValueError, match="needs gaussian_normals"):
        gsr.backward(None, None, None, **full)
    with pytest.raises(ValueError, match="needs gaussian_normals"):
        gsr.backward_view({}, {}, None, {}, None, **full)
    with pytest.raises(ValueError, match="dL_dnormal_image, gaussian_normals and normal_image together"):     # a half-given normal stage is still refused
        gsr.backward(None, None, None, **full, gaussian_normals=n, normal_image=dev(torch.zeros(H, W, 3)))
    with pytest.raises(ValueError, match="dL_dnormal_image, gaussian_normals and normal_image together"):     # ... and gaussian_normals alone belongs to nobody
        gsr.backward(None, None, None, gaussian_normals=n)
    with pytest.raises(TypeError, match="unexpected keyword"):
        gsr.backward(None, None, None, **full, gaussian_normals=n, plane_normals=n)
    # fuse_views: the plane model is not built under the median rule, and it needs the parameters
    with pytest.raises(ValueError, match="plane_depth=True"):
        tsdf.fuse_views(None, [], depth_mode="median", plane_depth=True, params={"positions": p, "scales": s, "rotations": n})
    with pytest.raises(ValueError, match="needs params"):
        tsdf.fuse_views(None, [], plane_depth=True)
    with pytest.raises(ValueError, match="depth_mode"):
        tsdf.fuse_views(None, [], depth_mode="plane")


@pytest.mark.parametrize("script,flags,bad", [
    ("examples/train.py", ("--mesh-depth", "--depth-render", "plane"), (["--depth-render", "mean"], ["--mesh-depth", "mean"])),
    ("examples/extract_mesh.py", ("--depth-mode", "plane"), (["--depth-mode", "mean"],)),
    ("examples/eval_mesh.py", ("--depth-mode", "--demo-flat", "plane"), (["--depth-mode", "mean"],)),
    ("tools/plane_depth_bench.py", ("--config", "--repeats", "--flatten"), (["--config", "C9"],)),
])
def test_tools_parse_the_plane_depth_flags(script, flags, bad):
    path = os.path.join(ROOT, script)
    p = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in flags:
        assert flag in p.stdout, flag
    for args in bad:
        p = subprocess.run([sys.executable, path] + list(args), capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and "invalid choice" in p.stderr, p.stderr[-500:]
    if script == "examples/train.py":                                                  # --depth-render plane wants the L1, as median does
        p = subprocess.run([sys.executable, path, "--depth-render", "plane", "--depth-loss", "pearson", "--lambda-depth", "1"], capture_output=True, text=True,
                           timeout=300)
        assert p.returncode != 0 and "--depth-render plane needs --depth-loss l1" in p.stderr + p.stdout, (p.stderr + p.stdout)[-800:]
