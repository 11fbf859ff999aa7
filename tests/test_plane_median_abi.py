"""CPU-side checks of the C ABI and Python surface of the plane depth under the median rule (include/gsr_plane_median.h): the header is
plain C99, the library exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented
order before anything is enqueued, the Python validators raise before the library is touched, fuse_views takes the new value of its
keyword and keeps its refusals, and the tools parse their flags."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest
import torch

from abi_helpers import A, OnDevice, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, pkg, sub

HDR = os.path.join(ROOT, "include", "gsr_plane_median.h")
NAMES = {"gsr_pmed_forward", "gsr_pmed_backward"}


def test_plane_median_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include <stddef.h>\n#include "gsr_plane_median.h"\n'
                                'typedef char size[sizeof(GsrDistortionFrame) == 104 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  int (*f)(const GsrDistortionFrame *, const float *, float *, int32_t *, void *) = gsr_pmed_forward;\n'
                                '  int (*b)(const GsrDistortionFrame *, const float *, const float *, const int32_t *, float *, void *) = gsr_pmed_backward;\n'
                                '  float c = GSR_PLANE_DEPTH_MAX_RATIO;\n'
                                '  (void)f; (void)b; (void)c; return 0; }\n')


def test_plane_median_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.PLANE_MEDIAN_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "PLANE_MEDIAN_EXPORTS"]
    assert len(tables) >= 21                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_plane_median.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "pmed" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_pmed" in ln} == declared        # exactly the declared names
    hdr = open(HDR).read()
    assert "typedef struct" not in hdr and "#define GSR_" not in hdr.split("#define GSR_PLANE_MEDIAN_H")[1]   # the frame, the clamp: the neighbours'
    for word in ("GsrDistortionFrame", "fma(-gx, dx, fma(-gy, dy, invd))", "invd * 0.25f", "T > 0.5f", "n_contrib's convention", "no atomics",
                 "bit for bit median_contrib of gsr_median_depth_forward", "bit for bit that call's median_inv_depth",
                 "dL_dplane_moments[id] += (g,  g * (-dx),  g * (-dy))", "A clamped entry is a constant", "No accumulator column is touched",
                 "THE CALLER CLEARS", "pixels 0-31 in order", "may differ from run", "(n + 2) 2^-24", "never an access out of bounds",
                 "No workspace is", "GSR_E_NULL", "GSR_E_DIMS", "GSR_E_ALIGN", "GSR_E_HIP"):
        assert word in hdr, word
    assert hdr.index("GSR_E_NULL ") < hdr.index("GSR_E_DIMS ") < hdr.index("GSR_E_ALIGN ") < hdr.index("GSR_E_HIP ")


def test_plane_median_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN, in
    that order, for both entry points; the argument order is held by which fake pointer a refusal answers to."""
    _lib = sub("_lib")
    L = _lib.lib()

    def frame(**kw):
        f = dict(W=40, H=30, N=100, D=500, xy=A, xy_stride=16, conic_opacity=A + 8, conic_opacity_stride=16, point_list=A, ranges=A, n_contrib=A,
                 block_masks=None, inv_depth=A + 36, inv_depth_stride=16)
        f.update(kw)
        return _lib.GsrDistortionFrame(*(f[k] for k, _ in _lib.GsrDistortionFrame._fields_))

    def fwd(a=A, b=A, c=A, d=A, fr=True, **kw):                  # (d: the backward's fourth array; the forward has three)
        return L.gsr_pmed_forward(C.byref(frame(**kw)) if fr else None, a, b, c, None)

    def bwd(a=A, b=A, c=A, d=A, fr=True, **kw):
        return L.gsr_pmed_backward(C.byref(frame(**kw)) if fr else None, a, b, c, d, None)

    for call, arrays in ((fwd, ("a", "b", "c")), (bwd, ("a", "b", "c", "d"))):
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
    assert bwd(point_list=None, D=0) == _lib.GSR_OK                                                    # D = 0: the backward enqueues nothing


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, pd, tsdf = sub("_lib"), sub("plane_depth"), sub("tsdf")
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(pd.render_plane_median_depth) == ["slopes", "buffers", "image_height", "image_width", "out", "use_block_masks"]
    assert sig(pd.plane_median_depth_backward) == ["dL_dmedian", "contrib", "slopes", "buffers", "image_height", "image_width", "out", "accumulate"]
    assert inspect.signature(pd.plane_median_depth_backward).parameters["accumulate"].default is False
    assert sig(pd.plane_median_gradients) == ["params", "camera", "buffers", "dL_dmedian", "contrib", "slopes", "normals", "grads"]
    assert sig(pd.render_view_plane_median_depth) == ["params", "camera", "buffers"]
    # the pinned neighbours stay
    assert sig(pd.plane_slopes) == ["normals", "scales", "means", "camera", "out"]
    assert sig(pd.render_plane_depth) == ["slopes", "buffers", "image_height", "image_width", "out", "use_block_masks"]
    fv = inspect.signature(tsdf.fuse_views).parameters
    assert fv["plane_depth"].default is False and fv["depth_mode"].default == "expected" and tsdf.DEPTH_MODES == ("expected", "median")
    assert not [n for n in inspect.signature(pkg().backward).parameters if "plane_median" in n]          # no stage of backward()

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    dev = lambda t: t.as_subclass(OnDevice)
    N, H, W, D = 8, 20, 33, 50
    tiles = 3 * 2
    i32 = torch.int32
    records = dev(torch.zeros(N, 16))

    def bufs(**kw):
        b = {"points_xy_image": records[:, 0:2], "conic_opacity": records[:, 2:6], "point_list": dev(torch.zeros(D, dtype=i32)),
             "ranges": dev(torch.zeros(tiles, 2, dtype=i32)), "n_contrib": dev(torch.zeros(H, W, dtype=i32)), "depths": dev(torch.ones(N))}
        b.update(kw)
        return b
    sl = dev(torch.zeros(N, 2))
    g, contrib = dev(torch.zeros(H, W)), dev(torch.zeros(H, W, dtype=i32))
    bad_bufs = ((bufs(ranges=dev(torch.zeros(tiles + 1, 2, dtype=i32))), "ranges"), (bufs(n_contrib=dev(torch.zeros(W, H, dtype=i32))), "n_contrib"),
                (bufs(point_list=dev(torch.zeros(D, dtype=torch.int64))), "point_list"), (bufs(depths=dev(torch.ones(N + 1))), "depths"),
                (bufs(depths=None), "depths"), (None, "buffers must be the dict"))
    bad_slopes = (dev(torch.zeros(N, 3)), dev(torch.zeros(N + 1, 2)), torch.zeros(N, 2), dev(torch.zeros(N, 2, dtype=torch.float64)),
                  dev(torch.zeros(N, 4))[:, :2], None)
    # the forward
    for bad_b, what in bad_bufs:
        with pytest.raises(ValueError, match=what):
            pd.render_plane_median_depth(sl, bad_b, H, W)
    for bad in bad_slopes:
        with pytest.raises(ValueError, match="slopes"):
            pd.render_plane_median_depth(bad, bufs(), H, W)
    for h, w in ((H + 16, W), (H, W + 16), (0, W), (H, 0), (float(H), W), (True, W)):
        with pytest.raises(ValueError):
            pd.render_plane_median_depth(sl, bufs(), h, w)
    good = (dev(torch.zeros(H, W)), dev(torch.zeros(H, W, dtype=i32)))
    for bad in (good[0], (good[0],), (good[1], good[0]), (torch.zeros(H, W), good[1]), (good[0], dev(torch.zeros(H, W))),
                (good[0], dev(torch.zeros(H, W, 1, dtype=i32))), (dev(torch.zeros(H, W, dtype=torch.float64)), good[1])):
        with pytest.raises(ValueError, match="out"):
            pd.render_plane_median_depth(sl, bufs(), H, W, out=bad)
    with pytest.raises(AssertionError, match="library was touched"):            # valid arguments pass the checks
        pd.render_plane_median_depth(sl, bufs(), H, W)
    with pytest.raises(AssertionError, match="library was touched"):
        pd.render_plane_median_depth(sl, bufs(), H, W, out=good, use_block_masks=False)
    # the backward
    for bad_b, what in bad_bufs:
        with pytest.raises(ValueError, match=what):
            pd.plane_median_depth_backward(g, contrib, sl, bad_b, H, W)
    for bad in bad_slopes:
        with pytest.raises(ValueError, match="slopes"):
            pd.plane_median_depth_backward(g, contrib, bad, bufs(), H, W)
    for bad in (dev(torch.zeros(W, H)), torch.zeros(H, W), dev(torch.zeros(H, W, dtype=torch.float64)), dev(torch.zeros(H, 2 * W))[:, :W], None):
        with pytest.raises(ValueError, match="dL_dmedian"):
            pd.plane_median_depth_backward(bad, contrib, sl, bufs(), H, W)
    for bad in (dev(torch.zeros(H, W)), torch.zeros(H, W, dtype=i32), dev(torch.zeros(W, H, dtype=i32)), dev(torch.zeros(H, W, dtype=torch.int64)), None):
        with pytest.raises(ValueError, match="contrib"):
            pd.plane_median_depth_backward(g, bad, sl, bufs(), H, W)
    for bad in (dev(torch.zeros(N, 2)), torch.zeros(N, 3), dev(torch.zeros(N + 1, 3)), dev(torch.zeros(N, 3, dtype=torch.float64))):
        with pytest.raises(ValueError, match="out"):
            pd.plane_median_depth_backward(g, contrib, sl, bufs(), H, W, out=bad)
    with pytest.raises(ValueError, match="accumulate=True needs out"):
        pd.plane_median_depth_backward(g, contrib, sl, bufs(), H, W, accumulate=True)
    seeded = dev(torch.ones(N, 3))
    with pytest.raises(AssertionError, match="library was touched"):
        pd.plane_median_depth_backward(g, contrib, sl, bufs(), H, W, out=seeded, accumulate=True)
    assert bool((seeded == 1).all())                                            # accumulate=True: not cleared
    with pytest.raises(AssertionError, match="library was touched"):
        pd.plane_median_depth_backward(g, contrib, sl, bufs(), H, W, out=seeded)
    assert not bool(seeded.any())                                               # the default clears first
    # plane_median_gradients: grads is a backward_view result or None
    cam = {"world_to_camera": torch.eye(4), "tan_fovx": 0.5, "tan_fovy": 0.4, "width": W, "height": H}
    P = {"positions": dev(torch.zeros(N, 3)), "scales": dev(torch.ones(N, 3)), "rotations": dev(torch.zeros(N, 4))}
    for bad in ({}, {"dL_dmean3D": seeded}, [seeded, seeded]):
        with pytest.raises(ValueError, match="grads must be a backward_view"):
            pd.plane_median_gradients(P, cam, bufs(), g, contrib, sl, P["positions"], grads=bad)
    # fuse_views: the new value of plane_depth, the old refusals
    params = {"positions": P["positions"], "scales": P["scales"], "rotations": P["rotations"]}
    with pytest.raises(ValueError, match="at least one camera"):                # accepted: the next check is the cameras'
        tsdf.fuse_views(None, [], plane_depth="median", params=params)
    with pytest.raises(ValueError, match="needs params"):
        tsdf.fuse_views(None, [], plane_depth="median")
    for pdv in ("median", True):
        with pytest.raises(ValueError, match="plane_depth='median'"):           # depth_mode stays the centre-depth axis; the message points on
            tsdf.fuse_views(None, [], depth_mode="median", plane_depth=pdv, params=params)
    with pytest.raises(ValueError, match="plane_depth=True"):                   # (what the message said before, still there)
        tsdf.fuse_views(None, [], depth_mode="median", plane_depth=True, params=params)
    for bad in ("mean", "plane", 2, "expected"):
        with pytest.raises(ValueError, match="plane_depth must be"):
            tsdf.fuse_views(None, [], plane_depth=bad, params=params)
    with pytest.raises(ValueError, match="depth_mode"):
        tsdf.fuse_views(None, [], depth_mode="plane-median")


@pytest.mark.parametrize("script,flags,bad", [
    ("examples/train.py", ("--mesh-depth", "--depth-render", "plane-median"), (["--depth-render", "plane-mean"], ["--mesh-depth", "median-plane"])),
    ("examples/extract_mesh.py", ("--depth-mode", "plane-median"), (["--depth-mode", "plane-mean"],)),
    ("examples/eval_mesh.py", ("--depth-mode", "--demo-flat", "plane-median"), (["--depth-mode", "plane-mean"],)),
    ("tools/plane_median_bench.py", ("--config", "--repeats", "--flatten"), (["--config", "C9"],)),
])
def test_tools_parse_the_plane_median_flags(script, flags, bad):
    path = os.path.join(ROOT, script)
    p = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in flags:
        assert flag in p.stdout, flag
    for args in bad:
        p = subprocess.run([sys.executable, path] + list(args), capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and "invalid choice" in p.stderr, p.stderr[-500:]
    if script == "examples/train.py":                                                  # --depth-render plane-median wants the L1, as median does
        p = subprocess.run([sys.executable, path, "--depth-render", "plane-median", "--depth-loss", "pearson", "--lambda-depth", "1"], capture_output=True,
                           text=True, timeout=300)
        assert p.returncode != 0 and "--depth-render plane-median needs --depth-loss l1" in p.stderr + p.stdout, (p.stderr + p.stdout)[-800:]
