"""CPU-side checks of the median-depth stage's C ABI and Python surface (include/gsr_median_depth.h): the header is plain C99, the
library exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented order before
anything is enqueued, the Python validators raise before the library is touched, and the tools parse their flags."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest
import torch

from abi_helpers import A, OnDevice, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, pkg, sub

HDR = os.path.join(ROOT, "include", "gsr_median_depth.h")
NAMES = {"gsr_median_depth_forward", "gsr_median_depth_backward"}


def test_median_depth_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include <stddef.h>\n#include "gsr_median_depth.h"\n'
                                'typedef char size[sizeof(GsrDistortionFrame) == 104 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  int (*f)(const GsrDistortionFrame *, float *, int32_t *, void *) = gsr_median_depth_forward;\n'
                                '  int (*b)(const GsrDistortionFrame *, const float *, const int32_t *, float *, void *) = gsr_median_depth_backward;\n'
                                '  (void)f; (void)b; return 0; }\n')


def test_median_depth_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.MEDIAN_DEPTH_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "MEDIAN_DEPTH_EXPORTS"]
    assert len(tables) >= 19                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_median_depth.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "median" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "median" in ln} == declared          # exactly the declared names
    hdr = open(HDR).read()
    assert "typedef struct" not in hdr                                                            # the frame is gsr_distortion.h's
    for word in ("GsrDistortionFrame", "T > 0.5f", "the same bits, no arithmetic applied", "n_contrib's convention", "No atomics",
                 "accumulators[id * 16 + 11] += g", "no other column is touched", "pixels 0-31 in order", "may differ from run", "No workspace is",
                 "never an access out of bounds", "GSR_E_NULL", "GSR_E_DIMS", "GSR_E_ALIGN", "GSR_E_HIP"):
        assert word in hdr, word
    assert hdr.index("GSR_E_NULL ") < hdr.index("GSR_E_DIMS ") < hdr.index("GSR_E_ALIGN ") < hdr.index("GSR_E_HIP ")


def test_median_depth_arguments_are_checked_in_order_before_any_hip_call(libpath):
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
        return L.gsr_median_depth_forward(C.byref(frame(**kw)) if fr else None, a, b, None)

    def bwd(a=A, b=A, c=A, fr=True, **kw):
        return L.gsr_median_depth_backward(C.byref(frame(**kw)) if fr else None, a, b, c, None)

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
    _lib, med, tsdf = sub("_lib"), sub("median_depth"), sub("tsdf")
    gsr = pkg()
    assert list(inspect.signature(med.render_median_depth).parameters) == ["buffers", "image_height", "image_width", "out", "use_block_masks"]
    assert list(inspect.signature(med.view_depth).parameters) == ["median_inv_depth", "final_Ts", "alpha_min"]
    assert inspect.signature(med.view_depth).parameters["alpha_min"].default == _lib.NORMALS_ALPHA_MIN
    params = inspect.signature(gsr.backward).parameters
    names = list(params)
    for k in ("dL_dmedian_depth", "median_contributor"):
        assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None
        assert names.index(k) < names.index("rendered_stage")                                          # in front of the catch-all
    assert "median_depth" in gsr.__all__
    assert inspect.signature(tsdf.fuse_views).parameters["depth_mode"].default == "expected" and tsdf.DEPTH_MODES == ("expected", "median")

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
            med.render_median_depth(bad_b, H, W)
    for h, w in ((H + 16, W), (H, W + 16), (0, W), (H, 0), (float(H), W), (True, W)):
        with pytest.raises(ValueError):
            med.render_median_depth(bufs(), h, w)
    good = (dev(torch.zeros(H, W)), dev(torch.zeros(H, W, dtype=i32)))
    for bad in (good[0], (good[0],), (good[1], good[0]), (torch.zeros(H, W), good[1]), (good[0], dev(torch.zeros(H, W))),
                (good[0], dev(torch.zeros(H, W, 1, dtype=i32))), (dev(torch.zeros(H, W, dtype=torch.float64)), good[1])):
        with pytest.raises(ValueError, match="out"):
            med.render_median_depth(bufs(), H, W, out=bad)
    with pytest.raises(AssertionError, match="library was touched"):            # valid arguments pass the checks
        med.render_median_depth(bufs(), H, W)
    with pytest.raises(AssertionError, match="library was touched"):
        med.render_median_depth(bufs(), H, W, out=good, use_block_masks=False)
    # view_depth is plain torch: nothing to touch, but its arguments are judged, and its rule is depth_from_buffers'
    m = torch.tensor([[0.5, 0.25, 0.0, -1.0], [float("nan"), float("inf"), 2.0, 4.0]])
    T = torch.tensor([[0.0, 0.5, 0.0, 0.0], [0.0, 0.0, 0.6, float("nan")]])
    assert med.view_depth(m, T).tolist() == [[2.0, 4.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    assert med.view_depth(m, T, alpha_min=0.3).tolist()[1][2] == 0.5
    for bad in ((m[0], T[0]), (m, T[:1]), (m.double(), T), (m.numpy(), T)):
        with pytest.raises(ValueError, match="median_inv_depth and final_Ts"):
            med.view_depth(*bad)
    with pytest.raises(ValueError, match="alpha_min"):
        med.view_depth(m, T, alpha_min=0.0)
    # backward(): both keywords or neither, refused before anything else is looked at
    for kw in (dict(dL_dmedian_depth=good[0]), dict(median_contributor=good[1])):
        with pytest.raises(ValueError, match="dL_dmedian_depth and median_contributor together"):
            gsr.backward(None, None, None, **kw)
        with pytest.raises(ValueError, match="dL_dmedian_depth and median_contributor together"):
            gsr.backward_view({}, {}, None, {}, None, **kw)
    with pytest.raises(ValueError, match="depth_mode"):
        tsdf.fuse_views(None, [], depth_mode="mean")


@pytest.mark.parametrize("script,flags,bad", [
    ("examples/train.py", ("--mesh-depth", "--depth-render"), (["--depth-render", "mean"], ["--mesh-depth", "mean"])),
    ("examples/extract_mesh.py", ("--depth-mode",), (["--depth-mode", "mean"],)),
    ("examples/eval_mesh.py", ("--depth-mode",), (["--depth-mode", "mean"],)),
    ("tools/median_depth_bench.py", ("--config", "--repeats"), (["--config", "C9"],)),
])
def test_tools_parse_the_median_depth_flags(script, flags, bad):
    path = os.path.join(ROOT, script)
    p = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in flags:
        assert flag in p.stdout, flag
    for args in bad:
        p = subprocess.run([sys.executable, path] + list(args), capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and "invalid choice" in p.stderr, p.stderr[-500:]
