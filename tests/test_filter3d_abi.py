"""CPU-side checks of the 3D smoothing filter's C ABI and Python surface (include/gsr_filter3d.h): the header is plain C99, the
library exports what it declares and _lib binds it, every argument of each entry point is refused in the documented order before
anything is enqueued, `filter_3d` is validated before the library is touched, backward() refuses an unfiltered or stale frame, and
the trainer parses its flags."""
import ctypes as C
import inspect
import os
import subprocess
import sys
import weakref

import numpy as np
import pytest
import torch

from abi_helpers import A, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_filter3d.h")
NAMES = {"gsr_filter3d_workspace_bytes", "gsr_filter3d_from_views", "gsr_filter3d_apply", "gsr_filter3d_backward"}


def test_filter3d_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_filter3d.h"\n'
                                'typedef char view_is_80_bytes[sizeof(GsrFilterView) == 80 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  float v = GSR_FILTER3D_VARIANCE, m = GSR_FILTER3D_MARGIN;\n'
                                '  size_t (*w)(int64_t) = gsr_filter3d_workspace_bytes;\n'
                                '  int (*a)(int64_t, const float *, int32_t, const GsrFilterView *, float, float *, void *, size_t, void *) = gsr_filter3d_from_views;\n'
                                '  int (*b)(int64_t, const float *, const float *, const float *, float *, float *, void *) = gsr_filter3d_apply;\n'
                                '  int (*c)(int64_t, const float *, const float *, const float *, const float *, const float *, float *, float *, void *) =\n'
                                '      gsr_filter3d_backward;\n'
                                '  (void)v; (void)m; (void)w; (void)a; (void)b; (void)c; return 0; }\n')


def test_filter3d_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.FILTER3D_EXPORTS) == declared
    for other in (_lib.EXPORTS, _lib.CAPACITY_EXPORTS, _lib.LOSS_EXPORTS, _lib.AUX_EXPORTS, _lib.CAMERA_EXPORTS, _lib.DENSIFY_STATS_EXPORTS,
                  _lib.ANTIALIAS_EXPORTS):
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_filter3d.h" in doc and "filter_3d" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "filter_3d" not in gsr_h and "filter3d" not in gsr_h and "GsrFilterView" not in gsr_h
    assert _lib.lib().gsr_abi_version() == 7
    assert C.sizeof(_lib.GsrFilterView) == 80
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_filter3d" in ln} == declared      # exactly the declared names


def test_filter3d_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake 16-byte-aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS,
    (N = 0: GSR_OK), GSR_E_ALIGN, GSR_E_WORKSPACE."""
    _lib = sub("_lib")
    L = _lib.lib()
    N, V = 8, 3
    wsb = int(L.gsr_filter3d_workspace_bytes(N))
    assert wsb > 0 and wsb % 16 == 0

    def fv(n=N, means=A, v=V, views=A, var=0.2, out=A, ws=A, b=wsb):
        return L.gsr_filter3d_from_views(n, means, v, views, var, out, ws, b, None)

    assert fv(means=None) == fv(out=None) == fv(views=None) == _lib.GSR_E_NULL
    assert fv(means=None, n=-1) == _lib.GSR_E_DIMS                           # (no array is asked of a call without Gaussians)
    assert fv(means=None, v=-1) == fv(means=None, var=0.0) == _lib.GSR_E_NULL   # NULL before the dimensions
    for bad in (dict(n=-1), dict(v=-1), dict(var=0.0), dict(var=-1.0), dict(var=float("inf")), dict(var=float("nan")), dict(n=1 << 31)):
        assert fv(**bad) == _lib.GSR_E_DIMS, bad
        assert fv(**bad, means=A + 4) == fv(**bad, b=0) == _lib.GSR_E_DIMS   # ... before alignment and workspace
    for k in ("means", "views", "out", "ws"):
        assert fv(**{k: A + 4}) == _lib.GSR_E_ALIGN, k
        assert fv(**{k: A + 4}, b=wsb - 1) == _lib.GSR_E_ALIGN              # alignment before the workspace
    assert fv(ws=None) == fv(b=wsb - 1) == fv(b=0) == _lib.GSR_E_WORKSPACE
    assert fv(v=0, views=None, b=0) == _lib.GSR_E_WORKSPACE                  # V = 0 needs no records, but is a real call
    assert fv(n=0, means=None, views=None, out=None, ws=None, b=0) == _lib.GSR_OK
    assert fv(n=0, means=A + 4) == _lib.GSR_OK                               # N = 0: nothing is looked at

    def ap(n=N, s=A, o=A, f=A, so=A, oo=A):
        return L.gsr_filter3d_apply(n, s, o, f, so, oo, None)

    def bw(n=N, s=A, o=A, f=A, gs=A, go=A, ds=A, do=A):
        return L.gsr_filter3d_backward(n, s, o, f, gs, go, ds, do, None)

    for fn, keys in ((ap, ("s", "o", "f", "so", "oo")), (bw, ("s", "o", "f", "gs", "go", "ds", "do"))):
        for k in keys:
            assert fn(**{k: None}) == _lib.GSR_E_NULL, k
            assert fn(**{k: A + 8}) == _lib.GSR_E_ALIGN, k
            assert fn(**{k: A + 8}, n=-1) == _lib.GSR_E_DIMS, k
        assert fn(n=-1) == fn(n=1 << 31) == _lib.GSR_E_DIMS
        assert fn(n=0, **{k: None for k in keys}) == _lib.GSR_OK
    assert ap(s=None, f=A + 4) == _lib.GSR_E_NULL


def test_filter_3d_is_validated_before_the_library_is_touched(monkeypatch):
    _lib, forward, backward, filter3d = sub("_lib"), sub("forward"), sub("backward"), sub("filter3d")
    for fn in (forward.render_gaussians, backward.backward):
        p = inspect.signature(fn).parameters["filter_3d"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert inspect.signature(sub("point_cloud").save_ply).parameters["filter_3d"].default is None

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    z, bg, dpix = np.zeros((4, 3), np.float32), np.zeros(3, np.float32), np.zeros((8, 8, 3), np.float32)
    bad = {"a torch tensor": np.zeros(4, np.float32), "float32": torch.zeros(4, dtype=torch.float64), "on the GPU": torch.zeros(4)}
    for msg, f in bad.items():
        with pytest.raises(ValueError, match="filter_3d must .*" + msg):
            forward.render_gaussians(bg, z, filter_3d=f)
        with pytest.raises(ValueError, match="filter_3d must .*" + msg):
            backward.backward(bg, z, dpix, filter_3d=f)
    # shape, packing and alignment: judged on a stand-in that claims to be a device tensor (there is no GPU here)
    class OnDevice(torch.Tensor):
        is_cuda = True
    dev = lambda t: t.as_subclass(OnDevice)
    for f, msg in ((dev(torch.zeros(5)), "shape"), (dev(torch.zeros(4, 1)), "shape"), (dev(torch.zeros(8)[::2]), "contiguous"),
                   (dev(torch.zeros(8)[1:5]), "aligned")):
        with pytest.raises(ValueError, match=msg):
            filter3d.check_filter_3d(f, z)
        with pytest.raises(ValueError, match=msg):
            forward.render_gaussians(bg, z, filter_3d=f)
    with pytest.raises(AssertionError, match="library was touched"):
        forward.render_gaussians(bg, z, filter_3d=dev(torch.zeros(4)))          # a valid filter passes the checks
    with pytest.raises(AssertionError, match="library was touched"):
        forward.render_gaussians(bg, z)                                         # None is today's call


def test_backward_refuses_an_unfiltered_or_stale_frame(monkeypatch):
    """States that Python can see and C cannot: a frame rendered without the filter, with another filter tensor, a filter or raw
    parameters written since the render, and a filtered frame handed to the plain backward.  Each raises before the library or
    the GPU is touched."""
    _lib, backward, filter3d = sub("_lib"), sub("backward"), sub("filter3d")

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)

    class OnDevice(torch.Tensor):
        is_cuda = True
    N = 8
    z, bg, dpix = np.zeros((N, 3), np.float32), np.zeros(3, np.float32), np.zeros((8, 8, 3), np.float32)
    f = torch.full((N,), 0.01).as_subclass(OnDevice)
    records = torch.zeros(N, 16)
    co, sc, op = records[:, 2:6], torch.full((N, 3), 0.1), torch.full((N,), 0.5)
    call = lambda flt, **kw: backward.backward(bg, z, dpix, opacity=kw.pop("op", op), scales=kw.pop("sc", sc), conic_opacity=co, filter_3d=flt, **kw)
    with pytest.raises(ValueError, match="not an unfiltered frame"):
        call(f)                                                                # rendered without the filter: no tag
    filter3d.tag_frame(co, f, sc, sc, op, op, sc.clone(), op.clone())
    with pytest.raises(ValueError, match="pass the same tensor"):
        call(None)                                                             # a filtered frame, plain backward
    with pytest.raises(ValueError, match="another filter tensor"):
        call(f.clone().as_subclass(OnDevice))
    with pytest.raises(ValueError, match="`scales` is not the raw tensor"):
        call(f, sc=sc.clone())
    with pytest.raises(ValueError, match="`opacity` is not the raw tensor"):
        call(f, op=op.clone())
    with pytest.raises(AssertionError, match="library was touched"):
        call(f)                                                                # the valid tag passes the checks
    sc.mul_(0.5)
    with pytest.raises(ValueError, match="`scales` is not the raw tensor .* written in place since"):
        call(f)                                                                # scales written in place since the forward
    filter3d.tag_frame(co, f, sc, sc, op, op, sc.clone(), op.clone())
    f.mul_(2.0)
    with pytest.raises(ValueError, match="filter_3d was written in place"):
        call(f)
    filter3d.tag_frame(co, f, sc, sc, op, op, sc.clone(), op.clone())
    records[0, 0] = 1.0
    with pytest.raises(ValueError, match="records were written in place"):
        call(f)
    assert weakref.ref(f)() is f


def _train(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_the_filter_flags_and_refuses_a_scale_that_does_not_divide():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--filter-3d", "--filter-3d-variance", "--filter-3d-interval", "--eval-scales"):
        assert flag in p.stdout, flag
    p = _train("--filter-3d", "--filter-3d-variance", "0")
    assert p.returncode != 0 and "--filter-3d-variance must be positive" in p.stderr
    p = _train("--filter-3d", "--filter-3d-interval", "0")
    assert p.returncode != 0 and "--filter-3d-interval >= 1" in p.stderr
    p = _train("--size", "100", "--eval-scales", "1,2,3")
    assert p.returncode != 0 and "3 does not divide the 100 x 100 image" in p.stderr
    p = _train("--size", "100", "--eval-scales", "1,two")
    assert p.returncode != 0 and "--eval-scales takes integers" in p.stderr
    # valid values are parsed before the other arguments are judged: the refusal below is theirs
    p = _train("--filter-3d", "--filter-3d-interval", "50", "--size", "100", "--eval-scales", "1,2,4", "--lambda-dssim", "2")
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr
