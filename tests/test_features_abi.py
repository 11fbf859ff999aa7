"""CPU-side checks of the feature-rendering stage's C ABI and Python surface (include/gsr_features.h): the header is plain C99, the
library exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented order before
anything is enqueued, the Python validators raise before the library is touched, and the example parses its flags.  The stage needs
no workspace: there is no gsr_features_workspace_bytes, which the header says and the name check holds."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import A, OnDevice, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_features.h")
NAMES = {"gsr_features_forward", "gsr_features_backward"}


def test_features_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include <stddef.h>\n#include "gsr_features.h"\n'
                                'typedef char most[GSR_FEATURES_MAX_CHANNELS == 64 ? 1 : -1];\n'
                                'typedef char side[GSR_FEATURES_MAX_SIDE == 32768 ? 1 : -1];\n'
                                'typedef char first[offsetof(GsrFeaturesFrame, W) == 0 && offsetof(GsrFeaturesFrame, N) == 8 ? 1 : -1];\n'
                                'typedef char size[sizeof(GsrFeaturesFrame) == 88 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  int (*f)(const GsrFeaturesFrame *, int32_t, const float *, float *, void *) = gsr_features_forward;\n'
                                '  int (*b)(const GsrFeaturesFrame *, int32_t, const float *, float *, void *) = gsr_features_backward;\n'
                                '  (void)f; (void)b; return 0; }\n')


def test_features_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.FEATURES_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "FEATURES_EXPORTS"]
    assert len(tables) >= 13                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_features.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "features" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_features" in ln} == declared   # exactly the declared names
    hdr = open(HDR).read()
    assert f"#define GSR_FEATURES_MAX_CHANNELS {_lib.FEATURES_MAX_CHANNELS}\n" in hdr
    assert f"#define GSR_FEATURES_MAX_SIDE {_lib.FEATURES_MAX_SIDE}\n" in hdr
    assert C.sizeof(_lib.GsrFeaturesFrame) == 88
    assert [f[0] for f in _lib.GsrFeaturesFrame._fields_] == ["W", "H", "N", "D", "xy", "xy_stride", "conic_opacity", "conic_opacity_stride",
                                                             "point_list", "ranges", "n_contrib", "block_masks"]
    for word in ("W, H", "int64_t N;", "int64_t D;", "xy_stride", "conic_opacity_stride", "point_list", "ranges", "n_contrib", "block_masks",
                 "may differ from run to run", "No workspace is"):
        assert word in hdr, word


def test_features_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN, in
    that order, for both entry points."""
    _lib = sub("_lib")
    L = _lib.lib()

    def frame(**kw):
        f = dict(W=40, H=30, N=100, D=500, xy=A, xy_stride=16, conic_opacity=A + 8, conic_opacity_stride=16, point_list=A, ranges=A, n_contrib=A,
                 block_masks=None)
        f.update(kw)
        return _lib.GsrFeaturesFrame(*(f[k] for k, _ in _lib.GsrFeaturesFrame._fields_))

    for entry in (L.gsr_features_forward, L.gsr_features_backward):
        def call(c=16, a=A, b=A, fr=True, **kw):
            return entry(C.byref(frame(**kw)) if fr else None, c, a, b, None)

        assert call(fr=False) == _lib.GSR_E_NULL
        for k in ("xy", "conic_opacity", "ranges", "n_contrib", "point_list"):
            assert call(**{k: None}) == _lib.GSR_E_NULL, k
            assert call(**{k: None}, c=0, a=A + 4) == call(**{k: None}, W=0) == _lib.GSR_E_NULL, k      # NULL before everything else
        for k in ("a", "b"):
            assert call(**{k: None}) == call(**{k: None}, c=65) == _lib.GSR_E_NULL, k
        bad_dims = [dict(W=0), dict(H=0), dict(W=-1), dict(W=32769), dict(H=32769), dict(N=0), dict(N=1 << 31), dict(D=-1), dict(D=(1 << 30) + 1),
                    dict(xy_stride=1), dict(conic_opacity_stride=3), dict(c=0), dict(c=-1), dict(c=65)]
        for kw in bad_dims:
            assert call(**kw) == _lib.GSR_E_DIMS, kw
            assert call(**kw, a=A + 4) == call(**kw, ranges=A + 2) == _lib.GSR_E_DIMS, kw              # ... before alignment
        for k in ("xy", "conic_opacity", "point_list", "ranges", "n_contrib"):
            assert call(**{k: A + 2}) == call(**{k: A + 1}) == _lib.GSR_E_ALIGN, k
        for k in ("a", "b"):
            assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, k
        assert call(point_list=None, D=0, c=0) == _lib.GSR_E_DIMS                                      # (a frame with D = 0 needs no list)


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, feat = sub("_lib"), sub("features")
    assert list(inspect.signature(feat.render_features).parameters) == ["features", "buffers", "image_height", "image_width", "out", "use_block_masks"]
    assert list(inspect.signature(feat.render_features_backward).parameters) == ["dL_dout", "buffers", "image_height", "image_width", "out",
                                                                                 "use_block_masks"]
    assert list(inspect.signature(feat.rasterize_features).parameters) == ["features", "buffers", "image_height", "image_width"]

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
             "ranges": dev(torch.zeros(tiles, 2, dtype=i32)), "n_contrib": dev(torch.zeros(H, W, dtype=i32))}
        b.update(kw)
        return b
    F, G = dev(torch.zeros(N, 5)), dev(torch.zeros(H, W, 5))
    calls = ((feat.render_features, F, "features"), (feat.render_features_backward, G, "dL_dout"), (feat.rasterize_features, F, "features"))
    for f, x, name in calls:
        shape = tuple(x.shape)
        for bad, what in ((np.zeros(shape, np.float32), "float32 device tensor"), (torch.zeros(shape), "float32 device tensor"),
                          (dev(torch.zeros(shape, dtype=torch.float64)), "float32 device tensor"), (dev(torch.zeros(shape[:-1])), "of shape"),
                          (dev(torch.zeros((shape[0] + 1,) + shape[1:])), "of shape"), (dev(torch.zeros(shape[:-1] + (0,))), "channels"),
                          (dev(torch.zeros(shape[:-1] + (65,))), "channels"), (dev(torch.zeros(shape[:-1] + (10,))[..., ::2]), "contiguous")):
            with pytest.raises(ValueError, match=name + ".*" + what):
                f(bad, bufs(), H, W)
        for bad_b, what in ((bufs(ranges=dev(torch.zeros(tiles + 1, 2, dtype=i32))), "ranges"), (bufs(ranges=dev(torch.zeros(tiles, 2))), "ranges"),
                            (bufs(n_contrib=dev(torch.zeros(H, W + 1, dtype=i32))), "n_contrib"), (bufs(n_contrib=dev(torch.zeros(W, H, dtype=i32))), "n_contrib"),
                            (bufs(n_contrib=torch.zeros(H, W, dtype=i32)), "n_contrib"), (bufs(point_list=dev(torch.zeros(D, dtype=torch.int64))), "point_list"),
                            (bufs(point_list=dev(torch.zeros(2 * D, dtype=i32))[::2]), "point_list"), (bufs(points_xy_image=dev(torch.zeros(N, 3))), "points_xy_image"),
                            (bufs(points_xy_image=dev(torch.zeros(2, N)).t()), "points_xy_image"), (bufs(conic_opacity=dev(torch.zeros(N + 1, 4))), "disagree"),
                            (bufs(conic_opacity=dev(torch.zeros(N, 4, dtype=torch.float64))), "conic_opacity"), ({"ranges": None}, "buffers must be the dict"),
                            (None, "buffers must be the dict")):
            with pytest.raises(ValueError, match=what):
                f(x, bad_b, H, W)
        for h, w in ((H + 16, W), (H, W + 16), (0, W), (H, 0), (H, 1 << 20), (float(H), W), (True, W)):
            with pytest.raises(ValueError):
                f(x, bufs(), h, w)
        with pytest.raises(AssertionError, match="library was touched"):        # valid arguments pass the checks
            f(x, bufs(), H, W)
        packed = bufs(points_xy_image=dev(torch.zeros(N, 2)), conic_opacity=dev(torch.zeros(N, 4)))
        with pytest.raises(AssertionError, match="library was touched"):        # ... and so do packed arrays
            f(x, packed, H, W)
    wrong_n = dev(torch.zeros(N + 1, 5))
    with pytest.raises(ValueError, match="features.*of shape"):
        feat.render_features(wrong_n, bufs(), H, W)
    for f, x, shape in ((feat.render_features, F, (H, W, 5)), (feat.render_features_backward, G, (N, 5))):
        for bad in (torch.zeros(shape), dev(torch.zeros(shape, dtype=torch.float64)), dev(torch.zeros(shape[:-1] + (4,))), dev(torch.zeros(shape[:-1] + (10,))[..., ::2]),
                    np.zeros(shape, np.float32)):
            with pytest.raises(ValueError, match="out must be"):
                f(x, bufs(), H, W, out=bad)
        with pytest.raises(AssertionError, match="library was touched"):
            f(x, bufs(), H, W, out=dev(torch.zeros(shape)))


def test_fit_features_example_parses_its_flags():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_features.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--size", "--iterations", "--out", "--gaussians", "--lr", "--seed"):
        assert flag in p.stdout, flag
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_features.py"), "--iterations", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--iterations must be at least 1" in p.stderr
