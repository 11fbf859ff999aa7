"""CPU-side checks of exposure compensation's C ABI and Python surface (include/gsr_exposure.h): the header is plain C99, the library
exports what it declares and _lib binds it in a table of its own, every argument of each entry point is refused in the documented
order before anything is enqueued, the Python validators raise before the library is touched, and the trainer parses its flags and
refuses the two combinations that are out of scope."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import A, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_exposure.h")
NAMES = {"gsr_exposure_workspace_bytes", "gsr_exposure_apply", "gsr_exposure_backward", "gsr_exposure_adam"}


def test_exposure_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_exposure.h"\n'
                                'typedef char twelve[GSR_EXPOSURE_FLOATS == 12 ? 1 : -1];\n'
                                'typedef char record[GSR_EXPOSURE_RECORD_BYTES >= 4 * GSR_EXPOSURE_FLOATS && GSR_EXPOSURE_RECORD_BYTES % 16 == 0 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  size_t (*w)(int32_t, int32_t) = gsr_exposure_workspace_bytes;\n'
                                '  int (*a)(const float *, const float *, float *, int32_t, int32_t, void *) = gsr_exposure_apply;\n'
                                '  int (*b)(const float *, const float *, const float *, float *, float *, int32_t, int32_t, void *, size_t, void *) =\n'
                                '      gsr_exposure_backward;\n'
                                '  int (*c)(float *, const float *, float *, float *, float, float, float, float, int32_t, void *) = gsr_exposure_adam;\n'
                                '  int n = GSR_EXPOSURE_BLOCK_PIXELS + GSR_EXPOSURE_MAX_BLOCKS;\n'
                                '  (void)w; (void)a; (void)b; (void)c; (void)n; return 0; }\n')


def test_exposure_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.EXPOSURE_EXPORTS) == declared
    for other in (_lib.EXPORTS, _lib.CAPACITY_EXPORTS, _lib.LOSS_EXPORTS, _lib.AUX_EXPORTS, _lib.CAMERA_EXPORTS, _lib.DENSIFY_STATS_EXPORTS,
                  _lib.ANTIALIAS_EXPORTS, _lib.FILTER3D_EXPORTS):
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_exposure.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "exposure" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_exposure" in ln} == declared      # exactly the declared names
    hdr = open(HDR).read()
    for macro, value in (("GSR_EXPOSURE_FLOATS", _lib.EXPOSURE_FLOATS), ("GSR_EXPOSURE_BLOCK_PIXELS", _lib.EXPOSURE_BLOCK_PIXELS),
                         ("GSR_EXPOSURE_MAX_BLOCKS", _lib.EXPOSURE_MAX_BLOCKS), ("GSR_EXPOSURE_RECORD_BYTES", _lib.EXPOSURE_RECORD_BYTES)):
        assert f"#define {macro} {value} " in hdr, macro
    assert sub("exposure") is getattr(__import__("importlib").import_module("3dgs-native_amd"), "exposure")


def test_exposure_workspace_bytes_follow_the_stated_grid(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    bp, mb, rb = _lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS, _lib.EXPOSURE_RECORD_BYTES
    for W, H in ((1, 1), (67, 33), (800, 800), (1920, 1080), (1 << 14, 1 << 14)):
        records = min(-(-W * H // bp), mb)
        assert int(L.gsr_exposure_workspace_bytes(W, H)) == -(-rb * records // 256) * 256, (W, H)
    for W, H in ((0, 5), (5, 0), (-1, 5), (1 << 14, (1 << 14) + 1)):
        assert int(L.gsr_exposure_workspace_bytes(W, H)) == 0, (W, H)


def test_exposure_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN,
    GSR_E_WORKSPACE, in that order."""
    _lib = sub("_lib")
    L = _lib.lib()
    W, H = 67, 33
    wsb = int(L.gsr_exposure_workspace_bytes(W, H))
    assert wsb > 0 and wsb % 16 == 0
    bad_dims = (dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 14, h=(1 << 14) + 1))

    def ap(r=A, e=A + 4, o=A, w=W, h=H):
        return L.gsr_exposure_apply(r, e, o, w, h, None)

    for k in ("r", "e", "o"):
        assert ap(**{k: None}) == _lib.GSR_E_NULL, k
        assert ap(**{k: None}, w=0) == _lib.GSR_E_NULL, k                         # NULL before the dimensions
    for bad in bad_dims:
        assert ap(**bad) == _lib.GSR_E_DIMS, bad
        assert ap(**bad, r=A + 4) == _lib.GSR_E_DIMS, bad                         # ... before alignment
    for k in ("r", "o"):
        assert ap(**{k: A + 4}) == ap(**{k: A + 8}) == _lib.GSR_E_ALIGN, k        # images: 16 bytes
    assert ap(e=A + 2) == ap(e=A + 1) == _lib.GSR_E_ALIGN                         # the 12 floats: 4 bytes (a row of a (V, 12) tensor)

    def bw(r=A, e=A + 4, g=A, d=A, de=A + 8, w=W, h=H, ws=A, b=wsb):
        return L.gsr_exposure_backward(r, e, g, d, de, w, h, ws, b, None)

    for k in ("r", "e", "g", "de", "ws"):
        assert bw(**{k: None}) == _lib.GSR_E_NULL, k
        assert bw(**{k: None}, w=0, b=0) == _lib.GSR_E_NULL, k
    for bad in bad_dims:
        assert bw(**bad) == _lib.GSR_E_DIMS, bad
        assert bw(**bad, g=A + 4, b=0) == bw(**bad, d=None) == _lib.GSR_E_DIMS, bad
    for k in ("r", "g", "d", "ws"):
        assert bw(**{k: A + 4}) == _lib.GSR_E_ALIGN, k
        assert bw(**{k: A + 4}, b=wsb - 1) == _lib.GSR_E_ALIGN, k                 # alignment before the workspace
    assert bw(e=A + 2) == bw(de=A + 3) == _lib.GSR_E_ALIGN
    assert bw(b=wsb - 1) == bw(b=0) == bw(d=None, b=wsb - 1) == _lib.GSR_E_WORKSPACE   # (dL_drendered may be NULL: not an error)

    def ad(e=A + 4, g=A + 8, m=A + 12, v=A, lr=0.01, b1=0.9, b2=0.999, eps=1e-15, step=1):
        return L.gsr_exposure_adam(e, g, m, v, lr, b1, b2, eps, step, None)

    for k in ("e", "g", "m", "v"):
        assert ad(**{k: None}) == _lib.GSR_E_NULL, k
        assert ad(**{k: None}, step=0) == _lib.GSR_E_NULL, k
    inf, nan = float("inf"), float("nan")
    for bad in (dict(step=0), dict(step=-1), dict(lr=-1e-3), dict(lr=inf), dict(lr=nan), dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0),
                dict(b2=-0.1), dict(b2=nan), dict(eps=0.0), dict(eps=-1e-15), dict(eps=inf), dict(eps=nan)):
        assert ad(**bad) == _lib.GSR_E_DIMS, bad
        assert ad(**bad, e=A + 2) == _lib.GSR_E_DIMS, bad                         # ... before alignment
    for k in ("e", "g", "m", "v"):
        assert ad(**{k: A + 2}) == _lib.GSR_E_ALIGN, k


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, X, forward, backward = sub("_lib"), sub("exposure"), sub("forward"), sub("backward")
    for fn in (forward.render_gaussians, backward.backward):
        assert not [p for p in inspect.signature(fn).parameters if "exposure" in p]      # an image-space stage: no new keyword

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    img, E = np.zeros((5, 7, 3), np.float32), np.asarray(X.IDENTITY, np.float32)
    for bad, msg in ((np.zeros((5, 7), np.float32), "shape"), (np.zeros((5, 7, 4), np.float32), "shape"), (np.zeros((0, 7, 3), np.float32), "shape"),
                     (np.zeros((5, 7, 3), np.float64), "float32"), (torch.zeros(5, 7, 3, dtype=torch.float16), "float32"), ([[[0.0] * 3]], "tensor or a numpy")):
        with pytest.raises(ValueError, match=msg):
            X.apply_exposure(bad, E)
        with pytest.raises(ValueError, match=msg):
            X.exposure_backward(bad, E, img)
    with pytest.raises(ValueError, match="image's shape"):
        X.exposure_backward(img, E, np.zeros((7, 5, 3), np.float32))
    with pytest.raises(ValueError, match="dL_dout must be float32"):
        X.exposure_backward(img, E, np.zeros((5, 7, 3), np.float64))
    for bad, msg in ((np.zeros(9, np.float32), "12 elements"), (np.zeros((3, 4, 2), np.float32), "12 elements"), (np.zeros(12, np.float64), "float32"),
                     (list(X.IDENTITY), "tensor or a numpy")):
        with pytest.raises(ValueError, match=msg):
            X.apply_exposure(img, bad)
        with pytest.raises(ValueError, match=msg):
            X.exposure_backward(img, bad, img)
    with pytest.raises(ValueError, match="out must be a contiguous"):
        X.apply_exposure(img, E, out=torch.zeros(5, 7, 3))                               # not on the device
    with pytest.raises(ValueError, match="out must be a contiguous"):
        X.exposure_backward(img, E, img, out=img)
    with pytest.raises(ValueError, match="want_image_grad=False"):
        X.exposure_backward(img, E, img, out=img, want_image_grad=False)
    with pytest.raises(ValueError, match="dE_out must be"):
        X.exposure_backward(img, E, img, dE_out=torch.zeros(12))

    class OnDevice(torch.Tensor):
        is_cuda = True
    on = lambda t, d: type("T", (OnDevice,), {"device": torch.device("cuda", d)})
    a, b = torch.zeros(5, 7, 3).as_subclass(on(None, 0)), torch.zeros(5, 7, 3).as_subclass(on(None, 1))
    with pytest.raises(ValueError, match="one device"):
        X.exposure_backward(a, E, b)
    with pytest.raises(AssertionError, match="library was touched"):
        X.apply_exposure(img, E)                                                         # valid arguments pass the checks
    with pytest.raises(AssertionError, match="library was touched"):
        X.exposure_backward(img, E.reshape(4, 3), img)
    with pytest.raises(ValueError, match="num_views"):
        X.ExposureModel(0, "cpu")
    assert (X.BETA1, X.BETA2, X.EPS) == (0.9, 0.999, 1e-15)


def _train(*extra, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, **(env or {})))


def test_trainer_parses_the_exposure_flags_and_refuses_the_two_combinations():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--optimize-exposure", "--exposure-lr-init", "--exposure-lr-final", "--exposure-noise", "--exposure-seed"):
        assert flag in p.stdout, flag
    p = _train("--optimize-exposure", "--gpus", "2")
    assert p.returncode != 0 and "--optimize-exposure trains on one GPU only" in p.stderr
    p = _train("--optimize-exposure", env={"WORLD_SIZE": "2"})
    assert p.returncode != 0 and "--optimize-exposure trains on one GPU only" in p.stderr
    p = _train("--optimize-exposure", "--capacity")
    assert p.returncode != 0 and "--optimize-exposure does not combine with --capacity" in p.stderr
    p = _train("--exposure-noise", "-0.1")
    assert p.returncode != 0 and "--exposure-noise must be >= 0" in p.stderr
    p = _train("--optimize-exposure", "--exposure-lr-init", "0")
    assert p.returncode != 0 and "--exposure-lr-init and --exposure-lr-final must be positive" in p.stderr
    # valid values are parsed before the other arguments are judged: the refusal below is theirs
    p = _train("--optimize-exposure", "--exposure-lr-init", "0.02", "--exposure-lr-final", "0.002", "--exposure-noise", "0.2", "--exposure-seed", "3",
               "--lambda-dssim", "2")
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr
