"""CPU-side checks of the Pearson-correlation depth loss's C ABI and Python surface (include/gsr_depth_corr.h): the header is plain C99,
the library exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented order
before anything is enqueued, the Python validators raise before the library is touched, and the trainer parses its flags and refuses
--depth-loss pearson without a depth weight."""
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

HDR = os.path.join(ROOT, "include", "gsr_depth_corr.h")
NAMES = {"gsr_depth_corr_workspace_bytes", "gsr_depth_corr_loss_grad"}


def test_depth_corr_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_depth_corr.h"\n'
                                'typedef char four[GSR_DEPTH_CORR_FIT_FLOATS == 4 ? 1 : -1];\n'
                                'typedef char record[GSR_DEPTH_CORR_RECORD_BYTES >= 6 * 8 && GSR_DEPTH_CORR_RECORD_BYTES % 16 == 0 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  size_t (*w)(int32_t, int32_t) = gsr_depth_corr_workspace_bytes;\n'
                                '  int (*f)(const float *, const float *, const float *, float *, float *, float *, int32_t, int32_t, float, void *, size_t,\n'
                                '           void *) = gsr_depth_corr_loss_grad;\n'
                                '  int n = GSR_DEPTH_CORR_BLOCK_PIXELS + GSR_DEPTH_CORR_MAX_BLOCKS;\n'
                                '  double v = GSR_DEPTH_CORR_MIN_REL_VAR;\n'
                                '  (void)w; (void)f; (void)n; (void)v; return 0; }\n')


def test_depth_corr_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.DEPTH_CORR_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "DEPTH_CORR_EXPORTS"]
    assert len(tables) >= 11                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_depth_corr.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "depth_corr" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_depth_corr" in ln} == declared    # exactly the declared names
    hdr = open(HDR).read()
    for macro, value in (("GSR_DEPTH_CORR_FIT_FLOATS", _lib.DEPTH_CORR_FIT_FLOATS), ("GSR_DEPTH_CORR_BLOCK_PIXELS", _lib.DEPTH_CORR_BLOCK_PIXELS),
                         ("GSR_DEPTH_CORR_MAX_BLOCKS", _lib.DEPTH_CORR_MAX_BLOCKS), ("GSR_DEPTH_CORR_RECORD_BYTES", _lib.DEPTH_CORR_RECORD_BYTES),
                         ("GSR_DEPTH_CORR_MIN_REL_VAR", _lib.DEPTH_CORR_MIN_REL_VAR)):
        assert f"#define {macro} {value} " in hdr, macro
    import depth_corr_reference as R
    import test_depth_corr_reference as T
    assert R.MIN_REL_VAR == _lib.DEPTH_CORR_MIN_REL_VAR                                   # the yardstick's constants are the header's
    assert (T.BP, T.MB) == (_lib.DEPTH_CORR_BLOCK_PIXELS, _lib.DEPTH_CORR_MAX_BLOCKS)


def test_depth_corr_workspace_bytes_follow_the_stated_grid(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    bp, mb, rb = _lib.DEPTH_CORR_BLOCK_PIXELS, _lib.DEPTH_CORR_MAX_BLOCKS, _lib.DEPTH_CORR_RECORD_BYTES
    for W, H in ((1, 1), (37, 29), (800, 800), (1920, 1080), (1 << 14, 1 << 14)):
        records = min(-(-W * H // bp), mb) + 1                                           # + the moments' record
        assert int(L.gsr_depth_corr_workspace_bytes(W, H)) == -(-rb * records // 256) * 256, (W, H)
    for W, H in ((0, 5), (5, 0), (-1, 5), (1 << 14, (1 << 14) + 1)):
        assert int(L.gsr_depth_corr_workspace_bytes(W, H)) == 0, (W, H)


def test_depth_corr_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN,
    GSR_E_WORKSPACE, in that order."""
    _lib = sub("_lib")
    L = _lib.lib()
    W, H = 37, 29
    wsb = int(L.gsr_depth_corr_workspace_bytes(W, H))
    assert wsb > 0 and wsb % 16 == 0
    inf, nan = float("inf"), float("nan")
    bad_dims = (dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 14, h=(1 << 14) + 1), dict(wt=inf), dict(wt=-inf), dict(wt=nan))

    def call(r=A, t=A, m=A, g=A, lo=A + 4, f=A + 8, w=W, h=H, wt=0.5, ws=A, b=wsb):
        return L.gsr_depth_corr_loss_grad(r, t, m, g, lo, f, w, h, wt, ws, b, None)

    for k in ("r", "t", "lo", "ws"):
        assert call(**{k: None}) == _lib.GSR_E_NULL, k
        assert call(**{k: None}, w=0, b=0) == call(**{k: None}, wt=nan) == _lib.GSR_E_NULL, k      # NULL before the dimensions
    for bad in bad_dims:
        assert call(**bad) == _lib.GSR_E_DIMS, bad
        assert call(**bad, r=A + 4, b=0) == call(**bad, m=None, g=None, f=None) == _lib.GSR_E_DIMS, bad   # ... before alignment
    for k in ("r", "t", "m", "g", "ws"):
        assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, k            # images and the workspace: 16 bytes
        assert call(**{k: A + 4}, b=wsb - 1) == _lib.GSR_E_ALIGN, k                       # alignment before the workspace
    assert call(lo=A + 2) == call(f=A + 1) == call(f=A + 2, b=0) == _lib.GSR_E_ALIGN      # loss and fit: 4 bytes (a row of a (V, 4) tensor)
    assert call(b=wsb - 1) == call(b=0) == _lib.GSR_E_WORKSPACE
    assert call(m=None, g=None, f=None, b=wsb - 1) == _lib.GSR_E_WORKSPACE               # (mask, grad and fit may be NULL: not an error)


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, loss, forward, backward = sub("_lib"), sub("loss"), sub("forward"), sub("backward")
    for fn in (forward.render_gaussians, backward.backward):
        assert not [p for p in inspect.signature(fn).parameters if "corr" in p]          # an image-space stage: no new keyword
    assert list(inspect.signature(loss.depth_corr_loss_and_gradients).parameters) == ["rendered", "target", "mask", "weight", "want_grad", "loss_out",
                                                                                      "fit_out"]

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    f = loss.depth_corr_loss_and_gradients
    r = np.zeros((5, 7), np.float32)
    for bad in (np.zeros(35, np.float32), np.zeros((5, 7, 3), np.float32), np.zeros((0, 7), np.float32), np.float32(1.0)):
        with pytest.raises(ValueError, match=r"rendered must have shape \(H, W\)"):
            f(bad, r)
    for bad in (np.zeros((7, 5), np.float32), np.zeros((5, 8), np.float32), torch.zeros(5, 7, 1, 1)):
        with pytest.raises(ValueError, match="target"):
            f(r, bad)
        with pytest.raises(ValueError, match="mask"):
            f(r, r, bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="weight must be finite"):
            f(r, r, weight=bad)
    with pytest.raises(ValueError, match="loss_out must be a 1-element float32 device tensor"):
        f(r, r, loss_out=torch.zeros(1))                                                 # not on the device
    for bad in (torch.zeros(4), np.zeros(4, np.float32), [0.0] * 4):                      # ... nor these
        with pytest.raises(ValueError, match="fit_out must be a contiguous 4-element float32 device tensor"):
            f(r, r, fit_out=bad)

    class OnDevice(torch.Tensor):
        is_cuda = True
    for bad in (torch.zeros(3), torch.zeros(5), torch.zeros(4, dtype=torch.float64), torch.zeros(8)[::2]):
        with pytest.raises(ValueError, match="fit_out must be"):
            f(r, r, fit_out=bad.as_subclass(OnDevice))                                   # "on the device", but not 4 packed float32
    with pytest.raises(AssertionError, match="library was touched"):
        f(r, r)                                                                          # valid arguments pass the checks
    with pytest.raises(AssertionError, match="library was touched"):
        f(r.reshape(5, 7, 1), torch.zeros(5, 7), r, weight=0.0, want_grad=False, fit_out=torch.zeros(4).as_subclass(OnDevice))


def _train(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_the_depth_flags_and_refuses_pearson_without_a_weight():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--depth-loss", "--depth-noise", "--depth-seed", "{l1,pearson}"):
        assert flag in p.stdout, flag
    assert "relative" in p.stdout
    p = _train("--depth-loss", "pearson")
    assert p.returncode != 0 and "--depth-loss pearson needs --lambda-depth > 0" in p.stderr
    p = _train("--depth-loss", "pearson", "--lambda-depth", "0")
    assert p.returncode != 0 and "--depth-loss pearson needs --lambda-depth > 0" in p.stderr
    p = _train("--depth-loss", "huber", "--lambda-depth", "0.1")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    p = _train("--depth-noise", "-0.5")
    assert p.returncode != 0 and "--depth-noise must be >= 0" in p.stderr
    # valid values are parsed before the other arguments are judged: the refusal below is theirs
    p = _train("--depth-loss", "pearson", "--lambda-depth", "0.1", "--depth-noise", "1", "--depth-seed", "3", "--lambda-dssim", "2")
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr
    p = _train("--depth-loss", "l1", "--depth-noise", "0.5", "--lambda-dssim", "2")      # l1 stays the default and takes the noise too
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr
