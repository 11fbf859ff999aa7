"""CPU-side checks of the L1 + D-SSIM loss (include/gsr_loss.h): the header is plain C, the library exports its entry points
through their own ctypes table (gsr.h and its table are untouched), every argument is checked before anything is enqueued,
the Python surface refuses bad arguments before the GPU, and the trainer takes --lambda-dssim / --ssim-window."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest

from abi_helpers import compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_loss.h")


def test_loss_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_loss.h"\n'
                                'int main(void) {\n'
                                '    size_t (*b)(int32_t, int32_t) = gsr_dssim_workspace_bytes;\n'
                                '    int (*f)(const float *, const float *, float *, float *, float *, int32_t, int32_t, float, int32_t, void *, size_t,\n'
                                '             void *) = gsr_l1_dssim_loss_grad;\n'
                                '    int w[2] = {GSR_SSIM_WINDOW_REFERENCE, GSR_SSIM_WINDOW_GAUSSIAN};\n'
                                '    (void)b; (void)f; (void)w; return 0; }\n')


def test_loss_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == {"gsr_dssim_workspace_bytes", "gsr_l1_dssim_loss_grad"}
    lib = C.CDLL(libpath)
    for name in declared:
        assert hasattr(lib, name), name
    _lib = sub("_lib")
    assert set(_lib.LOSS_EXPORTS) == declared
    assert not (declared & set(_lib.EXPORTS)) and not (declared & set(_lib.CAPACITY_EXPORTS))
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert not any(name in gsr_h for name in declared)
    assert "#define GSR_ABI_VERSION 7" in gsr_h
    assert _lib.SSIM_WINDOWS == {"reference": 0, "gaussian": 1}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gsr_l1_dssim_loss_grad" in doc and "gsr_loss.h" in doc
    L = _lib.lib()
    assert hasattr(L, "gsr_l1_dssim_loss_grad") and L.gsr_abi_version() == 7


def test_workspace_bytes(libpath):
    L = sub("_lib").lib()
    assert L.gsr_dssim_workspace_bytes(0, 10) == 0 and L.gsr_dssim_workspace_bytes(10, -1) == 0
    assert L.gsr_dssim_workspace_bytes(1 << 15, 1 << 14) == 0          # W * H > 2^28
    a, b = L.gsr_dssim_workspace_bytes(1, 1), L.gsr_dssim_workspace_bytes(800, 800)
    assert 0 < a <= b and a % 16 == 0 and b % 16 == 0
    assert b >= 8 * ((800 + 31) // 32) * ((800 + 15) // 16)             # a float2 of partial sums per 32 x 16 tile at least


def test_loss_arguments_are_checked_before_any_hip_call(libpath):
    """Fake 16-byte-aligned pointers: every case below returns before anything is dereferenced or enqueued."""
    _lib = sub("_lib")
    L = _lib.lib()
    A = 0x10000
    W, H = 40, 24
    need = int(L.gsr_dssim_workspace_bytes(W, H))

    def call(r=A, t=A, g=A, l1=A, ss=A, W=W, H=H, lam=0.2, window=1, ws=A, ws_bytes=need):
        return L.gsr_l1_dssim_loss_grad(r, t, g, l1, ss, W, H, lam, window, ws, ws_bytes, None)

    for k in ("r", "t", "l1", "ss", "ws"):
        assert call(**{k: None}) == _lib.GSR_E_NULL, k
    for over in ({"W": 0}, {"H": -3}, {"W": 1 << 15, "H": 1 << 14}, {"lam": -0.01}, {"lam": 1.01}, {"lam": math.nan},
                 {"window": 2}, {"window": -1}):
        assert call(**over) == _lib.GSR_E_DIMS, over
    for k in ("r", "t", "g", "ws"):
        assert call(**{k: A + 4}) == _lib.GSR_E_ALIGN, k
    assert call(l1=A + 2) == _lib.GSR_E_ALIGN and call(ss=A + 1) == _lib.GSR_E_ALIGN
    assert call(ws_bytes=need - 1) == _lib.GSR_E_WORKSPACE
    assert call(ws_bytes=int(L.gsr_dssim_workspace_bytes(W, H - 16))) == _lib.GSR_E_WORKSPACE


def test_python_surface_refuses_bad_arguments_before_the_gpu(monkeypatch):
    loss = sub("loss")

    def no_gpu(*a, **k):
        raise AssertionError("reached the GPU")
    monkeypatch.setattr(loss._host, "device_of", no_gpu)
    img = [[[0.0, 0.0, 0.0]]]
    for kw in ({"lambda_dssim": -0.1}, {"lambda_dssim": 1.5}, {"lambda_dssim": math.nan}, {"window": "box"}):
        with pytest.raises(ValueError):
            loss.l1_dssim_loss_and_gradients(img, img, **kw)
    import torch
    with pytest.raises(ValueError):
        loss.l1_dssim_loss_and_gradients(img, img, loss_out=torch.zeros(2))
    with pytest.raises(ValueError):
        loss.l1_dssim_loss_and_gradients(img, img, ssim_out=torch.zeros(1))   # a host tensor


def test_trainer_parses_the_dssim_flags():
    train = os.path.join(ROOT, "examples", "train.py")
    p = subprocess.run([sys.executable, train, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "--lambda-dssim" in p.stdout and "--ssim-window" in p.stdout, p.stderr[-2000:]
    for bad in ("-0.5", "1.5", "nan"):
        p = subprocess.run([sys.executable, train, "--lambda-dssim", bad], capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr, (bad, p.stderr[-2000:])
    p = subprocess.run([sys.executable, train, "--ssim-window", "box"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "invalid choice" in p.stderr
