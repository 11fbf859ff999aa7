"""CPU-side checks of the weighted colour loss's C ABI and Python surface (include/gsr_weighted_loss.h): the header is plain C99, the
library exports what it declares and _lib binds it in a table of its own, every argument of each entry point is refused in the
documented order before anything is enqueued, the workspace sizes are 0 for bad sizes and monotone otherwise, loss.py refuses bad
`weights` before the GPU, and the trainer parses its flags, loads masks and refuses one of the wrong shape."""
import ctypes as C
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import A, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_weighted_loss.h")
NAMES = {"gsr_weight_total_workspace_bytes", "gsr_weight_total", "gsr_weighted_l1_loss_grad", "gsr_weighted_dssim_workspace_bytes",
         "gsr_weighted_l1_dssim_loss_grad"}


def test_weighted_loss_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_weighted_loss.h"\n'
                                'int main(void) {\n'
                                '  size_t (*a)(int32_t, int32_t) = gsr_weight_total_workspace_bytes;\n'
                                '  int (*b)(const float *, int32_t, int32_t, float *, void *, size_t, void *) = gsr_weight_total;\n'
                                '  int (*c)(const float *, const float *, const float *, const float *, float *, float *, int32_t, int32_t, float,\n'
                                '           void *, size_t, void *) = gsr_weighted_l1_loss_grad;\n'
                                '  size_t (*d)(int32_t, int32_t) = gsr_weighted_dssim_workspace_bytes;\n'
                                '  int (*e)(const float *, const float *, const float *, const float *, float *, float *, float *, int32_t, int32_t,\n'
                                '           float, int32_t, void *, size_t, void *) = gsr_weighted_l1_dssim_loss_grad;\n'
                                '  int w[2] = {GSR_SSIM_WINDOW_REFERENCE, GSR_SSIM_WINDOW_GAUSSIAN};\n'
                                '  (void)a; (void)b; (void)c; (void)d; (void)e; (void)w; return 0; }\n')


def test_weighted_loss_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.WEIGHTED_LOSS_EXPORTS) == declared
    others = [v for k, v in vars(_lib).items() if k.endswith("EXPORTS") and k != "WEIGHTED_LOSS_EXPORTS"]
    assert len(others) >= 10
    for other in others:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_weighted_loss.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "gsr_weight" not in gsr_h and "gsr_weight" not in open(os.path.join(ROOT, "include", "gsr_loss.h")).read()
    assert "#define GSR_ABI_VERSION 7" in gsr_h and _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_weight" in ln} == declared      # exactly the declared names


def test_workspace_bytes_are_zero_for_bad_sizes_and_monotone(libpath):
    L = sub("_lib").lib()
    for fn in (L.gsr_weight_total_workspace_bytes, L.gsr_weighted_dssim_workspace_bytes):
        for W, H in ((0, 10), (10, 0), (-1, 5), (5, -3), (1 << 15, 1 << 14)):
            assert fn(W, H) == 0, (W, H)
        sizes = [fn(W, H) for W, H in ((1, 1), (31, 17), (64, 48), (800, 800), (1920, 1080), (1 << 14, 1 << 14))]
        assert sizes[0] > 0 and sizes == sorted(sizes) and all(b % 16 == 0 for b in sizes), sizes
    for W, H in ((1, 1), (33, 15), (800, 800)):
        assert L.gsr_weighted_dssim_workspace_bytes(W, H) == L.gsr_dssim_workspace_bytes(W, H)      # the unweighted call's layout
    assert L.gsr_weight_total_workspace_bytes(1 << 14, 1 << 14) >= 4 * 512                          # a float per workgroup, 512 at most


def test_weighted_loss_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN,
    GSR_E_WORKSPACE, in that order."""
    _lib = sub("_lib")
    L = _lib.lib()
    W, H = 40, 24
    sum_b, dssim_b = int(L.gsr_weight_total_workspace_bytes(W, H)), int(L.gsr_weighted_dssim_workspace_bytes(W, H))
    bad_dims = (dict(w=0), dict(h=-3), dict(w=1 << 15, h=1 << 14))

    def tot(m=A, w=W, h=H, t=A + 4, ws=A, b=sum_b):
        return L.gsr_weight_total(m, w, h, t, ws, b, None)

    for k in ("m", "t", "ws"):
        assert tot(**{k: None}) == tot(**{k: None}, w=0) == _lib.GSR_E_NULL, k                      # NULL before the dimensions
    for bad in bad_dims:
        assert tot(**bad) == tot(**bad, m=A + 4) == tot(**bad, b=0) == _lib.GSR_E_DIMS, bad         # ... before alignment and workspace
    for k in ("m", "ws"):
        assert tot(**{k: A + 4}) == tot(**{k: A + 4}, b=0) == _lib.GSR_E_ALIGN, k                   # alignment before the workspace
    assert tot(t=A + 2) == _lib.GSR_E_ALIGN                                                         # a single float: 4 bytes
    assert tot(b=sum_b - 1) == tot(b=0) == _lib.GSR_E_WORKSPACE

    def l1(r=A, t=A, m=A, mt=A + 4, g=A, ls=A + 8, w=W, h=H, scale=1.0, ws=A, b=sum_b):
        return L.gsr_weighted_l1_loss_grad(r, t, m, mt, g, ls, w, h, scale, ws, b, None)

    for k in ("r", "t", "m", "mt", "ls", "ws"):
        assert l1(**{k: None}) == l1(**{k: None}, h=0) == _lib.GSR_E_NULL, k
    for bad in bad_dims + (dict(scale=-0.5), dict(scale=math.nan), dict(scale=math.inf)):
        assert l1(**bad) == l1(**bad, r=A + 4) == l1(**bad, b=0) == _lib.GSR_E_DIMS, bad
    for k in ("r", "t", "m", "g", "ws"):
        assert l1(**{k: A + 4}) == l1(**{k: A + 4}, b=0) == _lib.GSR_E_ALIGN, k
    assert l1(mt=A + 2) == l1(ls=A + 1) == _lib.GSR_E_ALIGN
    assert l1(b=sum_b - 1) == l1(g=None, b=0) == _lib.GSR_E_WORKSPACE                               # (pixel_grad may be NULL: not an error)

    def ds(r=A, t=A, m=A, mt=A + 4, g=A, ls=A + 8, ss=A + 12, w=W, h=H, lam=0.2, window=1, ws=A, b=dssim_b):
        return L.gsr_weighted_l1_dssim_loss_grad(r, t, m, mt, g, ls, ss, w, h, lam, window, ws, b, None)

    for k in ("r", "t", "m", "mt", "ls", "ss", "ws"):
        assert ds(**{k: None}) == ds(**{k: None}, w=0) == _lib.GSR_E_NULL, k
    for bad in bad_dims + (dict(lam=-0.01), dict(lam=1.01), dict(lam=math.nan), dict(window=2), dict(window=-1)):
        assert ds(**bad) == ds(**bad, t=A + 4) == ds(**bad, b=0) == _lib.GSR_E_DIMS, bad
    for k in ("r", "t", "m", "g", "ws"):
        assert ds(**{k: A + 4}) == ds(**{k: A + 4}, b=0) == _lib.GSR_E_ALIGN, k
    assert ds(mt=A + 2) == ds(ls=A + 2) == ds(ss=A + 1) == _lib.GSR_E_ALIGN
    assert ds(b=dssim_b - 1) == ds(g=None, b=0) == _lib.GSR_E_WORKSPACE
    assert ds(b=int(L.gsr_weighted_dssim_workspace_bytes(W, H - 16))) == _lib.GSR_E_WORKSPACE


def test_python_surface_refuses_bad_weights_before_the_gpu(monkeypatch):
    loss, _lib = sub("loss"), sub("_lib")

    def no_gpu(*a, **k):
        raise AssertionError("reached the GPU")
    monkeypatch.setattr(loss._host, "device_of", no_gpu)
    monkeypatch.setattr(loss._host, "to_dev", no_gpu)
    monkeypatch.setattr(_lib, "lib", no_gpu)
    img = np.zeros((5, 7, 3), np.float32)
    ok = np.ones((5, 7), np.float32)
    for fn in (loss.l1_loss_and_gradients, loss.l1_dssim_loss_and_gradients):
        for bad, msg in ((np.ones((7, 5), np.float32), "shape"), (np.ones((5, 7, 1), np.float32), r"\(H, W\)"), (np.ones((5, 7), np.float64), "float32"),
                         (torch.ones(5, 7, dtype=torch.float16), "float32"), (torch.ones(5, 8), "shape"), ([[1.0] * 7] * 5, "tensor or a numpy"),
                         (np.ones((0, 7), np.float32), r"\(H, W\)")):
            with pytest.raises(ValueError, match=msg):
                fn(img, img, weights=bad)
        with pytest.raises(AssertionError, match="reached the GPU"):
            fn(img, img, weights=ok)                                                   # a valid image passes the checks
    for bad, msg in ((np.ones((5, 7), np.float64), "float32"), (np.ones(7, np.float32), r"\(H, W\)"), ("mask.png", "tensor or a numpy")):
        with pytest.raises(ValueError, match=msg):
            loss.PixelWeights(bad)
    for bad in (-1, 2.5, "5"):
        with pytest.raises(ValueError, match="dilate"):
            loss.PixelWeights(ok, dilate=bad)

    class OnDevice(torch.Tensor):
        is_cuda = True
    on = lambda d: type("T", (OnDevice,), {"device": torch.device("cuda", d)})
    with pytest.raises(ValueError, match="weights on cuda:1, image on cuda:0"):
        loss.l1_dssim_loss_and_gradients(torch.zeros(5, 7, 3).as_subclass(on(0)), img, weights=torch.ones(5, 7).as_subclass(on(1)))


def _train(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300)


def _train_module():
    spec = importlib.util.spec_from_file_location("gsr_example_train", os.path.join(ROOT, "examples", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)          # __name__ != "__main__": no self-launch, no GPU call
    return mod


def test_trainer_parses_the_mask_flags():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--mask-dir", "--mask-dilate", "--occluders", "--occluder-seed", "--occluder-size", "--mask-occluders"):
        assert flag in p.stdout, flag
    for args, msg in ((("--mask-dir", "masks"), "--mask-dir needs --dataset"), (("--mask-occluders",), "--mask-occluders needs --occluders"),
                      (("--mask-dilate", "-1"), "--mask-dilate and --occluders must be >= 0"), (("--occluders", "-2"), "must be >= 0"),
                      (("--occluders", "2", "--occluder-size", "0"), "--occluder-size in (0, 1]"),
                      (("--occluders", "2", "--occluder-size", "1.5"), "--occluder-size in (0, 1]")):
        p = _train(*args)
        assert p.returncode != 0 and msg in p.stderr, (args, p.stderr[-2000:])
    # valid values are parsed before the other arguments are judged: the refusal below is theirs
    p = _train("--dataset", "data/lego", "--mask-dir", "masks", "--mask-dilate", "3", "--occluders", "3", "--occluder-seed", "1", "--occluder-size",
               "0.2", "--mask-occluders", "--lambda-dssim", "2")
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr


def test_trainer_loads_masks_and_refuses_a_wrong_shape(tmp_path):
    from PIL import Image
    train = _train_module()
    data = os.path.join(ROOT, "data", "lego")
    rng = np.random.default_rng(0)
    m0 = rng.integers(0, 256, (800, 800), dtype=np.uint8)
    m1 = rng.integers(0, 256, (800, 800, 3), dtype=np.uint8)
    Image.fromarray(m0).save(tmp_path / "r_0.png")                    # one channel
    Image.fromarray(m1).save(tmp_path / "r_1.png")                    # RGB: the first channel counts
    masks = train.load_masks(data, str(tmp_path), 2, [(800, 800)] * 2)
    assert [m.dtype for m in masks] == [np.float32] * 2 and [m.shape for m in masks] == [(800, 800)] * 2
    np.testing.assert_array_equal(masks[0], m0.astype(np.float32) / 255.0)
    np.testing.assert_array_equal(masks[1], m1[:, :, 0].astype(np.float32) / 255.0)
    Image.fromarray(m0[:400]).save(tmp_path / "r_1.png")
    with pytest.raises(ValueError, match=r"r_1: mask \(400, 800\) for a \(800, 800\) image"):
        train.load_masks(data, str(tmp_path), 2, [(800, 800)] * 2)
    Image.fromarray(m0).save(tmp_path / "r_1.png")
    with pytest.raises(OSError):
        train.load_masks(data, str(tmp_path), 3, [(800, 800)] * 3)    # r_2.png is missing


def test_occluders_are_seeded_opaque_and_differ_per_view():
    train = _train_module()
    H, W = 60, 80
    a = train.occluder_rects(H, W, 3, 0.25, 0, 0)
    assert len(a) == 3 and train.occluder_rects(H, W, 3, 0.25, 0, 0)[0][:4] == a[0][:4]
    assert [r[:4] for r in train.occluder_rects(H, W, 3, 0.25, 0, 1)] != [r[:4] for r in a]       # elsewhere in the next view
    assert [r[:4] for r in train.occluder_rects(H, W, 3, 0.25, 1, 0)] != [r[:4] for r in a]       # ... and under another seed
    for y0, y1, x0, x1, rgb in a:
        assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W and y1 - y0 <= 0.25 * H and x1 - x0 <= 0.25 * W
        assert rgb.max() == 1.0 and rgb.min() == 0.0                                              # saturated
    t = np.full((H, W, 3), 0.5, np.float32)
    out, mask = train.paste_occluders(t, a)
    assert (t == 0.5).all() and mask.dtype == np.float32 and set(np.unique(mask)) == {0.0, 1.0}
    assert (out[mask == 1.0] == 0.5).all() and (out[mask == 0.0] != 0.5).any(axis=-1).all()
    y0, y1, x0, x1, rgb = a[-1]
    assert (out[y0:y1, x0:x1] == rgb).all()                                                        # the last one pasted lies on top
