"""CPU-side checks of the backward through the inverse-depth and alpha images (include/gsr_aux_grads.h): the header is plain C,
the library exports its entry points, every argument is checked before anything is enqueued, the trainer refuses bad
--lambda-depth / --lambda-alpha, load_nerf hands out the PNG alpha, and the float64 yardstick the GPU tests use
(f64_reference.blend_f64 with the depth not detached) is itself the gradient: it meets central finite differences."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import compile_c99_probe, declared_names, fake_call_setup, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub
import f64_reference as F

HDR = os.path.join(ROOT, "include", "gsr_aux_grads.h")
AUX_NAMES = {"gsr_backward_aux", "gsr_backward_blend_aux", "gsr_backward_geom_aux", "gsr_depth_loss_grad", "gsr_alpha_loss_grad"}


def test_aux_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_aux_grads.h"\n'
                                'int main(void) {\n'
                                '  GsrPixelGrads pg = {0, 0, 0};\n'
                                '  int (*a)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrBinning *, const GsrImage *,\n'
                                '           const GsrPixelGrads *, const GsrGrads *, float *, void *, size_t, void *) = gsr_backward_aux;\n'
                                '  int (*b)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrBinning *, const GsrImage *,\n'
                                '           const GsrPixelGrads *, float *, void *, size_t, void *) = gsr_backward_blend_aux;\n'
                                '  int (*g)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrGrads *, float *, void *, size_t, void *)\n'
                                '      = gsr_backward_geom_aux;\n'
                                '  int (*d)(const float *, const float *, const float *, float *, float *, int32_t, int32_t, float, void *) = gsr_depth_loss_grad;\n'
                                '  int (*l)(const float *, const float *, const float *, float *, float *, int32_t, int32_t, float, void *) = gsr_alpha_loss_grad;\n'
                                '  (void)pg; (void)a; (void)b; (void)g; (void)d; (void)l; return 0; }\n')


def test_aux_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == AUX_NAMES
    _lib = sub("_lib")
    assert set(_lib.AUX_EXPORTS) == declared
    for other in (_lib.EXPORTS, _lib.CAPACITY_EXPORTS, _lib.LOSS_EXPORTS):
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gsr_aux_grads.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in open(os.path.join(ROOT, "include", "gsr.h")).read()


def test_aux_backward_arguments_are_checked_before_any_hip_call(libpath):
    """Fake 16-byte-aligned pointers: every case below returns before anything is dereferenced or enqueued."""
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    ws_bytes = int(L.gsr_backward_workspace_bytes(N, 100, W, H))
    img = _lib.GsrImage(None, None, A, A)

    def geom(records=None, depths=None):   # re-packed records (xy / conic_opacity / rgb) unless `records`
        return _lib.GsrGeom(A, None, None, A, depths, A, A, A, A, records, None)

    def grads(**over):
        g = _lib.GsrGrads(A, A, A, A, A, None, None, None, None)
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def call(pg, g=None, gr=None, D=100, ws=A, wsb=ws_bytes, inv=None, half=None, **bover):
        b = _lib.GsrBinning(D, A, A, None, None, None, 0)
        for k, v in bover.items():
            setattr(b, k, v)
        g = geom(records=A) if g is None else g
        pgr = C.byref(pg) if pg is not None else None
        if half == "blend":
            return L.gsr_backward_blend_aux(C.byref(scene), C.byref(cam), C.byref(g), C.byref(b), C.byref(img), pgr, None, ws, wsb, None)
        if half == "geom":
            return L.gsr_backward_geom_aux(C.byref(scene), C.byref(cam), C.byref(g), C.byref(gr or grads()), inv, ws, wsb, None)
        return L.gsr_backward_aux(C.byref(scene), C.byref(cam), C.byref(g), C.byref(b), C.byref(img), pgr, C.byref(gr or grads()), inv,
                                  ws, wsb, None)

    PG = _lib.GsrPixelGrads
    for half in (None, "blend"):
        assert call(None, half=half) == _lib.GSR_E_NULL                             # no GsrPixelGrads at all
        assert call(PG(None, None, None), half=half) == _lib.GSR_E_NULL             # all three NULL
        # an inverse-depth gradient needs records that carry 1/depth: the forward's, or depths for the re-pack
        assert call(PG(None, A, None), g=geom(), half=half) == _lib.GSR_E_NULL
        assert call(PG(A, A, A), g=geom(), half=half) == _lib.GSR_E_NULL
        assert call(PG(None, A + 4, None), half=half) == _lib.GSR_E_ALIGN
        assert call(PG(None, None, A + 8), half=half) == _lib.GSR_E_ALIGN
        assert call(PG(A + 4, A, None), half=half) == _lib.GSR_E_ALIGN
        assert call(PG(None, A, None), D=-1, half=half) == _lib.GSR_E_OVERFLOW
        assert call(PG(None, A, None), D=(1 << 30) + 1, half=half) == _lib.GSR_E_OVERFLOW
        assert call(PG(None, None, A), wsb=ws_bytes - 1, half=half) == _lib.GSR_E_WORKSPACE
        assert call(PG(None, None, A), ws=None, half=half) == _lib.GSR_E_WORKSPACE
        assert call(PG(None, A, None), point_list=A + 4, half=half) == _lib.GSR_E_ALIGN
    # the whole call: the per-Gaussian half's own arguments are checked before the blend half enqueues anything
    assert call(PG(None, A, None), gr=grads(dL_dmean3D=None)) == _lib.GSR_E_NULL
    assert call(PG(None, A, None), gr=grads(dL_drot=A + 4)) == _lib.GSR_E_ALIGN
    assert call(PG(None, A, None), inv=A + 4) == _lib.GSR_E_ALIGN
    # the geom half
    assert call(PG(None, A, None), half="geom", gr=grads(dL_dscale=None)) == _lib.GSR_E_NULL
    assert call(PG(None, A, None), half="geom", inv=A + 8) == _lib.GSR_E_ALIGN
    assert call(PG(None, A, None), half="geom", wsb=int(L.gsr_backward_workspace_bytes(N, 0, W, H)) - 1) == _lib.GSR_E_WORKSPACE
    scene.rotations = A + 4
    assert call(PG(None, A, None)) == _lib.GSR_E_ALIGN


def test_aux_loss_arguments_are_checked_before_any_hip_call(libpath):
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    for fn in (L.gsr_depth_loss_grad, L.gsr_alpha_loss_grad):
        assert fn(None, A, None, A, A, W, H, 1.0, None) == _lib.GSR_E_NULL
        assert fn(A, None, A, A, A, W, H, 1.0, None) == _lib.GSR_E_NULL
        assert fn(A, A, A, A, None, W, H, 1.0, None) == _lib.GSR_E_NULL
        assert fn(A, A, A, A, A, 0, H, 1.0, None) == _lib.GSR_E_DIMS
        assert fn(A, A, None, None, A, W, -1, 1.0, None) == _lib.GSR_E_DIMS


def test_backward_refuses_a_call_without_any_pixel_gradient(monkeypatch):
    bwd = sub("backward")

    def no_gpu(*a, **k):
        raise AssertionError("reached the GPU")
    monkeypatch.setattr(bwd._host, "device_of", no_gpu)
    with pytest.raises(ValueError, match="dL_dpixels, dL_ddepth_image or dL_dalpha_image"):
        bwd.backward(background=[0, 0, 0], means3D=[[0, 0, 0]], dL_dpixels=None)


def _train(*extra):
    train = os.path.join(ROOT, "examples", "train.py")
    return subprocess.run([sys.executable, train, *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_the_depth_and_alpha_flags():
    p = _train("--help")
    assert p.returncode == 0 and "--lambda-depth" in p.stdout and "--depth-dir" in p.stdout and "--lambda-alpha" in p.stdout, p.stderr[-2000:]
    for extra in (["--lambda-depth", "-0.5"], ["--lambda-alpha", "-1"], ["--lambda-depth", "nan"]):
        p = _train(*extra)
        assert p.returncode != 0 and "must be >= 0" in p.stderr, (extra, p.stderr[-2000:])
    p = _train("--dataset", os.path.join(ROOT, "data", "lego"), "--lambda-depth", "0.1")
    assert p.returncode != 0 and "needs --depth-dir" in p.stderr, p.stderr[-2000:]


def _train_module():
    spec = importlib.util.spec_from_file_location("gsr_example_train_aux", os.path.join(ROOT, "examples", "train.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_load_nerf_returns_the_png_alpha(tmp_path):
    from PIL import Image
    lego = os.path.join(ROOT, "data", "lego")
    m = _train_module()
    cams, targets, alphas = m.load_nerf(lego, 2, alpha=True)
    cams0, targets0 = m.load_nerf(lego, 2)                     # unchanged without the keyword
    import json
    frames = json.load(open(os.path.join(lego, "transforms_train.json")))["frames"]
    for k in range(2):
        raw = np.asarray(Image.open(os.path.join(lego, frames[k]["file_path"] + ".png")))
        assert raw.shape[2] == 4
        np.testing.assert_array_equal(alphas[k], raw[:, :, 3].astype(np.float32) / 255.0)
        np.testing.assert_array_equal(targets[k], targets0[k])
        assert alphas[k].dtype == np.float32 and 0.0 < alphas[k].mean() < 1.0
    # --depth-dir: one .npy per frame, named after the file_path's last component
    for k in range(2):
        np.save(tmp_path / (os.path.basename(frames[k]["file_path"]) + ".npy"), np.full(alphas[k].shape, 0.25 + k, np.float32))
    *_, depths = m.load_nerf(lego, 2, depth_dir=str(tmp_path))
    assert [float(d.mean()) for d in depths] == [0.25, 1.25]


def _tiny_case():
    rng = np.random.default_rng(5)
    n, W, H = 6, 16, 16
    xy = torch.tensor(rng.uniform(3, 13, (n, 2)), dtype=torch.float64)
    conic = torch.tensor(np.stack([rng.uniform(0.05, 0.2, n), rng.uniform(-0.02, 0.02, n), rng.uniform(0.05, 0.2, n)], 1), dtype=torch.float64)
    op = torch.tensor(rng.uniform(0.3, 0.9, n), dtype=torch.float64)
    col = torch.tensor(rng.uniform(0, 1, (n, 3)), dtype=torch.float64)
    depth = torch.tensor(rng.uniform(1.0, 4.0, n), dtype=torch.float64)
    point_list = np.argsort(depth.numpy())
    ranges = np.array([[0, n]])
    bg = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    gD = torch.tensor(rng.normal(0, 1, (H, W)), dtype=torch.float64)
    gA = torch.tensor(rng.normal(0, 1, (H, W)), dtype=torch.float64)
    return xy, conic, op, col, depth, point_list, ranges, bg, W, H, gD, gA


def test_f64_inverse_depth_and_alpha_gradients_meet_finite_differences():
    """The GPU tests' yardstick: autograd of blend_f64's inverse-depth and alpha outputs (depth NOT detached) against central
    differences, on a 16x16 tile with six Gaussians whose alphas stay below the 0.99 cap."""
    xy, conic, op, col, depth, pl, ranges, bg, W, H, gD, gA = _tiny_case()

    def loss(xy, conic, op, col, depth):
        _, dep, fT, _ = F.blend_f64(xy, conic, op, col, depth, pl, ranges, bg, W, H)
        return (dep * gD).sum() + ((1.0 - fT) * gA).sum()
    args = [t.clone().requires_grad_(True) for t in (xy, conic, op, col, depth)]
    grads = [g if g is not None else torch.zeros_like(a)           # (the colours reach neither image)
             for g, a in zip(torch.autograd.grad(loss(*args), args, allow_unused=True), args)]
    assert float(grads[4].abs().max()) > 0 and float(grads[2].abs().max()) > 0      # depth and opacity both carry gradient
    h = 1e-6
    for k, (t, g) in enumerate(zip((xy, conic, op, col, depth), grads)):
        flat = t.reshape(-1)
        for i in range(flat.numel()):
            plus, minus = [a.clone() for a in (xy, conic, op, col, depth)], [a.clone() for a in (xy, conic, op, col, depth)]
            plus[k].reshape(-1)[i] += h
            minus[k].reshape(-1)[i] -= h
            with torch.no_grad():
                fd = (loss(*plus) - loss(*minus)) / (2 * h)
            assert abs(float(fd) - float(g.reshape(-1)[i])) <= 1e-5 * (1.0 + abs(float(fd))), (k, i, float(fd), float(g.reshape(-1)[i]))
