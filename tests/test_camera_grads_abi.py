"""CPU-side checks of the camera gradients (include/gsr_camera_grads.h): the header is plain C, the library exports and binds its
entry points, every argument is checked before anything is enqueued, the float64 yardstick the GPU tests use
(tests/camera_grad_reference.py) is itself the gradient -- it meets central finite differences of the float64 loss, with the
frustum clamp active and with a depth cotangent --, pose.pose_gradient meets finite differences in xi (through an independent
matrix exponential), apply_pose_delta(cam, 0) is the camera bit for bit, and the trainer refuses --optimize-poses with
several GPUs and a negative --pose-lr."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import compile_c99_probe, declared_names, fake_call_setup, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub
import camera_grad_reference as CG
import test_f64_reference as R

HDR = os.path.join(ROOT, "include", "gsr_camera_grads.h")
CAM_NAMES = {"gsr_backward_camera", "gsr_backward_camera_scratch_bytes"}


def test_camera_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_camera_grads.h"\n'
                                'int main(void) {\n'
                                '  int (*c)(const GsrScene *, const GsrCamera *, const GsrGeom *, float *, const void *, size_t, void *, size_t,\n'
                                '           void *) = gsr_backward_camera;\n'
                                '  size_t (*s)(int64_t) = gsr_backward_camera_scratch_bytes;\n'
                                '  float out[GSR_CAMERA_GRAD_FLOATS];\n'
                                '  (void)c; (void)s; (void)out; return 0; }\n')


def test_camera_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == CAM_NAMES
    _lib = sub("_lib")
    assert set(_lib.CAMERA_EXPORTS) == declared
    for other in (_lib.EXPORTS, _lib.CAPACITY_EXPORTS, _lib.LOSS_EXPORTS, _lib.AUX_EXPORTS):
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gsr_camera_grads.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in open(os.path.join(ROOT, "include", "gsr.h")).read()
    L = _lib.lib()
    assert L.gsr_backward_camera_scratch_bytes(0) == 0
    assert L.gsr_backward_camera_scratch_bytes(1) > 0
    # a fixed grid: the scratch stops growing with N
    assert L.gsr_backward_camera_scratch_bytes(1 << 26) == L.gsr_backward_camera_scratch_bytes(1 << 22)


def test_camera_arguments_are_checked_before_any_hip_call(libpath):
    """Fake 16-byte-aligned pointers: every case below returns before anything is dereferenced or enqueued."""
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    ws_bytes = int(L.gsr_backward_workspace_bytes(N, 0, W, H))
    sc_bytes = int(L.gsr_backward_camera_scratch_bytes(N))

    def geom(**over):
        g = _lib.GsrGeom(A, None, None, None, None, None, None, None, A, None, None)
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def call(g=None, out=A, ws=A, wsb=ws_bytes, scr=A, scb=sc_bytes, sc=scene, cm=cam, no_geom=False):
        gp = None if no_geom else C.byref(g or geom())
        return L.gsr_backward_camera(C.byref(sc) if sc is not None else None, C.byref(cm) if cm is not None else None, gp, out, ws, wsb,
                                     scr, scb, None)

    assert call(sc=None) == _lib.GSR_E_NULL
    assert call(cm=None) == _lib.GSR_E_NULL
    assert call(out=None) == _lib.GSR_E_NULL
    assert call(no_geom=True) == _lib.GSR_E_NULL
    assert call(g=geom(radii=None)) == _lib.GSR_E_NULL
    assert call(g=geom(clamped_state=None)) == _lib.GSR_E_NULL
    assert call(out=A + 4) == _lib.GSR_E_ALIGN
    assert call(ws=A + 8) == _lib.GSR_E_ALIGN
    assert call(scr=A + 4) == _lib.GSR_E_ALIGN
    assert call(g=geom(cov3D=A + 4)) == _lib.GSR_E_ALIGN
    assert call(g=geom(sh_dir_grad=A + 12)) == _lib.GSR_E_ALIGN
    assert call(ws=None) == _lib.GSR_E_WORKSPACE
    assert call(wsb=ws_bytes - 1) == _lib.GSR_E_WORKSPACE
    assert call(scr=None) == _lib.GSR_E_WORKSPACE
    assert call(scb=sc_bytes - 1) == _lib.GSR_E_WORKSPACE
    bad = _lib.GsrScene(-1, A, A, A, A, A, 3, 1.0, 1)
    assert call(sc=bad) == _lib.GSR_E_DIMS
    bad = _lib.GsrScene(N, A, A, A, A, A, 4, 1.0, 1)
    assert call(sc=bad) == _lib.GSR_E_DIMS
    bad_cam = _lib.GsrCamera()
    bad_cam.W, bad_cam.H = 0, H
    assert call(cm=bad_cam) == _lib.GSR_E_DIMS
    bad = _lib.GsrScene(N, A, A, None, A, A, 3, 1.0, 1)
    assert call(sc=bad) == _lib.GSR_E_NULL
    bad = _lib.GsrScene(N, A, A + 4, A, A, A, 3, 1.0, 1)
    assert call(sc=bad) == _lib.GSR_E_ALIGN


# ---------------------------------------------------------------------------------------------------- the float64 yardstick
def _small_case(cameras, oracle, **over):
    args = dict(W=40, H=32, n=14, degree=3, train=True, bg=(0.2, 0.1, 0.3), sm=1.1, seed=41, outside=0.0, behind=0.0, opaque=0.0,
                faint=0.0, bright=0.0)
    args.update(over)
    sc, cam, kw = R.make_case(cameras, **args)
    buf = oracle.render_gaussians(**kw)[2]
    return sc, cam, kw, buf


def _fd_check(sc, kw, buf, dpix=None, ddep=None, dalpha=None, h=1e-6):
    g, scale = CG.camera_gradient_f64(sc, kw, buf["radii"], buf["point_list"], buf["ranges"], dpix, ddep, dalpha)
    cam = CG.Cam(kw)
    base = [cam.view.clone(), cam.proj.clone(), cam.campos.clone()]
    fd = np.zeros(36)
    for k in range(35):
        t, j = (0, k) if k < 16 else ((1, k - 16) if k < 32 else (2, k - 32))
        vals = []
        for sgn in (1.0, -1.0):
            args = [b.clone() for b in base]
            args[t].view(-1)[j] += sgn * h
            vals.append(CG.loss_f64(sc, kw, args[0], args[1], args[2], buf["radii"], buf["point_list"], buf["ranges"], dpix, ddep, dalpha))
        fd[k] = (vals[0] - vals[1]) / (2 * h)
    assert np.abs(g).max() > 0
    err = np.abs(fd - g)
    tol = 1e-6 * (scale + np.abs(g).max())
    assert (err <= tol).all(), (np.where(err > tol)[0], fd[err > tol], g[err > tol])
    return g


def test_f64_camera_gradient_meets_finite_differences(cameras, oracle):
    sc, cam, kw, buf = _small_case(cameras, oracle)
    assert (buf["radii"] > 0).sum() >= 8
    dpix = R.pixel_grad(kw["image_height"], kw["image_width"], seed=3)
    g = _fd_check(sc, kw, buf, dpix=dpix)
    # the structure the kernel relies on: view column 3 and proj column 2 are never read, entry 35 is padding
    assert not np.any(g[[3, 7, 11, 15, 18, 22, 26, 30, 35]])


def test_f64_camera_gradient_with_the_frustum_clamp_active(cameras, oracle):
    sc, cam, kw, buf = _small_case(cameras, oracle, n=16, seed=43, outside=0.4)
    t = CG.Cam(kw)
    pv = CG.F._homog(CG.F._t(sc["means"], (-1, 3))) @ t.view
    r = (pv[:, :2] / pv[:, 2:3]).abs().numpy()
    clamped = ((r[:, 0] > 1.3 * t.tanx) | (r[:, 1] > 1.3 * t.tany)) & (buf["radii"] > 0)
    assert clamped.sum() >= 1, "no visible Gaussian beyond the 1.3 tan(fov) clamp"
    _fd_check(sc, kw, buf, dpix=R.pixel_grad(kw["image_height"], kw["image_width"], seed=4))


def test_f64_camera_gradient_with_depth_and_alpha_cotangents(cameras, oracle):
    sc, cam, kw, buf = _small_case(cameras, oracle, seed=44, train=False)
    H, W = kw["image_height"], kw["image_width"]
    rng = np.random.default_rng(5)
    ddep = rng.normal(0, 1, (H, W))
    dalpha = rng.normal(0, 1, (H, W))
    g_d = _fd_check(sc, kw, buf, ddep=ddep)                 # the depth cotangent alone reaches view (not proj's xy only)
    assert np.abs(g_d[[2, 6, 10, 14]]).max() > 0
    _fd_check(sc, kw, buf, dpix=R.pixel_grad(H, W, seed=6), ddep=ddep, dalpha=dalpha)


# ------------------------------------------------------------------------------------------------------------ pose helpers
def _lego_cam(cameras):
    from conftest import lego_camera
    return lego_camera(cameras, frame=0, width=64, height=48)


def test_apply_pose_delta_zero_is_the_camera_bit_for_bit(cameras):
    pose = sub("pose")
    for cam in (_lego_cam(cameras), cameras.toy_camera(64, 48)):
        out = pose.apply_pose_delta(cam, np.zeros(6))
        assert set(out) == set(cam)
        for k, v in cam.items():
            if isinstance(v, np.ndarray):
                assert out[k].dtype == v.dtype and np.array_equal(out[k], v), k
            else:
                assert out[k] == v, k


def _V_of(cam, xi):
    """V(xi) through torch.linalg.matrix_exp of the 4x4 twist: independent of pose.se3_exp's closed form."""
    xi = torch.as_tensor(xi, dtype=torch.float64)
    rho, phi = xi[:3], xi[3:]
    X = torch.zeros(4, 4, dtype=torch.float64)
    X[0, 1], X[0, 2], X[1, 2] = -phi[2], phi[1], -phi[0]
    X[1, 0], X[2, 0], X[2, 1] = phi[2], -phi[1], phi[0]
    X[:3, 3] = rho
    return torch.as_tensor(np.asarray(cam["world_to_camera"], np.float64)) @ torch.linalg.matrix_exp(X).T


def test_pose_gradient_meets_finite_differences(cameras):
    pose = sub("pose")
    cam = _lego_cam(cameras)
    rng = np.random.default_rng(9)
    gV, gP, gc = rng.normal(size=(4, 4)), rng.normal(size=(4, 4)), rng.normal(size=3)
    P = torch.as_tensor(np.asarray(cam["proj_matrix"], np.float64))

    def L(xi):
        V = _V_of(cam, xi)
        c = torch.linalg.inv(V)[3, :3]
        return float((V * torch.as_tensor(gV)).sum() + ((V @ P) * torch.as_tensor(gP)).sum() + (c * torch.as_tensor(gc)).sum())
    for xi0 in (np.zeros(6), np.array([0.03, -0.02, 0.05, 0.02, -0.01, 0.03])):
        g = pose.pose_gradient(cam, xi0, gV, gP, gc)
        h = 1e-6
        fd = np.array([(L(xi0 + h * e) - L(xi0 - h * e)) / (2 * h) for e in np.eye(6)])
        np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-7 * np.abs(fd).max())
        # and apply_pose_delta is that same V(xi), rounded to the camera's float32
        V = pose.apply_pose_delta(cam, xi0)["world_to_camera"]
        np.testing.assert_allclose(V, _V_of(cam, xi0).numpy(), rtol=0, atol=1e-6)
    # the torch tensors backward() returns are taken as they are
    g_t = pose.pose_gradient(cam, np.zeros(6), torch.as_tensor(gV, dtype=torch.float32), torch.as_tensor(gP, dtype=torch.float32),
                             torch.as_tensor(gc, dtype=torch.float32))
    np.testing.assert_allclose(g_t, pose.pose_gradient(cam, np.zeros(6), np.float32(gV), np.float32(gP), np.float32(gc)), rtol=0, atol=0)


def test_pose_error_and_random_delta(cameras):
    pose = sub("pose")
    cam = _lego_cam(cameras)
    xi = pose.random_pose_delta(np.random.default_rng(1), 2.0, 0.1)
    rot, _ = pose.pose_error(pose.apply_pose_delta(cam, xi), cam)
    assert abs(rot - 2.0) < 1e-3
    assert pose.pose_error(cam, cam) == (0.0, 0.0)


# ----------------------------------------------------------------------------------------------------------------- trainer
def _train(*extra):
    train = os.path.join(ROOT, "examples", "train.py")
    return subprocess.run([sys.executable, train, *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_and_checks_the_pose_flags():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--optimize-poses", "--pose-lr", "--pose-noise-deg", "--pose-noise-trans", "--pose-seed"):
        assert flag in p.stdout, flag
    p = _train("--optimize-poses", "--gpus", "2")
    assert p.returncode != 0 and "--optimize-poses" in p.stderr and "one GPU" in p.stderr, p.stderr[-2000:]
    for extra in (["--optimize-poses", "--pose-lr", "-0.001"], ["--pose-lr", "nan"], ["--pose-noise-deg", "-1"],
                  ["--pose-noise-trans", "-0.1"]):
        p = _train(*extra)
        assert p.returncode != 0 and "must be >= 0" in p.stderr, (extra, p.stderr[-2000:])
