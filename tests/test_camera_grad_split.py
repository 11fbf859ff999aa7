"""
The stage-isolated float64 camera gradient (camera_grad_reference.camera_gradient_from_cotangents) is camera_gradient_f64 split
in two.  On every case of test_f64_reference.CASE_NAMES, with the oracle's visibility and lists, the float64 blend cotangents
(blend_cotangents) are written in the kernel's accumulator layout (dL/dndc, half of dL/dB, dL/d(1/depth)) with the float64
colour clamp as `clamped`, and the second stage alone must give camera_gradient_f64's gradient and scale to 1e-12 of the
scale, for colour cotangents alone and for colour + inverse depth + alpha, in one chunk and in many.  The GPU tests of
test_gpu_camera_grads.py rely on this when they run the second stage alone on the kernel's own cotangents at millions of
Gaussians.  No GPU.
"""
import numpy as np
import pytest
import torch

import camera_grad_reference as CG
import f64_reference as F
import test_f64_reference as R

EXACT = 1e-12


def _cotangents(sc, kw, radii, point_list, ranges, dpix, ddep, dalpha):
    """The first stage of camera_gradient_f64 (its blend cotangents), converted to the kernel's layout."""
    cam = CG.Cam(kw)
    degree, sm = int(kw["degree"]), float(kw["scale_modifier"])
    sub, idx, N = CG._visible(sc, radii)
    with torch.no_grad():
        xy, con, raw, invd = CG._geometry_raw(sub, kw, cam, cam.view, cam.proj, cam.campos, degree, sm)
    col = torch.where(raw < 0, torch.zeros_like(raw), raw)
    clamped = torch.zeros(N, 3, dtype=torch.float64)
    clamped[idx] = (raw < 0).to(torch.float64)
    xy, con, col, invd = CG._scatter(N, idx, xy, con, col, invd)
    op = CG._scatter(N, idx, F._t(sub["opacities"], (idx.numel(),)))[0]
    gxy, gcon, gcol, ginv = CG.blend_cotangents(xy, con, op, col, invd, point_list, ranges, cam, dpix, ddep, dalpha)
    g_ndc = torch.zeros(N, 3, dtype=torch.float64)
    g_ndc[:, 0], g_ndc[:, 1] = gxy[:, 0] * (0.5 * cam.W), gxy[:, 1] * (0.5 * cam.H)
    g_conic = torch.zeros(N, 4, dtype=torch.float64)
    g_conic[:, 0], g_conic[:, 1], g_conic[:, 3] = gcon[:, 0], 0.5 * gcon[:, 1], gcon[:, 2]
    return [x.numpy() for x in (clamped, g_ndc, g_conic, gcol, ginv)]


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_isolated_second_stage_is_the_f64_camera_gradient(oracle, cameras, name):
    c = R.oracle_case(oracle, cameras, name)
    sc, kw, buf = c["sc"], c["kw"], c["buf"]
    H, W = kw["image_height"], kw["image_width"]
    rng = np.random.default_rng(23)
    dpix, ddep, dalpha = rng.normal(0, 1, (H, W, 3)), rng.normal(0, 1, (H, W)), rng.normal(0, 1, (H, W))
    radii, pl, ranges = (np.asarray(buf[k]) for k in ("radii", "point_list", "ranges"))
    n_vis = int((radii.reshape(-1) > 0).sum())
    assert n_vis > 0
    for label, (p, d, a) in {"colour": (dpix, None, None), "all": (dpix, ddep, dalpha)}.items():
        ref, ref_scale = CG.camera_gradient_f64(sc, kw, radii, pl, ranges, p, d, a)
        cot = _cotangents(sc, kw, radii, pl, ranges, p, d, a)
        assert np.abs(ref_scale).max() > 0
        for chunk in (262144, 1000, 7):
            got, scale = CG.camera_gradient_from_cotangents(sc, kw, radii, *cot, chunk=chunk)
            assert np.array_equal(got[ref_scale == 0], np.zeros(int((ref_scale == 0).sum()))), (label, chunk)
            np.testing.assert_allclose(scale, ref_scale, rtol=EXACT, atol=0, err_msg=f"{label} chunk {chunk}")
            err = np.abs(got - ref) / np.where(ref_scale > 0, ref_scale, 1.0)
            assert err.max() <= EXACT, (label, chunk, err.max(), int(err.argmax()))
    # the colour cotangent of a clamped channel passes nothing, whatever its value
    clamped, g_ndc, g_conic, gcol, ginv = cot
    if clamped.any():
        junk = np.where(clamped > 0, 1e3, gcol)
        a = CG.camera_gradient_from_cotangents(sc, kw, radii, clamped, g_ndc, g_conic, gcol, ginv)
        b = CG.camera_gradient_from_cotangents(sc, kw, radii, clamped, g_ndc, g_conic, junk, ginv)
        assert np.array_equal(a[0], b[0])
