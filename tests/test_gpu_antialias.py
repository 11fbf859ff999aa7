"""
The antialiased mode (include/gsr_antialias.h) on the MI355X, against the float64 yardstick tests/antialias_reference.py and
against the classic mode of the same build.

  * forward identities, exact: everything but the opacity column is the classic render's, bit for bit; the opacity column is
    float32(opacity) * float32(aa_scale); the images are those of a classic render of the scene with that product as its opacity;
    sized and capacity mode give the same bits;
  * aa_scale against the float64 rho by a float32 error model: the one cancellation is det0 = a0 c0 - b^2, so
        |rho32 - rho64| <= K eps32 rho (1 + (a0 c0 + b^2) / |det0|) / 2        (the 1/2: through the square root)
    with K from tests/golden/antialias_margins.json: the worst ratio measured on the case matrix on the MI355X, times ten;
  * image / final_T / n_contrib against the yardstick by parity's image contract, the backward by parity.assert_grad, from the
    kernels' own forward (records, recomputed Sigma3D, direction sums) and from packed copies with cov3D read back; Gaussians within
    a relative 1e-3 of the floor r = 0.000025 sit on a kink of rho and are left out of the gradient comparison (at most 1 % of
    the visible ones, asserted);
  * exact side conditions: the blend-stage gradients are those of the classic backward over the substituted scene, and
    dL_dopacity is aa_scale times that backward's, to one rounding;
  * it is a real change; the camera gradient; composition with the other keywords; NULL = classic through every entry point; a
    seeded sweep; the trainer.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, sub
import antialias_reference as AA
import f64_reference as F
import parity
import test_antialias_reference as TA
import test_f64_reference as R
from test_gpu_camera_grads import TRIP as CAMERA_TRIP, _cam36
from test_gpu_fuzz import _case as fuzz_case

pytestmark = pytest.mark.gpu
MODE = dict(rasterize_mode="antialiased")
EPS32 = float(np.finfo(np.float32).eps)
MARGINS = json.load(open(os.path.join(ROOT, "tests", "golden", "antialias_margins.json")))
RHO_K = float(MARGINS["rho_model_constant"])              # 10 x rho_model_worst_measured
SWEEP = int(os.environ.get("GSR_AA_FUZZ_CASES", "32"))
IDENTICAL = ["radii", "point_offsets", "points_xy_image", "depths", "colors", "cov3Ds", "clamped_state", "point_list", "ranges"]


def _np(buf):
    return {k: parity.to_np(v) for k, v in buf.items()}


def _aa_scale(buf):
    return parity.to_np(buf["conic_opacity"]._gsr_aa_scale[0])


def _substituted(sc, eff):
    """The scene with the effective opacity as its opacity (float32: the very product the kernel stored)."""
    return dict(sc, opacities=np.ascontiguousarray(eff, np.float32).reshape(np.asarray(sc["opacities"]).shape))


def _kw_of(kw, sc):
    return dict(kw, opacity=sc["opacities"])


def _forward_identities(gsr, sc, kw, capacity=False):
    """Item 3.  Returns (antialiased frame, classic frame of the substituted scene, aa_scale)."""
    fwd = sub("forward").render_gaussians
    cl = gsr.render_gaussians(**kw)
    aa = gsr.render_gaussians(**kw, **MODE)
    b_cl, b_aa = _np(cl[2]), _np(aa[2])
    for k in IDENTICAL:
        parity.assert_exact(k, b_aa[k], b_cl[k])
    parity.assert_exact("conic", b_aa["conic_opacity"][:, :3], b_cl["conic_opacity"][:, :3])
    rho = _aa_scale(aa[2])
    op = np.asarray(sc["opacities"], np.float32).reshape(-1)
    vis = b_aa["radii"] > 0
    assert rho.dtype == np.float32 and np.all(rho[~vis] == 0) and np.all(rho[vis] > 0) and np.all(rho <= 1)
    parity.assert_exact("effective opacity", b_aa["conic_opacity"][:, 3], np.where(vis, op * rho, np.float32(0)))
    sub_sc = _substituted(sc, b_aa["conic_opacity"][:, 3])
    cs = gsr.render_gaussians(**_kw_of(kw, sub_sc))
    for name, a, b in (("image", aa[0], cs[0]), ("depth image", aa[1], cs[1]), ("final_Ts", aa[2]["final_Ts"], cs[2]["final_Ts"]),
                       ("n_contrib", aa[2]["n_contrib"], cs[2]["n_contrib"])):
        parity.assert_exact(name, a, b)
    if capacity:
        D = int(b_aa["point_list"].shape[0])
        cp = fwd(**kw, **MODE, capacity=D + 7, capacity_hint=D)
        assert sub("forward").rendered_count(cp[2]) == (D, False)
        b_cp = _np(cp[2])
        for k in IDENTICAL + ["conic_opacity", "final_Ts", "n_contrib"]:
            parity.assert_exact("capacity " + k, b_cp[k][:D] if k == "point_list" else b_cp[k], b_aa[k])
        parity.assert_exact("capacity image", cp[0], aa[0])
        parity.assert_exact("capacity depth image", cp[1], aa[1])
        parity.assert_exact("capacity aa_scale", _aa_scale(cp[2]), rho)
    return aa, cs, rho


def _rho_ratio(pre, rho32, radii):
    """Item 4: worst |rho32 - rho64| / (eps32 rho (1 + cond) / 2) over the visible Gaussians off the kink; on the floor, exact."""
    vis = (radii > 0) & ~pre["culled"]
    r, rho64, cond = pre["rho_r"], pre["rho"].numpy(), pre["rho_cond"]
    floor = vis & (r <= AA.FLOOR) & ~AA.near_floor(pre)
    assert np.all(rho32[floor] == np.float32(np.sqrt(np.float32(AA.FLOOR)))), "rho on the floor is sqrt(0.000025) in float32"
    m = vis & (r > AA.FLOOR) & ~AA.near_floor(pre)
    if not m.any():
        return 0.0
    model = EPS32 * rho64[m] * (1.0 + cond[m]) / 2.0
    return float((np.abs(rho32[m].astype(np.float64) - rho64[m]) / model).max())


def _bkw(sc, cam, kw, buf, dpix, packed=False):
    b = backward_kwargs(sc, cam, kw, buf, dpix)
    if packed:      # packed copies of everything but the tagged conic_opacity view: records re-packed, Sigma3D read back, SH re-read
        for k in ("means2D", "rgb", "cov3Ds", "clamped"):
            b[k] = b[k].clone()
        b["geom_buffer"] = dict(b["geom_buffer"], means2D=b["means2D"], rgb=b["rgb"], clamped=b["clamped"])
    return b


def _acc(g, N):
    """The (N, 16) accumulator records of a backward() result, as float32 numpy (gsr_backward_accumulators_offset)."""
    ws = g["dL_dmean2D"]._gsr_backward_ws[0]
    off = int(sub("_lib").lib().gsr_backward_accumulators_offset(N))
    return parity.to_np(ws[off:off + 64 * N].view(torch.float32).view(N, 16))


def _masked(a, keep, n):
    a = parity.to_np(a).astype(np.float64)
    return a.reshape(n, -1)[keep]


def _check_case(gsr, sc, cam, kw, label, capacity=False, report=None):
    """Items 3, 4 and 5 on one scene."""
    N = np.asarray(sc["means"]).reshape(-1, 3).shape[0]
    H, W = kw["image_height"], kw["image_width"]
    aa, cs, rho32 = _forward_identities(gsr, sc, kw, capacity)
    buf = _np(aa[2])
    pre = AA.preprocess_aa_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    ratio = _rho_ratio(pre, rho32, buf["radii"])
    if report is not None:
        report[label] = ratio
    print(f"\n{label}: rho error / model, worst {ratio:.3f} (bound {RHO_K})")
    assert ratio <= RHO_K, (label, ratio)
    if N == 0 or not (buf["radii"] > 0).any():
        return
    # image, final_T, n_contrib against the yardstick (the float64 blend over the kernel's own lists)
    i64, d64, T64, n64 = AA.render_aa_f64(sc, kw, buf["point_list"], buf["ranges"], pre=pre)
    parity.assert_image("image", aa[0], i64)
    parity.assert_image("final_T", buf["final_Ts"], T64)
    parity.assert_counts("n_contrib", buf["n_contrib"], n64)
    # backward
    dpix = R.pixel_grad(H, W)
    vis = buf["radii"] > 0
    kink = AA.near_floor(pre) & vis
    assert kink.sum() <= 0.01 * vis.sum(), (label, int(kink.sum()), int(vis.sum()))
    keep = ~kink
    ref = AA.backward_aa_f64(sc, kw, buf["point_list"], buf["ranges"], dpix, pre=pre)
    g_cl = gsr.backward(**backward_kwargs(_substituted(sc, buf["conic_opacity"][:, 3]), cam, _kw_of(kw, sc), cs[2], dpix))
    for packed in (False, True):
        g = gsr.backward(**_bkw(sc, cam, kw, aa[2], dpix, packed), **MODE)
        if not packed and all(isinstance(sc[k], torch.Tensor) for k in ("scales", "rotations")):
            assert sub("backward").backward.last_call_recomputed_sigma3d
        for k in parity.GRAD_KEYS:
            rows = N * 16 if k == "dL_dshs" else N
            kk = np.repeat(keep, 16) if k == "dL_dshs" else keep
            parity.assert_grad(f"{label} {k}{' (packed)' if packed else ''}", _masked(g[k], kk, rows), _masked(ref[k], kk, rows))
        assert not np.any(parity.to_np(g["dL_dcov3D"]))
        # exact side conditions against the classic backward over the substituted scene
        for k in ("dL_dcolor", "dL_dmean2D", "dL_dconic"):
            parity.assert_grad(f"{label} {k} vs classic", g[k], parity.to_np(g_cl[k]))
        acc10 = _acc(g, N)[:, 10]      # dL_dopacity = aa_scale * (column 10 of this call's own records), one rounding
        parity.assert_exact(f"{label} dL_dopacity = aa_scale * g", g["dL_dopacity"], np.where(vis, rho32 * acc10, acc10).astype(np.float32))
        parity.assert_grad(f"{label} dL_dopacity vs aa_scale * classic", g["dL_dopacity"], rho32.astype(np.float64) * parity.to_np(g_cl["dL_dopacity"]))


# ------------------------------------------------------------------------------------------- items 3-5: the case matrix
@pytest.mark.parametrize("name", TA.AA_CASE_NAMES)
def test_case_matrix_forward_rho_and_backward(cameras, name):
    sc, cam, kw = TA.aa_case(cameras, name)
    _check_case(pkg(), sc, cam, kw, name, capacity=True)


def test_device_tensors_in_place_recompute_sigma3d_and_use_the_direction_sums(cameras):
    """The trainer's path: device tensors used in place, so the backward recomputes Sigma3D (cov3D = NULL) and takes the forward's
    direction sums; against the yardstick as above."""
    gsr = pkg()
    sc, cam, kw = TA.aa_case(cameras, "aa_200x136_n700")
    dev = torch.device("cuda", 0)
    t = {k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in sc.items()}
    t["opacities"] = t["opacities"].reshape(-1)
    kw_t = dict(kw, means3D=t["means"], opacity=t["opacities"], scales=t["scales"], rotations=t["rotations"], sh=t["shs"].reshape(-1, 3))
    t["shs"] = kw_t["sh"]
    aa = gsr.render_gaussians(**kw_t, **MODE)
    buf = _np(aa[2])
    dpix = R.pixel_grad(kw["image_height"], kw["image_width"])
    g = gsr.backward(**backward_kwargs(t, cam, kw_t, aa[2], dpix), **MODE)
    bw = sub("backward").backward
    assert bw.last_call_recomputed_sigma3d and bw.last_call_used_forward_sh_dir and bw.last_call_used_forward_records
    pre = AA.preprocess_aa_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    ref = AA.backward_aa_f64(sc, kw, buf["point_list"], buf["ranges"], dpix, pre=pre)
    assert not (AA.near_floor(pre) & (buf["radii"] > 0)).any()
    for k in parity.GRAD_KEYS:
        parity.assert_grad(k, g[k], ref[k])
    # a write into the opacity after the render: the frame is stale
    t["opacities"].mul_(1.0)
    with pytest.raises(ValueError, match="written in place since"):
        gsr.backward(**backward_kwargs(t, cam, kw_t, aa[2], dpix), **MODE)


C2_SCALE_MEDIAN = 0.002      # scene units: about half a pixel at C2's camera (the share with rho < 0.5 is asserted)


def test_c2_size_geometry_half_against_f64():
    """At C2 size the float64 blend is out of reach; the per-Gaussian half is not: the float64 geometry (f64_reference's two stages
    plus the rho VJP) fed with the kernel's own blend-stage cotangents, against the kernel's dL_dmean3D / dL_dscale / dL_drot /
    dL_dopacity by the gradient contract; the forward identities hold there as everywhere."""
    gsr = pkg()
    from conftest import render_kwargs
    cfg = dict(gsr.scenes.CONFIGS["C2"])
    W, H = cfg.pop("width"), cfg.pop("height")
    sc = gsr.scenes.synthetic_scene(cfg["n"], C2_SCALE_MEDIAN, cfg["scale_sigma"], cfg["seed"])     # sub-pixel splats at 800 x 800
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H)
    aa, cs, rho32 = _forward_identities(gsr, sc, kw)
    buf = _np(aa[2])
    vis = buf["radii"] > 0
    pre = AA.preprocess_aa_f64(sc, kw, 3, 1.0)
    share = float((rho32[vis] < 0.5).mean())
    ratio = _rho_ratio(pre, rho32, buf["radii"])
    print(f"\nC2: {int(vis.sum())} visible, rho < 0.5 on {share:.3f}; rho error / model worst {ratio:.3f}")
    assert share >= TA.SUBPIXEL_SHARE and ratio <= RHO_K
    kink = AA.near_floor(pre) & vis
    assert kink.sum() <= 0.01 * vis.sum()
    dpix = (np.random.default_rng(0).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)
    g = gsr.backward(**backward_kwargs(sc, cam, kw, aa[2], dpix), **MODE)
    N = sc["means"].shape[0]
    acc = _acc(g, N)
    m3, _, dcov6, _ = F.geometry_vjp_f64(sc, kw, 3, vis, buf["clamped_state"], acc[:, 3:6], acc[:, 6:10], acc[:, 0:3], cov3D=buf["cov3Ds"])
    r_mean, r_cov = AA.rho_vjp_f64(sc, kw, vis, np.asarray(sc["opacities"], np.float64).reshape(-1) * acc[:, 10], cov3D=buf["cov3Ds"])
    dsc, drot = F.cov3d_backward_f64(sc, kw, vis, dcov6 + r_cov, None)
    keep = ~kink
    for k, ref in (("dL_dmean3D", m3 + r_mean), ("dL_dscale", dsc), ("dL_drot", drot)):
        print("  %-12s frac %.6f  max err / max|g| %.3e" % ((k,) + parity.grad_margin(_masked(g[k], keep, N), ref.numpy()[keep])))
        parity.assert_grad("C2 " + k, _masked(g[k], keep, N), ref.numpy()[keep])
    parity.assert_exact("C2 dL_dopacity", g["dL_dopacity"], np.where(vis, rho32 * acc[:, 10], acc[:, 10]).astype(np.float32))
    # the rho term is a good part of the scale gradient there
    assert np.abs(F.cov3d_backward_f64(sc, kw, vis, r_cov, None)[0].numpy()).max() > 1e-2 * np.abs(dsc.numpy()).max()


# ------------------------------------------------------------------------------------------- item 6: it is a real change
def test_the_mode_changes_the_image_and_the_scale_gradient(cameras):
    gsr = pkg()
    sc, cam, kw = TA.aa_case(cameras, "aa_200x136_n700")
    cl, aa = gsr.render_gaussians(**kw), gsr.render_gaussians(**kw, **MODE)
    d = np.abs(parity.to_np(cl[0]) - parity.to_np(aa[0])).max(axis=2)
    assert (d > parity.IMG_LOOSE).mean() > 0.05, float((d > parity.IMG_LOOSE).mean())
    with pytest.raises(AssertionError):
        parity.assert_image("classic as antialiased", cl[0], parity.to_np(aa[0]))
    dpix = R.pixel_grad(kw["image_height"], kw["image_width"])
    g_aa = gsr.backward(**backward_kwargs(sc, cam, kw, aa[2], dpix), **MODE)
    g_cl = gsr.backward(**backward_kwargs(sc, cam, kw, cl[2], dpix))
    with pytest.raises(AssertionError):
        parity.assert_grad("classic dL_dscale as antialiased", g_cl["dL_dscale"], parity.to_np(g_aa["dL_dscale"]))
    # ... and not only through the opacity: the classic backward of the substituted scene misses the rho term
    cs = gsr.render_gaussians(**_kw_of(kw, _substituted(sc, parity.to_np(aa[2]["conic_opacity"])[:, 3])))
    g_cs = gsr.backward(**backward_kwargs(sc, cam, kw, cs[2], dpix))
    with pytest.raises(AssertionError):
        parity.assert_grad("substituted classic dL_dscale as antialiased", g_cs["dL_dscale"], parity.to_np(g_aa["dL_dscale"]))


# ------------------------------------------------------------------------------------------- item 7: the camera gradient
@pytest.mark.parametrize("name", ["aa_64x48_n65", "aa_200x136_n700", "aa_needles"])
def test_camera_gradient_against_the_extended_yardstick(cameras, name):
    gsr = pkg()
    sc, cam, kw = TA.aa_case(cameras, name)
    H, W = kw["image_height"], kw["image_width"]
    dpix = (np.random.default_rng(17).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)
    aa = gsr.render_gaussians(**kw, **MODE)
    buf = _np(aa[2])
    got = _cam36(gsr.backward(**backward_kwargs(sc, cam, kw, aa[2], dpix), **MODE, camera_grad=True))
    again = _cam36(gsr.backward(**backward_kwargs(sc, cam, kw, aa[2], dpix), **MODE, camera_grad=True))
    ref, scale = AA.camera_gradient_aa_f64(sc, kw, buf["radii"], buf["point_list"], buf["ranges"], dpix)
    zero = scale == 0
    assert not np.any(got[zero]) and np.isfinite(got).all()
    err = float((np.abs(got - ref)[~zero] / scale[~zero]).max())
    classic = _cam36(gsr.backward(**backward_kwargs(sc, cam, kw, gsr.render_gaussians(**kw)[2], dpix), camera_grad=True))
    print(f"\n{name}: camera gradient error / sum |term| {err:.2e} (bound {CAMERA_TRIP:.1e}); classic differs by "
          f"{float((np.abs(classic - ref)[~zero] / scale[~zero]).max()):.2e}")
    assert err <= CAMERA_TRIP
    assert float((np.abs(classic - ref)[~zero] / scale[~zero]).max()) > 10 * CAMERA_TRIP      # a build that ignores the mode fails
    assert np.abs(got - again).max() <= 1e-5 * np.abs(ref).max()        # two whole calls: float-atomic order of the blend only


def test_camera_call_is_bitwise_reproducible_and_null_is_the_classic_call(cameras):
    """gsr_backward_camera_aa twice on one workspace gives the same bits; with aa_scale = NULL it gives gsr_backward_camera's."""
    gsr = pkg()
    _lib, _host = sub("_lib"), sub("_host")
    L = _lib.lib()
    sc, cam, kw = TA.aa_case(cameras, "aa_200x136_n3000")
    dev = torch.device("cuda", 0)
    H, W = kw["image_height"], kw["image_width"]
    aa = gsr.render_gaussians(**kw, **MODE)
    dpix = R.pixel_grad(H, W)
    g = gsr.backward(**backward_kwargs(sc, cam, kw, aa[2], dpix), **MODE, camera_grad=True)
    ws = g["dL_dmean2D"]._gsr_backward_ws[0]
    N = sc["means"].shape[0]
    t = lambda a, shape: torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).to(dev)
    means, scales, rots, op, shs = t(sc["means"], (N, 3)), t(sc["scales"], (N, 3)), t(sc["rotations"], (N, 4)), t(sc["opacities"], (N,)), t(sc["shs"], (N * 16, 3))
    scene = _lib.GsrScene(N, means.data_ptr(), scales.data_ptr(), rots.data_ptr(), op.data_ptr(), shs.data_ptr(), int(kw["degree"]),
                          float(kw["scale_modifier"]), 1)
    camera = _host.make_camera(kw["viewmatrix"], kw["projmatrix"], kw["campos"], kw["background"], kw["tan_fovx"], kw["tan_fovy"], W, H)
    radii, cl, c3 = aa[2]["radii"], aa[2]["clamped_state"], aa[2]["cov3Ds"]
    geom = _lib.GsrGeom(radii.data_ptr(), None, None, None, None, c3.data_ptr(), None, None, cl.data_ptr(), None, None)
    rho = aa[2]["conic_opacity"]._gsr_aa_scale[0]
    scratch = torch.empty(int(L.gsr_backward_camera_scratch_bytes(N)), dtype=torch.uint8, device=dev)
    stream = _host.raw_stream(dev)
    outs = []
    for aa_ptr in (rho.data_ptr(), rho.data_ptr(), None):
        out = torch.full((36,), float("nan"), device=dev)
        _lib.check(L.gsr_backward_camera_aa(C.byref(scene), C.byref(camera), C.byref(geom), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                            scratch.data_ptr(), scratch.numel(), aa_ptr, stream))
        outs.append(out.cpu().numpy())
    out = torch.full((36,), float("nan"), device=dev)
    _lib.check(L.gsr_backward_camera(C.byref(scene), C.byref(camera), C.byref(geom), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     scratch.data_ptr(), scratch.numel(), stream))
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[2], out.cpu().numpy())
    assert not np.array_equal(outs[0], outs[2])
    assert np.abs(outs[0] - _cam36(g)).max() <= 1e-6 * np.abs(outs[0]).max()     # (cov3D read back here, recomputed or read there)


# ------------------------------------------------------------------------------------------- item 8: composition
def test_null_aa_scale_is_the_classic_call_through_python_sized_entry_points(cameras):
    """aa_scale = NULL through gsr_forward_count_aa, gsr_forward_capacity_aa, gsr_backward_aa and gsr_backward_geom_aa gives the
    bits of the classic entry points: the Python surface is driven with a library handle whose classic names are bound to the _aa
    functions with a NULL array."""
    gsr = pkg()
    _lib = sub("_lib")
    L = _lib.lib()
    sc, cam, kw = TA.aa_case(cameras, "aa_200x136_n700")
    dpix = R.pixel_grad(kw["image_height"], kw["image_width"])
    payloads = []

    def run():
        f = gsr.render_gaussians(**kw)
        fc = sub("forward").render_gaussians(**kw, capacity=int(f[2]["point_list"].shape[0]))
        g = gsr.backward(**backward_kwargs(sc, cam, kw, f[2], dpix))
        g2 = gsr.backward(**backward_kwargs(sc, cam, kw, f[2], dpix), sh_gradient="both", on_payload=payloads.append,
                          dL_dalpha_image=np.ones(dpix.shape[:2], np.float32))
        return f, fc, g, g2

    ref = run()

    class Null:
        """The library with the classic names routed through the _aa entry points, aa_scale = NULL."""
        def __getattr__(self, name):
            return getattr(L, name)
        gsr_forward_count = staticmethod(lambda *a: L.gsr_forward_count_aa(*a[:-1], None, a[-1]))
        gsr_forward_capacity = staticmethod(lambda *a: L.gsr_forward_capacity_aa(*a[:-1], None, a[-1]))
        gsr_backward_flags = staticmethod(lambda *a: L.gsr_backward_aa(*a[:-1], None, a[-1]))
        gsr_backward_geom_aux = staticmethod(lambda *a: L.gsr_backward_geom_aa(*a[:-1], None, a[-1]))

    real = _lib.lib
    _lib.lib = lambda: Null()
    try:
        got = run()
    finally:
        _lib.lib = real
    for k in ref[0][2]:
        parity.assert_exact(k, got[0][2][k], ref[0][2][k])
        parity.assert_exact("capacity " + k, got[1][2][k], ref[1][2][k])
    parity.assert_exact("image", got[0][0], ref[0][0])
    parity.assert_exact("capacity image", got[1][0], ref[1][0])
    for a, b in ((got[2], ref[2]), (got[3], ref[3])):
        for k in ("dL_dcolor", "dL_dmean2D", "dL_dconic", "dL_dopacity"):       # float atomics: the same kernels, atomic order
            parity.assert_grad(k, a[k], parity.to_np(b[k]))
        # the per-Gaussian half is deterministic given the accumulators: recompute nothing, compare through them
        for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dshs"):
            parity.assert_grad(k, a[k], parity.to_np(b[k]))


def test_composes_with_aux_absgrad_and_on_payload(cameras):
    gsr = pkg()
    sc, cam, kw = TA.aa_case(cameras, "aa_200x136_n700")
    H, W = kw["image_height"], kw["image_width"]
    rng = np.random.default_rng(5)
    dpix, gD, gA = R.pixel_grad(H, W), rng.normal(0, 1, (H, W)).astype(np.float32), rng.normal(0, 1, (H, W)).astype(np.float32)
    aa = gsr.render_gaussians(**kw, **MODE)
    buf = _np(aa[2])
    sub_sc = _substituted(sc, buf["conic_opacity"][:, 3])
    cs = gsr.render_gaussians(**_kw_of(kw, sub_sc))
    rho = _aa_scale(aa[2])
    N = sc["means"].shape[0]

    def bk(scene, frame, **extra):
        b = backward_kwargs(scene, cam, _kw_of(kw, scene), frame[2], dpix)
        b["geom_buffer"] = dict(b["geom_buffer"], depths=frame[2]["depths"])
        return gsr.backward(**b, **extra)

    # depth + alpha: blend-stage arrays and dL_dinv_depths as the classic aux backward of the substituted scene; the rest differs by rho
    g = bk(sc, aa, dL_ddepth_image=gD, dL_dalpha_image=gA, **MODE)
    c = bk(sub_sc, cs, dL_ddepth_image=gD, dL_dalpha_image=gA)
    for k in ("dL_dcolor", "dL_dmean2D", "dL_dconic", "dL_dinv_depths", "dL_dshs"):
        parity.assert_grad("aux " + k, g[k], parity.to_np(c[k]))
    parity.assert_grad("aux dL_dopacity", g["dL_dopacity"], rho.astype(np.float64) * parity.to_np(c["dL_dopacity"]))
    # ... and the geometry half against float64 fed with this call's own cotangents (the aux z term included through dL_dmean3D)
    acc = _acc(g, N)
    vis = buf["radii"] > 0
    r_mean, r_cov = AA.rho_vjp_f64(sc, kw, vis, np.asarray(sc["opacities"], np.float64).reshape(-1) * acc[:, 10], cov3D=buf["cov3Ds"])
    parity.assert_grad("aux dL_dmean3D = classic + rho term", g["dL_dmean3D"], parity.to_np(c["dL_dmean3D"]).astype(np.float64) + r_mean.numpy())
    # absgrad
    g = bk(sc, aa, absgrad=True, **MODE)
    c = bk(sub_sc, cs, absgrad=True)
    parity.assert_grad("dL_dmean2D_abs", g["dL_dmean2D_abs"], parity.to_np(c["dL_dmean2D_abs"]))
    plain = bk(sc, aa, **MODE)
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity"):
        parity.assert_grad("absgrad " + k, g[k], parity.to_np(plain[k]))
    # on_payload: two halves (gsr_backward_blend_flags + gsr_backward_geom_aa)
    seen = []
    g = bk(sc, aa, sh_gradient="both", on_payload=seen.append, **MODE)
    assert len(seen) == 1 and seen[0] is g["_view_payload"]
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dshs"):
        parity.assert_grad("on_payload " + k, g[k], parity.to_np(plain[k]))
    g = bk(sc, aa, sh_gradient="factored", on_payload=seen.append, **MODE)
    parity.assert_grad("factored dL_dscale", g["dL_dscale"], parity.to_np(plain["dL_dscale"]))


def test_two_views_on_two_streams(cameras):
    gsr = pkg()
    dev = torch.device("cuda", 0)
    cases = [TA.aa_case(cameras, n) for n in ("aa_200x136_n700", "aa_200x136_n3000")]
    serial = []
    for sc, cam, kw in cases:
        f = gsr.render_gaussians(**kw, **MODE)
        dpix = R.pixel_grad(kw["image_height"], kw["image_width"])
        serial.append((parity.to_np(f[0]), {k: parity.to_np(v) for k, v in gsr.backward(**backward_kwargs(sc, cam, kw, f[2], dpix), **MODE).items()
                                            if k in parity.GRAD_KEYS}))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in cases]
    out = []
    for _ in range(3):
        out = []
        for (sc, cam, kw), s in zip(cases, streams):
            with torch.cuda.stream(s):
                f = gsr.render_gaussians(**kw, **MODE)
                dpix = R.pixel_grad(kw["image_height"], kw["image_width"])
                out.append((f[0], gsr.backward(**backward_kwargs(sc, cam, kw, f[2], dpix), **MODE)))
    torch.cuda.synchronize()
    for (img, g), (img0, g0) in zip(out, serial):
        parity.assert_exact("image", img, img0)
        for k in parity.GRAD_KEYS:
            parity.assert_grad(k, g[k], g0[k])


# ------------------------------------------------------------------------------------------- item 9: a seeded sweep
@pytest.mark.parametrize("seed", range(SWEEP))
def test_random_configuration(cameras, scenes, seed):
    """Kind 2 of the generator (opacities 0.003 and 0.999 under large splats) puts whole regions of an image behind two layers at
    the alpha cap, where the stop test T < 1e-4 is decided by the float32 value of the cap: antialias_reference.ALPHA_CAP.  Seeds 22
    and 28 are such frames (58 and 21 % of the pixels)."""
    from conftest import render_kwargs
    sc, cam, W, H, degree, train, bg = fuzz_case(scenes, cameras, 7000 + seed)
    kw = render_kwargs(sc, cam, width=W, height=H, degree=degree, train_convention=train, bg=bg)
    _check_case(pkg(), sc, cam, kw, f"sweep {seed} ({W}x{H}, n={sc['means'].shape[0]})", capacity=seed % 4 == 0)


# ------------------------------------------------------------------------------------------- item 10: the trainer
def test_trainer_antialiased_through_density_control(tmp_path):
    """tests/test_gpu_train_real.py's reference schedule (1 600 iterations at 800 x 800 on the committed Lego views, ten
    density-control calls) with --rasterize-mode antialiased --lambda-dssim 0.2: finite parameters, that test's L1 bound, the PLY
    written and re-read."""
    log, out = tmp_path / "train.jsonl", tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
           "--iterations", "1600", "--gaussians", "5000", "--print-interval", "100", "--log", str(log), "--output", str(out),
           "--save-interval", "800", "--rasterize-mode", "antialiased", "--lambda-dssim", "0.2"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    rows = [json.loads(l) for l in open(log)]
    summary = [r for r in rows if r.get("record") == "summary"][-1]
    calls = [r for r in rows if r.get("record") == "density_control"]
    print(f"\nantialiased: {summary['iterations_per_s']} iterations/s; final 8-view L1 {summary['train_l1_mean']:.5f}, "
          f"PSNR {summary['train_psnr_mean']:.2f} dB; points {summary['points_final']}")
    assert len(calls) >= 10
    assert all(summary["parameters_finite"].values()), summary["parameters_finite"]
    assert summary["train_l1_mean"] < 0.045, summary
    ply = out / "point_cloud" / "iteration_1599" / "point_cloud.ply"
    assert ply.exists()
    back = sub("point_cloud").load_ply(str(ply))
    assert int(np.asarray(back["positions"]).shape[0]) == summary["points_final"]
    for k in ("positions", "scales", "rotations", "opacities", "shs"):
        assert np.isfinite(np.asarray(back[k])).all(), k
