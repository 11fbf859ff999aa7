"""
The backward through the inverse-depth and alpha images (include/gsr_aux_grads.h) on the MI355X.

1. Identity: zero depth and alpha gradients give plain backward() (forward records and masks, and re-packed records; both
   blend block shapes through GSR_BWD_BLOCK in a subprocess).  Not bit for bit: the blend's float atomics add each Gaussian's
   per-block sums in whatever order the blocks finish, so two plain calls differ too; the bound is the plain call's own
   run-to-run spread, floored at SPREAD_FLOOR of max|g|.  (gsr_backward_aux with both pointers NULL runs gsr_backward's kernels.)
2. Against float64: tests/f64_reference.py's blend with the inverse depth differentiated (not detached) and the alpha image
   1 - T_final, chained into its geometry VJP plus the true z term of 1/depth, on test_f64_reference.CASES and the two LARGE
   cases of test_gpu_f64_reference.  Error = max |kernel - f64| / max |f64| per array; the tripwire is TRIP (see there).
   With the colour gradient in the mix the plain backward's own error against float64 on the same case is allowed on top
   (x 3): its dL_dmean3D is up to 0.66 of max|g| off on some cases (a float32 ill-conditioning test_gpu_f64_reference
   bounds per Gaussian with error models; depth or alpha alone stay below 5e-5).
3. Linearity: backward(dpix, gD, gA) = backward(dpix) + backward(gD) + backward(gA) - 2 backward(0) up to float-atomic
   reordering.  The backward is affine, not linear: quirk Q3 ((dL_dt, 1) * view^T) adds view[j][3] to dL_dmean3D of every visible
   Gaussian whatever the pixel gradients, so a sum of three calls holds that constant three times.
4. The factored / on_payload halves and a capacity-mode forward (K = D) agree with the dense call.
5. The loss kernels against torch float64.
6. Training: depth and alpha supervision lower their L1 against the same seed without them.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, render_kwargs, sub
import f64_reference as F
import parity
import test_f64_reference as R
import test_gpu_f64_reference as G

pytestmark = pytest.mark.gpu
GRAD_ARRAYS = ("dL_dmean3D", "dL_dcolor", "dL_dshs", "dL_dopacity", "dL_dscale", "dL_drot", "dL_dmean2D", "dL_dconic")

# Tripwire of check 2, max |kernel - f64| / max |f64| per array.  MEASURED: the worst margin on the MI355X over every case and the
# depth-only, alpha-only and all-three inputs (the all-three dL_dmean3D aside, see above); TRIP is 10x that.
MEASURED = {"dL_dmean3D": 4.14e-5, "dL_dcolor": 1.16e-5, "dL_dshs": 1.72e-5, "dL_dopacity": 3.75e-5, "dL_dscale": 1.21e-4,
            "dL_drot": 1.39e-4, "dL_dmean2D": 6.19e-5, "dL_dconic": 1.53e-5, "dL_dinv_depths": 2.34e-5}
TRIP = {k: 10.0 * v for k, v in MEASURED.items()}
# Checks 1, 3, 4: float-atomic reordering, relative to max|g|.  Measured at C2 (both block shapes): two plain calls differ by up to
# 1.9e-5 (dL_drot), a zero-aux call and a plain one by up to 8.0e-5 (dL_drot; every other array below 1.5e-5); 10x that.
SPREAD_FLOOR = 8e-4


def _rng_grads(H, W, seed):
    rng = np.random.default_rng(seed)
    dpix = (rng.normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)
    gD = (rng.normal(0, 1, (H, W)) / (H * W)).astype(np.float32)
    gA = (rng.normal(0, 1, (H, W)) / (H * W)).astype(np.float32)
    return dpix, gD, gA


def _c2_frame(bg=(0.1, 0.2, 0.3)):
    gsr = pkg()
    cfg = dict(gsr.scenes.CONFIGS["C2"])
    W, H = cfg.pop("width"), cfg.pop("height")
    sc = gsr.scenes.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H, bg=bg)
    return sc, cam, kw


def _bkw(sc, cam, kw, buf, dpix, packed=False):
    b = backward_kwargs(sc, cam, kw, buf, dpix)
    if packed:       # copies of the three arrays: the records are re-packed, with 1/depth from the forward's depths
        for k in ("means2D", "conic_opacity", "rgb"):
            b[k] = b[k].clone()
        b["geom_buffer"] = dict(b["geom_buffer"], means2D=b["means2D"], conic_opacity=b["conic_opacity"], rgb=b["rgb"],
                                depths=buf["depths"])
    else:
        b["geom_buffer"] = dict(b["geom_buffer"], depths=buf["depths"])
    return b


def _assert_within_spread(aux, p1, p2):
    for k in GRAD_ARRAYS:
        x, y, z = (parity.to_np(t[k]).astype(np.float64) for t in (aux, p1, p2))
        scale = max(float(np.abs(y).max()), 1e-30)
        spread = float(np.abs(z - y).max()) / scale
        err = float(np.abs(x - y).max()) / scale
        print(f"  {k}: zero-aux vs plain {err:.2e}, plain vs plain {spread:.2e}")
        assert err <= max(3.0 * spread, SPREAD_FLOOR), (k, err, spread)


@pytest.mark.parametrize("packed", [False, True])
def test_zero_aux_gradients_match_plain_backward(packed):
    gsr = pkg()
    bwd = sub("backward").backward
    sc, cam, kw = _c2_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    H, W = kw["image_height"], kw["image_width"]
    dpix, _, _ = _rng_grads(H, W, 1)
    snap = lambda g: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.items()}
    plain = snap(gsr.backward(**_bkw(sc, cam, kw, buf, dpix, packed)))
    assert bwd.last_call_used_forward_records is (not packed)
    plain2 = snap(gsr.backward(**_bkw(sc, cam, kw, buf, dpix, packed)))
    z = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    aux = gsr.backward(**_bkw(sc, cam, kw, buf, dpix, packed), dL_ddepth_image=z, dL_dalpha_image=z)
    assert bwd.last_call_used_forward_records is (not packed)
    _assert_within_spread(aux, plain, plain2)
    assert set(aux) == set(plain) | {"dL_dinv_depths"} and aux["dL_dinv_depths"].shape == (sc["means"].shape[0],)
    assert not torch.any(aux["dL_dinv_depths"])


@pytest.mark.parametrize("px", [32, 64])
def test_zero_aux_gradients_with_each_block_shape(px):
    env = dict(os.environ, GSR_BWD_BLOCK=str(px))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "match_plain or linear"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(r"\b3 passed", r.stdout), r.stdout[-2000:]


# ---- 2. against float64 ----
def aux_backward_f64(c, dpix, gD, gA):
    """Four float64 backwards of one case (colour only, inverse depth only, alpha only, all zero): autograd of the blend tile by tile
    (f64_reference's _blend_tile on the per-Gaussian 1/depth as a leaf), then f64_reference's geometry VJP and cov3d step,
    plus the true z term of the inverse depth, -invd^2 dL/dinvd dz/dmean."""
    sw = F._sw(None)
    pre, sc, kw = c["pre"], c["sc"], c["kw"]
    cam, N = pre["cam"], pre["N"]
    W, H = cam.W, cam.H
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    xy, con, op, col = leaf(pre["xy"]), leaf(pre["conic"]), leaf(pre["opacity"]), leaf(pre["colour"])
    depth = pre["depth"].detach()
    invd = leaf(torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth)))
    wrt = (xy, con, op, col, invd)
    t64 = lambda a, shape: torch.as_tensor(np.asarray(a, np.float64)).reshape(shape)
    cots = (t64(dpix, (H, W, 3)), t64(gD, (H, W)), t64(gA, (H, W)))
    acc = [[torch.zeros_like(t) for t in wrt] for _ in range(3)]
    pl = torch.as_tensor(np.asarray(c["buf"]["point_list"], dtype=np.int64))
    for s, e, yy, xx in F._tiles(W, H, c["buf"]["ranges"]):
        if e <= s:
            continue
        yt, xt = torch.as_tensor(yy), torch.as_tensor(xx)
        rgb, inv_d, T, _ = F._blend_tile(xy, con, op, col, invd, pl[s:e], xt.to(F.D), yt.to(F.D), cam.bg, sw["alpha_cap_passes_grad"])
        losses = ((rgb * cots[0][yt, xt]).sum(), (inv_d * cots[1][yt, xt]).sum(), ((1.0 - T) * cots[2][yt, xt]).sum())
        for j, l in enumerate(losses):
            gs = torch.autograd.grad(l, wrt, allow_unused=True, retain_graph=j < 2)
            for a, g in zip(acc[j], gs):
                if g is not None:
                    a += g
    acc.append([torch.zeros_like(t) for t in wrt])                    # zero cotangents: the Q3 constant alone
    visible = ~pre["culled"]
    view_z = cam.view[:3, 2].to(F.D)                                  # z = (m, 1) . view[:, 2]: dz/dm = view[:3, 2]
    out = []
    for gxy, gcon, gop, gcol, ginvd in acc:
        dL_dmean2D = torch.zeros(N, 3, dtype=F.D)
        dL_dmean2D[:, 0] = gxy[:, 0] * (0.5 * W)
        dL_dmean2D[:, 1] = gxy[:, 1] * (0.5 * H)
        dL_dconic = torch.zeros(N, 4, dtype=F.D)
        dL_dconic[:, 0], dL_dconic[:, 3] = gcon[:, 0], gcon[:, 2]
        dL_dconic[:, 1] = gcon[:, 1] * (0.5 if sw["conic_b_half"] else 1.0)
        m3, dshs, dcov6, _ = F.geometry_vjp_f64(sc, kw, int(kw["degree"]), visible, pre["clamped"], dL_dmean2D, dL_dconic, gcol)
        dsc, drot = F.cov3d_backward_f64(sc, kw, visible, dcov6)
        vis = torch.as_tensor(np.asarray(visible, dtype=bool))
        m3 = m3 + torch.where(vis, -(invd.detach() ** 2) * ginvd, torch.zeros_like(ginvd))[:, None] * view_z[None, :]
        n = lambda x: x.detach().numpy()
        out.append({"dL_dmean3D": n(m3), "dL_dcolor": n(gcol), "dL_dshs": n(dshs), "dL_dopacity": n(gop), "dL_dscale": n(dsc),
                    "dL_drot": n(drot), "dL_dmean2D": n(dL_dmean2D), "dL_dconic": n(dL_dconic), "dL_dinv_depths": n(ginvd)})
    return out


def _rel(k, ref):
    k = parity.to_np(k).astype(np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    return float(np.abs(k - ref).max()) / scale if scale > 0 else float(np.abs(k).max())


@pytest.mark.parametrize("name", R.CASE_NAMES + list(G.LARGE))
def test_aux_gradients_against_f64(oracle, cameras, name):
    gsr = pkg()
    c = G._case(oracle, cameras, name)
    sc, cam, kw = c["sc"], c["cam"], c["kw"]
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, gA = _rng_grads(H, W, 7)
    f_pix, f_dep, f_alp, f_zero = aux_backward_f64(c, dpix, gD, gA)
    f_all = {k: f_pix[k] + f_dep[k] + f_alp[k] - 2.0 * f_zero[k] for k in f_pix}     # (affine: Q3's constant once)
    buf = c["buf"]
    runs = {"plain": (dpix, None, None, f_pix), "depth": (None, gD, None, f_dep), "alpha": (None, None, gA, f_alp),
            "all": (dpix, gD, gA, f_all)}
    worst = {}
    for label, (p, d, a, ref) in runs.items():
        g = gsr.backward(**_bkw(sc, cam, kw, buf, p), dL_ddepth_image=d, dL_dalpha_image=a)
        for k in GRAD_ARRAYS + ("dL_dinv_depths",):
            if k not in g:
                continue
            if k == "dL_dshs":
                e = _rel(parity.to_np(g[k]).reshape(-1, 3)[:ref[k].reshape(-1, 3).shape[0]], ref[k].reshape(-1, 3))
            else:
                e = _rel(g[k], ref[k])
            worst[(label, k)] = e
    print(f"\n{name}: " + ", ".join(f"{l}/{k} {v:.2e}" for (l, k), v in worst.items()))
    bad = {}
    for (label, k), v in worst.items():
        bound = TRIP[k] + (3.0 * worst.get(("plain", k), 0.0) if label == "all" else 0.0)
        if label != "plain" and not v <= bound:
            bad[(label, k)] = (v, bound)
    assert not bad, bad


# ---- 3. linearity, 4. other paths ----
def _case_frame(oracle, cameras, name="256x256_n20000"):
    c = G._case(oracle, cameras, name)
    return c["sc"], c["cam"], c["kw"]


def _close(a, b, keys, rel):
    for k in keys:
        x, y = parity.to_np(a[k]).astype(np.float64), parity.to_np(b[k]).astype(np.float64)
        scale = max(float(np.abs(y).max()), 1e-30)
        assert float(np.abs(x - y).max()) <= rel * scale, (k, float(np.abs(x - y).max()) / scale)


def test_aux_backward_is_linear_in_its_three_inputs():
    gsr = pkg()
    sc, cam, kw = _c2_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, gA = _rng_grads(H, W, 3)
    snap = lambda g: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.items()}
    full = snap(gsr.backward(**_bkw(sc, cam, kw, buf, dpix), dL_ddepth_image=gD, dL_dalpha_image=gA))
    parts = [snap(gsr.backward(**_bkw(sc, cam, kw, buf, dpix))),
             snap(gsr.backward(**_bkw(sc, cam, kw, buf, None), dL_ddepth_image=gD)),
             snap(gsr.backward(**_bkw(sc, cam, kw, buf, None), dL_dalpha_image=gA))]
    zero = snap(gsr.backward(**_bkw(sc, cam, kw, buf, np.zeros_like(dpix))))
    summed = {k: sum(p[k].double() for p in parts) - 2.0 * zero[k].double() for k in GRAD_ARRAYS}
    _close(full, summed, GRAD_ARRAYS, 2 * SPREAD_FLOOR)
    _close(full, {"dL_dinv_depths": parts[1]["dL_dinv_depths"]}, ["dL_dinv_depths"], SPREAD_FLOOR)


def test_factored_halves_and_capacity_mode_agree_with_the_dense_aux_call():
    gsr = pkg()
    fwd = sub("forward")
    sc, cam, kw = _c2_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, gA = _rng_grads(H, W, 4)
    keys = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity")
    dense = gsr.backward(**_bkw(sc, cam, kw, buf, dpix), dL_ddepth_image=gD, dL_dalpha_image=gA)
    got = []
    fac = gsr.backward(**_bkw(sc, cam, kw, buf, dpix), dL_ddepth_image=gD, dL_dalpha_image=gA, sh_gradient="factored",
                       on_payload=got.append)
    assert len(got) == 1
    _close(fac, dense, keys + ("dL_dinv_depths",), SPREAD_FLOOR)
    D = int(buf["point_list"].shape[0])
    _, _, cbuf = fwd.render_gaussians(**kw, capacity=D, capacity_hint=D)
    cap = gsr.backward(**_bkw(sc, cam, kw, cbuf, dpix), dL_ddepth_image=gD, dL_dalpha_image=gA)
    _close(cap, dense, keys + ("dL_dinv_depths",), SPREAD_FLOOR)


# ---- 5. loss kernels ----
def test_depth_and_alpha_loss_kernels_against_torch_float64():
    gsr = pkg()
    H, W = 203, 317
    rng = np.random.default_rng(11)
    r = torch.tensor(rng.uniform(0, 1, (H, W)), dtype=torch.float32, device="cuda")
    t = torch.tensor(rng.uniform(0, 1, (H, W)), dtype=torch.float32, device="cuda")
    t[:5] = r[:5]                                                     # ties: sign(0) = +1
    mask = (torch.tensor(rng.uniform(0, 1, (H, W)), device="cuda") > 0.3).float()
    w = 0.37
    for m in (mask, None):
        s, g = gsr.loss.depth_loss_and_gradients(r, t, m, weight=w)
        d = r.double() - t.double()
        m64 = m.double() if m is not None else torch.ones_like(d)
        ref_g = (w / (W * H)) * m64 * torch.where(d < 0, -1.0, 1.0).double()
        assert torch.equal(g.double(), ref_g.float().double())
        ref_s = float((d.abs() * m64).sum())
        assert abs(float(s) - ref_s) <= 1e-6 * ref_s
        if m is not None:                                             # the reference's value kernel, same sum
            assert abs(gsr.loss.depth_loss(r, t, m) * (W * H) - float(s)) <= 1e-5 * ref_s
        # alpha form: r = 1 - final_T (evaluated in float32, as the kernel does)
        T = 1.0 - r
        s2, g2 = gsr.loss.alpha_loss_and_gradients(T, t, m, weight=w)
        d2 = (1.0 - T).double() - t.double()
        assert torch.equal(g2.double(), ((w / (W * H)) * m64 * torch.where(d2 < 0, -1.0, 1.0).double()).float().double())
        ref_s2 = float((d2.abs() * m64).sum())
        assert abs(float(s2) - ref_s2) <= 1e-6 * ref_s2
    s3, g3 = gsr.loss.alpha_loss_and_gradients(T, t, None, want_grad=False)
    assert g3 is None and float(s3) > 0


# ---- 6. training ----
def _train(tmp_path, tag, *extra):
    log = tmp_path / f"{tag}.jsonl"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--log", str(log), "--print-interval", "1000", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    for line in open(log):
        rec = json.loads(line)
        if rec["record"] == "summary":
            return rec


# Measured on the MI355X (300 iterations): synthetic 200x200, 8 views, --lambda-depth 1: depth L1 0.02770 -> 0.00937 (gain 0.662,
# colour L1 0.0314 -> 0.0363); Lego, 8 views, --lambda-alpha 0.1: alpha L1 0.1228 -> 0.1024 (gain 0.165, colour L1 0.0644 -> 0.0649).
# The bounds are half those gains.
DEPTH_GAIN_MIN = 0.33
ALPHA_GAIN_MIN = 0.08


def test_depth_supervision_lowers_the_depth_error(tmp_path):
    base = ["--iterations", "300", "--gaussians", "5000", "--views", "8", "--size", "200", "--init", "random"]
    s0 = _train(tmp_path, "d0", *base)
    s1 = _train(tmp_path, "d1", *base, "--lambda-depth", "1.0")
    gain = 1.0 - s1["train_depth_l1_mean"] / s0["train_depth_l1_mean"]
    print(f"\ndepth L1 {s0['train_depth_l1_mean']:.6f} -> {s1['train_depth_l1_mean']:.6f} (gain {gain:.3f}); colour L1 "
          f"{s0['train_l1_mean']:.5f} -> {s1['train_l1_mean']:.5f}")
    assert gain >= DEPTH_GAIN_MIN


def test_alpha_supervision_lowers_the_alpha_error_on_lego(tmp_path):
    base = ["--dataset", os.path.join(ROOT, "data", "lego"), "--iterations", "300", "--views", "8"]
    s0 = _train(tmp_path, "a0", *base)
    s1 = _train(tmp_path, "a1", *base, "--lambda-alpha", "0.1")
    gain = 1.0 - s1["train_alpha_l1_mean"] / s0["train_alpha_l1_mean"]
    print(f"\nalpha L1 {s0['train_alpha_l1_mean']:.6f} -> {s1['train_alpha_l1_mean']:.6f} (gain {gain:.3f}); colour L1 "
          f"{s0['train_l1_mean']:.5f} -> {s1['train_l1_mean']:.5f}")
    assert gain >= ALPHA_GAIN_MIN


# ---- 6. every backward export, driven directly: backward() itself calls only three of them ----
def test_every_backward_export_agrees_with_backward():
    """All eight backward entry points are one request behind the ABI.  On one frame with the forward's records, masks and a view
    payload, each export is called through ctypes with equivalent arguments -- whole or split, the pixel gradient alone or with the
    depth and alpha gradients, flags 0 or GSR_BWD_ABSGRAD -- and must give what backward() gives, under parity.assert_grad's
    contract (float atomics: not bit for bit)."""
    import ctypes as C
    gsr = pkg()
    _lib, _host = sub("_lib"), sub("_host")
    L = _lib.lib()
    W, H, N = 208, 160, 3000
    sc = gsr.scenes.synthetic_scene(N, 0.05, 0.6, 7)
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw = render_kwargs(sc, cam, width=W, height=H, bg=(0.1, 0.2, 0.3))
    _, _, buf = gsr.render_gaussians(**kw)
    dpix, gD, gA = _rng_grads(H, W, 6)
    dev, f32 = buf["radii"].device, torch.float32
    up = lambda a, shape: _host.to_dev(a, f32, dev, shape)
    t = dict(means=up(sc["means"], (-1, 3)), scales=up(sc["scales"], (-1, 3)), rot=up(sc["rotations"], (-1, 4)),
             op=up(sc["opacities"], (-1,)), sh=up(sc["shs"], (-1, 3)), dpix=up(dpix, (H, W, 3)), gD=up(gD, (H, W)), gA=up(gA, (H, W)))
    records = buf["points_xy_image"]._gsr_records[0]
    masks, _, order = buf["point_list"]._gsr_block_masks
    D = int(buf["point_list"].shape[0])
    assert D > 1000 and records.shape == (N, 16) and masks.numel() == D
    p = _host.ptr
    scene = _lib.GsrScene(N, p(t["means"]), p(t["scales"]), p(t["rot"]), p(t["op"]), p(t["sh"]), 3, 1.0, 1)
    camera = _host.make_camera(kw["viewmatrix"], kw["projmatrix"], kw["campos"], kw["background"], kw["tan_fovx"], kw["tan_fovy"], W, H)
    geom = _lib.GsrGeom(p(buf["radii"]), None, None, None, None, p(buf["cov3Ds"]), None, None, p(buf["clamped_state"]), p(records), None)
    binning = _lib.GsrBinning(D, p(buf["point_list"]), p(buf["ranges"]), p(masks), p(order), None, 0)
    img = _lib.GsrImage(None, None, p(buf["final_Ts"]), p(buf["n_contrib"]))
    head = (C.byref(scene), C.byref(camera), C.byref(geom))
    mid = (C.byref(binning), C.byref(img))
    need, off = int(L.gsr_backward_workspace_bytes(N, D, W, H)), int(L.gsr_backward_accumulators_offset(N))
    stream = _host.raw_stream(dev)
    refs = {}

    def reference(aux, absgrad):
        if (aux, absgrad) not in refs:
            extra = dict(dL_ddepth_image=gD, dL_dalpha_image=gA) if aux else {}
            g = gsr.backward(**_bkw(sc, cam, kw, buf, dpix), sh_gradient="both", absgrad=absgrad, **extra)
            assert sub("backward").backward.last_call_used_forward_records and sub("backward").backward.last_call_used_forward_masks
            refs[aux, absgrad] = {k: parity.to_np(v).copy() for k, v in g.items() if isinstance(v, torch.Tensor)}
        return refs[aux, absgrad]

    def run(api, split, aux, absgrad):
        """api: 'plain' (gsr.h), 'aux' (gsr_aux_grads.h) or 'flags' (gsr_densify_stats.h)."""
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = dict(dL_dmean3D=torch.empty((N, 3), dtype=f32, device=dev), dL_dscale=torch.empty((N, 3), dtype=f32, device=dev),
                   dL_drot=torch.empty((N, 4), dtype=f32, device=dev), dL_dopacity=torch.empty((N,), dtype=f32, device=dev),
                   dL_dshs=torch.empty((16 * N, 3), dtype=f32, device=dev))
        payload = torch.empty(3 * N + 4, dtype=f32, device=dev)
        inv = torch.empty((N,), dtype=f32, device=dev) if aux else None
        grads = _lib.GsrGrads(p(out["dL_dmean3D"]), p(out["dL_dscale"]), p(out["dL_drot"]), p(out["dL_dopacity"]), p(out["dL_dshs"]),
                              None, None, None, None if split else p(payload))
        pg = _lib.GsrPixelGrads(p(t["dpix"]), p(t["gD"]) if aux else None, p(t["gA"]) if aux else None)
        tail = (p(ws), need) + ((_lib.BWD_ABSGRAD if absgrad else 0,) if api == "flags" else ()) + (stream,)
        pix = p(t["dpix"]) if api == "plain" else C.byref(pg)
        with _host.on_device(dev):
            if split:
                blend = {"plain": L.gsr_backward_blend, "aux": L.gsr_backward_blend_aux, "flags": L.gsr_backward_blend_flags}[api]
                _lib.check(blend(*head, *mid, pix, p(payload), *tail))
                if aux:
                    _lib.check(L.gsr_backward_geom_aux(*head, C.byref(grads), p(inv), p(ws), need, stream))
                else:
                    _lib.check(L.gsr_backward_geom(*head, C.byref(grads), p(ws), need, stream))
            elif api == "plain":
                _lib.check(L.gsr_backward(*head, *mid, pix, C.byref(grads), *tail))
            else:
                whole = L.gsr_backward_aux if api == "aux" else L.gsr_backward_flags
                _lib.check(whole(*head, *mid, pix, C.byref(grads), p(inv), *tail))
        acc = ws[off:off + 64 * N].view(f32).view(N, 16)
        out.update(dL_dcolor=acc[:, 0:3], dL_dmean2D=acc[:, 3:6], dL_dconic=acc[:, 6:10], payload_rows=payload[:3 * N], payload_campos=payload[3 * N:])
        if aux:
            out.update(dL_dinv_depths=inv, dL_dinv_depths_column=acc[:, 11])
        if absgrad:
            out["dL_dmean2D_abs"] = acc[:, 12:14]
        return {k: parity.to_np(v).copy() for k, v in out.items()}

    variants = [(api, split, aux, absgrad) for api in ("plain", "aux", "flags") for split in (False, True)
                for aux in ((False,) if api == "plain" else (False, True)) for absgrad in ((False, True) if api == "flags" else (False,))]
    assert len(variants) == 14
    for api, split, aux, absgrad in variants:
        got, ref = run(api, split, aux, absgrad), reference(aux, absgrad)
        ref = dict(ref, payload_rows=ref["_view_payload"][:3 * N], payload_campos=ref["_view_payload"][3 * N:])
        if aux:
            ref["dL_dinv_depths_column"] = ref["dL_dinv_depths"]
        assert set(got) <= set(ref), set(got) - set(ref)
        for k in got:
            assert np.abs(ref[k]).max() > 0, k
            frac, worst = parity.assert_grad(f"{api} {'split' if split else 'whole'} aux={aux} absgrad={absgrad} {k}", got[k], ref[k])[:2]
            print(f"  {api:5s} {'split' if split else 'whole'} aux={aux!s:5s} absgrad={absgrad!s:5s} {k:22s} {frac:.6f} within the tight band, max err {worst:.2e} max|g|")
