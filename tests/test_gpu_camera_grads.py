"""
Camera gradients (include/gsr_camera_grads.h, backward(camera_grad=True)) and pose refinement on the MI355X.

1. Against float64 (tests/camera_grad_reference.py): dL_dcamera on test_f64_reference.CASE_NAMES and the LARGE cases of
   test_gpu_f64_reference, from colour cotangents alone and from colour + inverse depth + alpha.  Error per entry =
   |kernel - f64| / sum over Gaussians |f64 term| (the per-Gaussian terms cancel in the sum, so |sum| is no scale); an entry
   whose every term is zero must be exactly zero.  Tripwire TRIP = 10x the measured worst case.
2. Nothing else changes: a camera call on a finished backward's workspace leaves every returned array bit-identical; repeated
   calls on the same workspace give identical bits (the sum is reproducible); and the forward's d(colour)/d(direction) hand-over
   and the Sigma3D recompute give the same bits as the coefficients and the forward's cov3D.  Whole backward calls -- dense,
   camera_grad=False, the on_payload halves, sh_gradient="factored", the aux entry and a capacity-mode forward -- agree within
   the float-atomic run-to-run spread of the blend accumulators the camera sum starts from (two plain backward calls already
   differ there), not bit for bit.
3. Empty frames (N = 0, everything culled) give zeros.
4. Pose recovery with frozen Gaussians: Adam on xi alone brings a perturbed camera back to the one that rendered the target.
5. The trainer on Lego with perturbed poses: --optimize-poses lowers the final pose error without raising the training L1.
6. Against the stage-isolated float64 reference (camera_grad_reference.camera_gradient_from_cotangents, fed the kernel's own
   accumulator records and clamped_state; tests/test_camera_grad_split.py shows it is check 1's reference split in two) on
   the case matrix and at the sizes where the kernel pair's structure changes: N = 255 (one partial block), 65 536 / 65 537
   (camera_finish_kernel sums a second row per lane past 256 rows), 262 144 / 262 145 (the grid is capped at 1024 blocks and
   the stride loop takes a second lap), C2, C3 and C5 (5 M, about 19 Gaussians per lane).  Same error measure as check 1, but
   what remains is only the kernel's float32 arithmetic per Gaussian and its float32 lane and wave sums, so the tripwire
   TRIP_ISOLATED is tighter than TRIP.
7. One Gaussian at a time, at every structural position of the kernel pair (lane, wave and block edges, finish rows 255 /
   256 / 512 / 768, both ends of every lap of the stride loop, N - 1) on a 262 145-Gaussian frame and a C5 frame: unit-scale
   random cotangents in the accumulator records and a copy of radii that is zero except at the chosen Gaussians, so the
   kernel's output is that one Gaussian's term, checked against the reference's term (TRIP_TERM, relative to the largest
   entry of the term's view / proj / campos block).  A dropped or duplicated term is an error of 1 there.  Then all chosen
   Gaussians together, and all-zero radii (exact zeros).  The forward's smallest radius is 3 (the 0.3 blur), so a few
   Gaussians carry radius 1 in the copy: the kernel's visibility test is radius > 0.  The camera call on the full frame is
   also bitwise reproducible at these sizes (check 2's assertion at C3).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, render_kwargs, sub
import camera_grad_reference as CG
import parity
import test_f64_reference as R
import test_gpu_f64_reference as G

pytestmark = pytest.mark.gpu

# check 1: max over the 35 entries of |kernel - f64| / sum |f64 term|, worst case over every case and both inputs, measured on
# the MI355X (16x16_n1, colour + depth + alpha; every other case below 6.5e-5); TRIP = 10x
MEASURED = 8.9e-5
TRIP = 10.0 * MEASURED
# check 6: max over the entries of |kernel - isolated f64| / sum |f64 term|, worst case over the case matrix, the large cases and
# every size, both inputs, measured on the MI355X: 3.73e-5 (200x136_n700, colour + depth + alpha, worst of nine runs: its blend
# cotangents are float-atomic sums that largely cancel, so they and the conditioning of its terms change from run to run,
# 8.6e-6 to 3.73e-5; every other case below 6.1e-6 and steady, every size from n255 to C5 below 1.0e-6, C5 1.5e-7);
# TRIP_ISOLATED = 10x, 2.4x tighter than TRIP
MEASURED_ISOLATED = 3.73e-5
TRIP_ISOLATED = 10.0 * MEASURED_ISOLATED
# check 7: one Gaussian's term, max |kernel - f64| over each block (view, proj, campos) / max |f64| over that block, worst case
# over every chosen index of both frames, measured on the MI355X: 7.3e-7 (C5, Gaussian 63, campos; the 262 145 frame 3.9e-7);
# TRIP_TERM = 10x.  All chosen Gaussians together: 2.6e-7 of sum |term| (C5), held to TRIP_ISOLATED.
MEASURED_TERM = 7.3e-7
TRIP_TERM = 10.0 * MEASURED_TERM
# check 2 (whole calls), relative to max |camera gradient| of the dense call: two dense calls differ by up to 6.2e-7 at C3 and the
# other paths by up to 6.7e-7 from the dense one (float-atomic order of the blend accumulators); the floor is 10x that
SPREAD_FLOOR = 7e-6


def _grads(H, W, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32), (rng.normal(0, 1, (H, W)) / (H * W)).astype(np.float32),
            (rng.normal(0, 1, (H, W)) / (H * W)).astype(np.float32))


def _bkw(sc, cam, kw, buf, dpix):
    b = backward_kwargs(sc, cam, kw, buf, dpix)
    b["geom_buffer"] = dict(b["geom_buffer"], depths=buf["depths"])
    return b


def _cam36(g):
    return torch.cat([g["dL_dviewmatrix"].reshape(-1), g["dL_dprojmatrix"].reshape(-1), g["dL_dcampos"],
                      torch.zeros(1, device=g["dL_dcampos"].device)]).cpu().double().numpy()


@pytest.mark.parametrize("name", R.CASE_NAMES + list(G.LARGE))
def test_camera_gradient_against_f64(oracle, cameras, name):
    gsr = pkg()
    c = G._case(oracle, cameras, name)
    sc, cam, kw = c["sc"], c["cam"], c["kw"]
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, gA = _grads(H, W, 17)
    _, _, buf = gsr.render_gaussians(**kw)
    lists = {k: parity.to_np(buf[k]) for k in ("radii", "point_list", "ranges")}
    worst = {}
    for label, (p, d, a) in {"colour": (dpix, None, None), "all": (dpix, gD, gA)}.items():
        g = gsr.backward(**_bkw(sc, cam, kw, buf, p), dL_ddepth_image=d, dL_dalpha_image=a, camera_grad=True)
        got = _cam36(g)
        ref, scale = CG.camera_gradient_f64(sc, kw, lists["radii"], lists["point_list"], lists["ranges"], p, d, a)
        zero = scale == 0
        assert not np.any(got[zero]), (label, np.where(zero & (got != 0))[0])
        err = np.abs(got - ref)[~zero] / scale[~zero]
        worst[label] = float(err.max()) if err.size else 0.0
        assert np.isfinite(got).all()
    print(f"\n{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= TRIP, worst


# ------------------------------------------------------------------------------------------------ check 2: nothing else changes
def _c3_frame(n=None, W=None, H=None):
    gsr = pkg()
    cfg = dict(gsr.scenes.CONFIGS["C3"])
    W, H = W or cfg["width"], H or cfg["height"]
    sc = gsr.scenes.synthetic_scene(n or cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    return sc, cam, render_kwargs(sc, cam, width=W, height=H, bg=(0.1, 0.2, 0.3))


def _direct_camera_call(sc, kw, buf, g, sh_dir=None, cov3D=None):
    """gsr_backward_camera on the workspace of the backward() call that returned `g` (its accumulator columns are views of it)."""
    _lib, _host = sub("_lib"), sub("_host")
    L = _lib.lib()
    dev = g["dL_dcolor"].device
    t = lambda a, shape: torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).to(dev)
    N = int(np.asarray(sc["means"]).reshape(-1, 3).shape[0])
    means, scales, rots = t(sc["means"], (N, 3)), t(sc["scales"], (N, 3)), t(sc["rotations"], (N, 4))
    op, shs = t(sc["opacities"], (N,)), t(sc["shs"], (N * 16, 3))
    scene = _lib.GsrScene(N, _host.ptr(means), _host.ptr(scales), _host.ptr(rots), _host.ptr(op), _host.ptr(shs), int(kw["degree"]),
                          float(kw["scale_modifier"]), 1)
    cam = _host.make_camera(kw["viewmatrix"], kw["projmatrix"], kw["campos"], kw["background"], kw["tan_fovx"], kw["tan_fovy"],
                            kw["image_width"], kw["image_height"])
    geom = _lib.GsrGeom(_host.ptr(buf["radii"]), None, None, None, None, _host.ptr(cov3D), None, None, _host.ptr(buf["clamped_state"]),
                        None, _host.ptr(sh_dir))
    off = int(L.gsr_backward_accumulators_offset(N))
    ws_ptr = g["dL_dcolor"].data_ptr() - off
    ws_bytes = int(L.gsr_backward_workspace_bytes(N, 0, kw["image_width"], kw["image_height"]))
    out = torch.full((36,), float("nan"), device=dev)
    scratch = torch.empty(int(L.gsr_backward_camera_scratch_bytes(N)), dtype=torch.uint8, device=dev)
    _lib.check(L.gsr_backward_camera(C.byref(scene), C.byref(cam), C.byref(geom), _host.ptr(out), ws_ptr, ws_bytes, _host.ptr(scratch),
                                     scratch.numel(), _host.raw_stream(dev)))
    torch.cuda.synchronize()
    return out.cpu().double().numpy()


def _snapshot(g):
    return {k: v.clone() for k, v in g.items() if isinstance(v, torch.Tensor)}


def test_camera_call_changes_nothing_else_and_is_reproducible():
    gsr = pkg()
    sc, cam, kw = _c3_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, _ = _grads(H, W, 2)
    for aux in (None, gD):
        g = gsr.backward(**_bkw(sc, cam, kw, buf, dpix), dL_ddepth_image=aux, camera_grad=True)
        assert {"dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"} <= set(g)
        assert g["dL_dviewmatrix"].shape == (4, 4) and g["dL_dprojmatrix"].shape == (4, 4) and g["dL_dcampos"].shape == (3,)
        assert all(g[k].dtype == torch.float32 and g[k].is_cuda for k in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"))
        torch.cuda.synchronize()
        first = _cam36(g)
        before = _snapshot(g)
        keys = [k for k in parity.GRAD_KEYS if g.get(k) is not None] + (["dL_dinv_depths"] if aux is not None else [])
        assert len(keys) >= 9 if aux is not None else len(keys) >= 8
        # the same workspace again, three times, through every geometry source the kernel has: the same bits each time
        sh_dir = buf["clamped_state"]._gsr_sh_dir[0] if getattr(buf["clamped_state"], "_gsr_sh_dir", None) else None
        runs = [_direct_camera_call(sc, kw, buf, g), _direct_camera_call(sc, kw, buf, g, cov3D=buf["cov3Ds"])]
        if sh_dir is not None:
            runs.append(_direct_camera_call(sc, kw, buf, g, sh_dir=sh_dir, cov3D=buf["cov3Ds"]))
        for r in runs:
            assert np.array_equal(r, first), np.abs(r - first).max()
        for k in keys:
            assert torch.equal(g[k], before[k]), k
        assert np.abs(first).max() > 0


def test_camera_grad_keyword_leaves_the_other_outputs_alone():
    """camera_grad=True runs the camera pair after the backward's own launches: the other keys are those of the call without it,
    up to the blend accumulators' float-atomic spread (two calls without it differ by that much too)."""
    gsr = pkg()
    sc, cam, kw = _c3_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    dpix, _, _ = _grads(kw["image_height"], kw["image_width"], 5)
    raw = gsr.backward(**_bkw(sc, cam, kw, buf, dpix))
    keys = set(raw)
    plain, plain2 = _snapshot(raw), _snapshot(gsr.backward(**_bkw(sc, cam, kw, buf, dpix)))
    withc = gsr.backward(**_bkw(sc, cam, kw, buf, dpix), camera_grad=True)
    assert set(withc) == keys | {"dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"}
    for k in parity.GRAD_KEYS:
        if plain.get(k) is None:
            continue
        x, y, z = (t[k].double() for t in (withc, plain, plain2))
        scale = max(float(y.abs().max()), 1e-30)
        err, spread = float((x - y).abs().max()) / scale, float((z - y).abs().max()) / scale
        assert err <= max(3.0 * spread, 8e-4), (k, err, spread)


def test_every_backward_path_gives_the_same_camera_gradient():
    gsr = pkg()
    fwd = sub("forward")
    sc, cam, kw = _c3_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, gA = _grads(H, W, 6)
    for aux in ({}, {"dL_ddepth_image": gD, "dL_dalpha_image": gA}):
        dense = _cam36(gsr.backward(**_bkw(sc, cam, kw, buf, dpix), camera_grad=True, **aux))
        dense2 = _cam36(gsr.backward(**_bkw(sc, cam, kw, buf, dpix), camera_grad=True, **aux))
        scale = np.abs(dense).max()
        spread = np.abs(dense2 - dense).max() / scale
        got = []
        paths = {"factored": _cam36(gsr.backward(**_bkw(sc, cam, kw, buf, dpix), camera_grad=True, sh_gradient="factored", **aux)),
                 "halves": _cam36(gsr.backward(**_bkw(sc, cam, kw, buf, dpix), camera_grad=True, sh_gradient="factored",
                                               on_payload=got.append, **aux))}
        assert len(got) == 1
        D = int(buf["point_list"].shape[0])
        _, _, cbuf = fwd.render_gaussians(**kw, capacity=D, capacity_hint=D)
        paths["capacity"] = _cam36(gsr.backward(**_bkw(sc, cam, kw, cbuf, dpix), camera_grad=True, **aux))
        if not aux:
            z = np.zeros((H, W), np.float32)
            paths["aux_zero"] = _cam36(gsr.backward(**_bkw(sc, cam, kw, buf, dpix), camera_grad=True, dL_ddepth_image=z))
        print(f"\naux={bool(aux)}: dense vs dense {spread:.2e}, " + ", ".join(f"{k} {np.abs(v - dense).max() / scale:.2e}"
                                                                               for k, v in paths.items()))
        for k, v in paths.items():
            assert np.abs(v - dense).max() / scale <= max(3.0 * spread, SPREAD_FLOOR), k


def test_empty_frames_give_zeros():
    gsr = pkg()
    sc, cam, kw = _c3_frame(n=3000, W=64, H=48)
    empty = {k: np.asarray(v)[:0] for k, v in sc.items()}
    kw0 = render_kwargs(empty, cam, width=64, height=48)
    _, _, b0 = gsr.render_gaussians(**kw0)
    g0 = gsr.backward(**_bkw(empty, cam, kw0, b0, np.ones((48, 64, 3), np.float32)), camera_grad=True)
    assert not np.any(_cam36(g0)) and g0["dL_dviewmatrix"].shape == (4, 4)
    behind = dict(sc)                                                       # every Gaussian behind the camera: all culled, D = 0
    c = np.asarray(cam["camera_center"], np.float32)
    fwd_dir = np.asarray(cam["world_to_camera"], np.float64)[:3, 2]
    behind["means"] = (c - 3.0 * fwd_dir + 0.1 * np.asarray(sc["means"])).astype(np.float32)
    kw1 = render_kwargs(behind, cam, width=64, height=48)
    _, _, b1 = gsr.render_gaussians(**kw1)
    assert int(parity.to_np(b1["radii"]).max()) == 0 and int(b1["point_list"].shape[0]) == 0
    dpix = np.ones((48, 64, 3), np.float32)
    g1 = gsr.backward(**_bkw(behind, cam, kw1, b1, dpix), dL_ddepth_image=np.ones((48, 64), np.float32), camera_grad=True)
    assert not np.any(_cam36(g1))


# ------------------------------------------------------------------------------- check 6: against the isolated f64 reference
# name -> (scene config, N): the sizes where the kernel pair's structure changes, on C3's scene statistics unless named
SIZES = {"n255": ("C3", 255), "n65536": ("C3", 65536), "n65537": ("C3", 65537), "n262144": ("C3", 262144),
         "n262145": ("C3", 262145), "C2": ("C2", None), "C3": ("C3", None), "C5": ("C5", None)}
LAP = 1024 * 256     # lanes of the capped grid (GSR_CAMERA_MAX_BLOCKS blocks of 256): one lap of the stride loop
GROUPS = (slice(0, 16), slice(16, 32), slice(32, 36))   # view, proj, campos (+ the zero entry 35)


def _frame(name):
    gsr = pkg()
    cfg_name, n = SIZES[name]
    cfg = gsr.scenes.CONFIGS[cfg_name]
    W, H = cfg["width"], cfg["height"]
    sc = gsr.scenes.synthetic_scene(n or cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    cam = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    return sc, cam


def _records(g):
    """The (N, 16) float32 accumulator records of the workspace that `g` (a backward() result) returned views of."""
    c = g["dL_dcolor"]
    assert c.stride() == (16, 1), c.stride()
    return c.as_strided((c.shape[0], 16), (16, 1))


def _isolated_f64(sc, kw, radii, clamped, rec):
    """The isolated reference on the kernel's own cotangents (GradRec slots 0-2, 3-4, 6-9, 11)."""
    return CG.camera_gradient_from_cotangents(sc, kw, radii, clamped, rec[:, 3:5], rec[:, 6:10], rec[:, 0:3], rec[:, 11])


def _isolated_error(got, ref, scale, what):
    zero = scale == 0
    assert not np.any(got[zero]), (what, np.where(zero & (got != 0))[0])
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)[~zero] / scale[~zero]
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("name", R.CASE_NAMES + list(G.LARGE) + list(SIZES))
def test_camera_gradient_against_isolated_f64(oracle, cameras, name):
    gsr = pkg()
    if name in SIZES:
        sc, cam = _frame(name)
        kw = render_kwargs(sc, cam, width=cam["width"], height=cam["height"], bg=(0.1, 0.2, 0.3))
    else:
        c = G._case(oracle, cameras, name)
        sc, cam, kw = c["sc"], c["cam"], c["kw"]
    H, W = kw["image_height"], kw["image_width"]
    N = int(np.asarray(sc["means"]).reshape(-1, 3).shape[0])
    dpix, gD, gA = _grads(H, W, 19)
    _, _, buf = gsr.render_gaussians(**kw)
    radii, clamped = parity.to_np(buf["radii"]), parity.to_np(buf["clamped_state"])
    n_vis = int((radii > 0).sum())
    worst = {}
    for label, (p, d, a) in {"colour": (dpix, None, None), "all": (dpix, gD, gA)}.items():
        g = gsr.backward(**_bkw(sc, cam, kw, buf, p), dL_ddepth_image=d, dL_dalpha_image=a, camera_grad=True)
        got = _cam36(g)
        rec = _records(g).cpu().numpy()
        del g
        ref, scale = _isolated_f64(sc, kw, radii, clamped, rec)
        worst[label] = _isolated_error(got, ref, scale, label)
    print(f"\n{name} (N {N}, visible {n_vis}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert n_vis > 0
    assert max(worst.values()) <= TRIP_ISOLATED, worst


# --------------------------------------------------------------------------------------- check 7: one Gaussian at a time
def _structural_indices(N):
    """Lane / wave / block edges, the finish kernel's row edges (256 rows per pass), both ends of every lap of the stride
    loop, and N - 1."""
    nblk = min(-(-N // 256), 1024)
    lap = nblk * 256
    idx = {0, 63, 64, 255, 256, 65535, 65536, 131071, 131072, 196607, 196608, 262143, 262144, 262145, N - 1}
    for start in range(0, N, lap):
        idx |= {start, min(start + lap, N) - 1}
    return sorted(i for i in idx if 0 <= i < N)


@pytest.mark.parametrize("name", ["n262145", "C5"])
def test_camera_gradient_one_gaussian_at_a_time(name):
    gsr = pkg()
    sc, cam = _frame(name)
    N = int(sc["means"].shape[0])
    assert N > LAP
    idx = _structural_indices(N)
    ones = idx[1::4]                                                # these carry radius 1 in the copy
    rng = np.random.default_rng(41)
    sc = {k: np.array(v) for k, v in sc.items()}                    # the chosen Gaussians, moved into the middle of the view
    sc["means"][idx] = rng.uniform(-0.5, 0.5, (len(idx), 3)).astype(np.float32)
    sc["scales"][idx] = rng.uniform(0.01, 0.05, (len(idx), 3)).astype(np.float32)
    sc["opacities"][idx] = 0.5
    W, H = cam["width"], cam["height"]
    kw = render_kwargs(sc, cam, width=W, height=H, bg=(0.1, 0.2, 0.3))
    _, _, buf = gsr.render_gaussians(**kw)
    radii = buf["radii"]
    r_np, clamped = parity.to_np(radii), parity.to_np(buf["clamped_state"])
    assert (r_np[idx] > 0).all(), [i for i in idx if r_np[i] <= 0]
    dpix, _, _ = _grads(H, W, 8)
    g = gsr.backward(**_bkw(sc, cam, kw, buf, dpix), camera_grad=True)
    torch.cuda.synchronize()
    whole = _cam36(g)
    # check 2 at this size: the same workspace again gives the same bits
    for _ in range(2):
        again = _direct_camera_call(sc, kw, buf, g)
        assert np.array_equal(again, whole), np.abs(again - whole).max()
    # unit-scale random cotangents in every slot the camera kernel reads
    rec = _records(g)
    cols = [0, 1, 2, 3, 4, 6, 7, 9, 11]
    rec[:, cols] = torch.as_tensor(rng.normal(0.0, 1.0, (N, len(cols))).astype(np.float32)).to(rec.device)
    torch.cuda.synchronize()
    rec_np = rec.cpu().numpy()

    def only(chosen):
        m = torch.zeros_like(radii)
        if chosen:
            sel = torch.as_tensor(chosen, device=radii.device)
            m[sel] = radii[sel]
            one = [i for i in chosen if i in ones]
            if one:
                m[torch.as_tensor(one, device=radii.device)] = 1
        return m

    worst, where = 0.0, None
    for i in idx:
        m = only([i])
        got = _direct_camera_call(sc, kw, dict(buf, radii=m), g)
        ref, scale = _isolated_f64(sc, kw, parity.to_np(m), clamped, rec_np)
        assert not np.any(got[scale == 0]), (i, np.where((scale == 0) & (got != 0))[0])
        for s in GROUPS:
            top = np.abs(ref[s]).max()
            if top == 0:        # campos when every channel is clamped: the exact-zero check above covers it
                continue
            e = float(np.abs(got[s] - ref[s]).max() / top)
            if e > worst:
                worst, where = e, (i, s.start)
        assert worst <= TRIP_TERM, (name, i, worst, where, got, ref)
    m = only(idx)
    got = _direct_camera_call(sc, kw, dict(buf, radii=m), g)
    together = _isolated_error(got, *_isolated_f64(sc, kw, parity.to_np(m), clamped, rec_np), "chosen together")
    zeros = _direct_camera_call(sc, kw, dict(buf, radii=torch.zeros_like(radii)), g)
    print(f"\n{name} (N {N}): {len(idx)} Gaussians, one at a time worst {worst:.2e} (index, block {where}), together "
          f"{together:.2e}")
    assert not np.any(zeros)
    assert together <= TRIP_ISOLATED, together


# --------------------------------------------------------------------------------------------------- check 4: pose recovery
# start / final error after 200 Adam steps: measured 2.9x (rotation, 2.0 -> 0.68 deg) and 3.5x (translation); bounds at half
POSE_ROT_GAIN_MIN = 1.45
POSE_TRANS_GAIN_MIN = 1.75


def test_pose_recovery_with_frozen_gaussians():
    gsr = pkg()
    pose = gsr.pose
    W = H = 256
    sc = gsr.scenes.synthetic_scene(20000, 0.03, 0.5, seed=12)
    cam0 = gsr.cameras.nerf_camera(gsr.scenes.LEGO_FRAME0, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    kw0 = render_kwargs(sc, cam0, width=W, height=H, bg=(0.0, 0.0, 0.0))
    target = gsr.render_gaussians(**kw0)[0].reshape(H, W, 3).clone()
    dist = float(np.linalg.norm(cam0["camera_center"]))
    start = pose.apply_pose_delta(cam0, pose.random_pose_delta(np.random.default_rng(3), 2.0, 0.03 * dist))
    xi, m, v = np.zeros(6), np.zeros(6), np.zeros(6)
    lr = 2e-3
    for it in range(200):
        c = pose.apply_pose_delta(start, xi)
        kw = render_kwargs(sc, c, width=W, height=H, bg=(0.0, 0.0, 0.0))
        img, _, buf = gsr.render_gaussians(**kw)
        dpix = (2.0 / (H * W * 3)) * (img.reshape(H, W, 3) - target)          # mean squared error
        g = gsr.backward(**_bkw(sc, c, kw, buf, dpix), camera_grad=True)
        gx = pose.pose_gradient(start, xi, g["dL_dviewmatrix"], g["dL_dprojmatrix"], g["dL_dcampos"])
        m = 0.9 * m + 0.1 * gx
        v = 0.999 * v + 0.001 * gx * gx
        xi = xi - lr * (m / (1 - 0.9 ** (it + 1))) / (np.sqrt(v / (1 - 0.999 ** (it + 1))) + 1e-15)
    r0, t0 = pose.pose_error(start, cam0)
    r1, t1 = pose.pose_error(pose.apply_pose_delta(start, xi), cam0)
    print(f"\npose recovery: rotation {r0:.4f} -> {r1:.4f} deg ({r0 / max(r1, 1e-12):.1f}x), translation {t0:.5f} -> {t1:.5f} "
          f"({t0 / max(t1, 1e-12):.1f}x)")
    assert r1 * POSE_ROT_GAIN_MIN <= r0 and t1 * POSE_TRANS_GAIN_MIN <= t0, (r0, r1, t0, t1)


# ------------------------------------------------------------------------------------------------------- check 5: the trainer
# relative drop of the final mean pose error with --optimize-poses, measured 0.29 (rotation, 1.0 -> 0.71 deg) and 0.18
# (translation, 0.050 -> 0.041); bounds at half.  The training L1 fell (0.0682 -> 0.0648) and may not rise.
TRAIN_ROT_GAIN_MIN = 0.145
TRAIN_TRANS_GAIN_MIN = 0.089


def _train(tmp_path, tag, *extra):
    log = tmp_path / f"{tag}.jsonl"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--log", str(log), "--print-interval", "1000", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    for line in open(log):
        rec = json.loads(line)
        if rec["record"] == "summary":
            return rec


def test_trainer_pose_refinement_on_lego(tmp_path):
    base = ["--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8", "--iterations", "300", "--pose-noise-deg", "1",
            "--pose-noise-trans", "0.05"]
    off = _train(tmp_path, "off", *base)
    on = _train(tmp_path, "on", *base, "--optimize-poses")
    for s in (off, on):
        assert len(s["pose_error_start"]["rot_deg"]) == 8 and len(s["pose_error_final"]["trans"]) == 8
    assert off["pose_rot_deg_mean_start"] == on["pose_rot_deg_mean_start"] and abs(off["pose_rot_deg_mean_start"] - 1.0) < 1e-3
    assert off["pose_rot_deg_mean_final"] == off["pose_rot_deg_mean_start"]
    rot_gain = 1.0 - on["pose_rot_deg_mean_final"] / off["pose_rot_deg_mean_final"]
    trans_gain = 1.0 - on["pose_trans_mean_final"] / off["pose_trans_mean_final"]
    print(f"\nlego pose refinement: rotation {off['pose_rot_deg_mean_final']:.4f} -> {on['pose_rot_deg_mean_final']:.4f} deg "
          f"(gain {rot_gain:.3f}), translation {off['pose_trans_mean_final']:.5f} -> {on['pose_trans_mean_final']:.5f} (gain "
          f"{trans_gain:.3f}); train L1 {off['train_l1_mean']:.5f} -> {on['train_l1_mean']:.5f}; it/s {off['iterations_per_s']} -> "
          f"{on['iterations_per_s']}")
    assert rot_gain >= TRAIN_ROT_GAIN_MIN and trans_gain >= TRAIN_TRANS_GAIN_MIN, (rot_gain, trans_gain)
    assert on["train_l1_mean"] <= off["train_l1_mean"]
