"""
The Gaussians' normals, their image, its gradient stage and the consistency term (csrc/normal_render.hip,
include/gsr_normal_render.h) on the MI355X, against the float64 yardstick and the float32 restatement of
tests/normal_render_reference.py, both taken on the KERNEL forward's own buffers.

Frames: the four small scenes of the CPU matrix, the toy scene at 120x90, one Gaussian over 40x40, and the second scene antialiased,
under the 3D filter and in capacity mode; for (a) and (b) N = 1, 63, 64, 65 and 257 with ties, non-unit and zero quaternions mixed in.

  (a)  against float64: the normals within 3 E_f32 + eps32 on the decided Gaussians (which holds c* and sigma: a wrong axis or side is
       an error of order 1), the zero quaternion exactly 0;
  (b)  distortion_reference.criterion per row in the scale of normal_render_reference.vjp_f64; the kernel ADDS; the same bits twice;
  (c)  bit-identical to features.render_features(n) at C = 3; the same bits across two calls, two streams, with and without block
       masks; every pixel written, over a poisoned output;
  (d)  criterion(E_kernel, E_f32, E_spread, floor) per output: E_f32 the CPU-recorded restatement error of the frame
       (tests/golden/normal_render_margins.json; for the three n2000 variants, which the CPU matrix does not have, the restatement's
       error on the frame's own buffers), E_spread two runs' difference, floor the smallest CPU E_f32;
       three cross-checks under the same criterion with the existing calls' own two-run spread added: dL_dgaussian_normals against
       features.render_features_backward(G), columns 3, 4, 6, 7, 9, 10 against the existing backward(rgb=n, background=0,
       dL_dpixels=G), the untouched columns bit-equal to the plain call's;
  linearity of the arena per segment, as test_gpu_distortion.test_arena_is_linear_in_the_two_cotangents;
  camera_grad, sh_gradient="factored", normal_param_grad=False and dL_dnormal_image alone against the dense call;
  (e)  sums and the three gradients against float64 within the restatement's error, the same bits every call;
  the trainer, three starts (see NC_* below).

Every measured figure is printed as a NORMAL_RENDER_ROW JSON line; tools/record_normal_render_margins.py files the E_kernel of a run in
tests/golden/normal_render_margins.json, as a record only.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, lego_camera, pkg, sub
import blend_grad_reference as B
import frame_walk_reference as FWR
import features_reference as FR
import normal_render_reference as NR
import parity
from test_gpu_features import _case

pytestmark = pytest.mark.gpu
FRAMES = list(FR.SCENES) + ["toy", "one_gaussian_40x40", "n2000_antialiased", "n2000_filter3d", "n2000_capacity"]
_FRAMES = {}


def _row(**kw):
    print("\nNORMAL_RENDER_ROW " + json.dumps(kw))


def _bwd_extra(extra):
    return {k: v for k, v in extra.items() if k in ("rasterize_mode", "filter_3d")}


def _dev(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def frame(name):
    """The kernel forward of a frame (background 0), the kernel's normals, G, and the yardstick and restatement on its buffers, once
    per session."""
    if name not in _FRAMES:
        gsr = pkg()
        nr = sub("normal_render")
        sc, cam, kw, extra = _case(name)
        H, W = kw["image_height"], kw["image_width"]
        image, inv_depth, buf = gsr.render_gaussians(**kw, **extra)
        dev = image.device
        nb = {k: parity.to_np(buf[k]) for k in ("points_xy_image", "conic_opacity", "depths", "point_list", "ranges", "n_contrib")}
        if "capacity" in extra:
            D, over = sub("forward").rendered_count(buf)
            assert not over and 0 < D < extra["capacity"]
            nb["point_list"] = nb["point_list"][:D]
        N = sc["means"].shape[0]
        view = np.asarray(kw["viewmatrix"], np.float32)
        n = nr.gaussian_normals(_dev(sc["scales"], dev), _dev(sc["rotations"], dev), _dev(sc["means"], dev), view)
        n32 = parity.to_np(n)
        r = NR.yardstick(nb, W, H, n32, NR.draw_G(H, W))
        print(f"\n{name}: D {nb['point_list'].shape[0]}, {int(r['mask'].sum())} of {r['mask'].size} pixels masked")
        assert r["mask"].sum() <= FR.MAX_MASKED * r["mask"].size
        G32 = r["G"].astype(np.float32)                              # zero at the masked pixels: both sides lose them
        img32 = NR.render_f32(nb, W, H, n32)
        acc32, dn32 = NR.render_backward_f32(nb, W, H, n32, G32, img32)
        _FRAMES[name] = dict(sc=sc, cam=cam, kw=kw, extra=extra, H=H, W=W, N=N, buf=buf, nb=nb, r=r, G=G32, img32=img32, acc32=acc32, dn32=dn32,
                             n=n, n32=n32, view=view, Gd=_dev(G32, dev), dev=dev)
    return _FRAMES[name]


def _accumulators(g, N):
    """The (N, 16) accumulator rows of a backward() result, through the tag densify.DensifyStats.update uses."""
    ws = g["dL_dmean2D"]._gsr_backward_ws[0]
    off = int(sub("_lib").lib().gsr_backward_accumulators_offset(N))
    return ws[off:off + 64 * N].view(torch.float32).view(N, 16)


def _backward(f, dpix=None, G=None, nimg=None, **more):
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], dpix)
    if G is not None:
        kw.update(dL_dnormal_image=G, gaussian_normals=f["n"], normal_image=nimg)
    return pkg().backward(**kw, **_bwd_extra(f["extra"]), **more)


def _e_f32(name, f):
    """The restatement's errors the criterion uses: the CPU record of the frame, or for a frame the CPU matrix does not have the
    restatement's errors on the frame's own buffers."""
    rec = NR.golden()["E_f32"].get(name)
    if rec is not None:
        return {k: rec[k] for k in NR.OUTPUTS}, "recorded"
    return NR.backward_errors(f["acc32"], f["dn32"], f["r"]), "on the frame's buffers"


# ---- (a), (b) ----
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_gaussian_normals_and_backward_against_float64(N):
    nr = sub("normal_render")
    dev = torch.device("cuda", torch.cuda.current_device())
    view = np.asarray(lego_camera(sub("cameras"), 0, width=50, height=37)["world_to_camera"], np.float32)
    s, q, p = NR.draw_gaussians(N)
    sd, qd, pd = _dev(s, dev), _dev(q, dev), _dev(p, dev)
    r = NR.normals_f64(s, q, p, view)
    keep = ~r["undecided"]
    assert r["undecided"].mean() <= 0.01
    out = torch.full((N, 3), float("nan"), device=dev)
    n = nr.gaussian_normals(sd, qd, pd, view, out=out)
    assert n is out and torch.equal(n, nr.gaussian_normals(sd, qd, pd, {"world_to_camera": view}))
    nk = parity.to_np(n)
    n32, c32, sigma32 = NR.normals_f32(s, q, p, view)
    E_k, E_32 = float(np.abs(nk - r["n"])[keep].max()), float(np.abs(n32 - r["n"])[keep].max())
    _row(test="gaussian_normals", N=N, E_kernel=E_k, E_f32=E_32, bit_equal_to_restatement=bool(np.array_equal(nk, n32)))
    assert E_k <= 3.0 * E_32 + NR.EPS32, (E_k, E_32)             # (a wrong c* or sigma is an error of order 1)
    assert not nk[~r["ok"]].any()
    if N > 4:
        assert not r["ok"][4]
    g = np.random.default_rng(9).normal(0, 1, (N, 3)).astype(np.float32)
    dq64, scale, _ = NR.vjp_f64(s, q, p, view, g)
    gd = _dev(g, dev)
    a, b = nr.gaussian_normals_backward(gd, sd, qd, pd, view), nr.gaussian_normals_backward(gd, sd, qd, pd, view)
    assert torch.equal(a, b)                                     # no atomics: the same bits
    E_k = NR.rows_error(parity.to_np(a), dq64, scale, keep)
    E_32 = NR.rows_error(NR.normals_backward_f32(s, q, p, view, g), dq64, scale, keep)
    _row(test="gaussian_normals_backward", N=N, E_kernel=E_k, E_f32=E_32)
    assert FWR.criterion(E_k, E_32, 0.0, 0.5 * NR.EPS32), (E_k, E_32)      # (floor: one rounding of the result in its scale)
    assert not parity.to_np(a)[~r["ok"]].any()
    pre = torch.rand((N, 4), device=dev)
    added = nr.gaussian_normals_backward(gd, sd, qd, pd, view, dL_drot=pre.clone())
    assert torch.equal(added, pre + a)                           # it ADDS: one read-modify-write per Gaussian


# ---- (c) ----
@pytest.mark.parametrize("name", FRAMES + ["behind_n300"])
def test_forward_is_features_at_c3_deterministic_and_writes_every_pixel(name):
    nr, feat = sub("normal_render"), sub("features")
    if name.startswith("behind"):
        sc, cam, kw, extra = _case(name)
        H, W = kw["image_height"], kw["image_width"]
        buf = pkg().render_gaussians(**kw)[2]
        assert int(buf["point_list"].shape[0]) == 0
        dev = buf["ranges"].device
        n = nr.gaussian_normals(_dev(sc["scales"], dev), _dev(sc["rotations"], dev), _dev(sc["means"], dev), np.asarray(kw["viewmatrix"], np.float32))
    else:
        f = frame(name)
        buf, H, W, n, dev = f["buf"], f["H"], f["W"], f["n"], f["dev"]
        if "capacity" not in f["extra"]:
            assert sub("_frame").masks_of(buf, int(buf["point_list"].shape[0]), dev) is not None   # the masks are this forward's
    a = nr.render_normals(n, buf, H, W)
    assert tuple(a.shape) == (H, W, 3) and bool(torch.isfinite(a).all())
    assert torch.equal(a, feat.render_features(n, buf, H, W))          # bit for bit gsr_features_forward at C = 3
    assert torch.equal(a, nr.render_normals(n, buf, H, W))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = nr.render_normals(n, buf, H, W)
    s.synchronize()
    assert torch.equal(a, c)
    assert torch.equal(a, nr.render_normals(n, buf, H, W, use_block_masks=False))
    out = torch.full((H, W, 3), float("nan"), device=dev)
    got = nr.render_normals(n, buf, H, W, out=out)
    assert got is out and torch.equal(out, a)
    if name.startswith("behind"):
        assert not bool(a.any())                                       # a frame without lists: every pixel 0
        G = torch.ones((H, W, 3), device=dev)
        f0 = dict(sc=sc, cam=cam, kw=kw, buf=buf, extra={}, n=n)
        res = _backward(f0, None, G, a)
        assert not bool(res["dL_dgaussian_normals"].any()) and not bool(res["dL_dmean3D"].any()) and not bool(res["dL_drot"].any())
        return
    r = f["r"]
    E_k, E_32 = NR.image_error(a, r), NR.image_error(f["img32"], r)
    _row(test="forward", case=name, E_kernel=E_k, E_f32=E_32)
    assert E_k <= 3.0 * E_32 + NR.EPS32, (E_k, E_32)
    assert float(a.norm(dim=-1).max()) <= 1.0 + 1e-5                   # at most the coverage


# ---- (d) ----
def _runs(f, nimg, n_runs=2):
    runs = []
    for _ in range(n_runs):
        res = _backward(f, None, f["Gd"], nimg, normal_param_grad=False)
        acc = _accumulators(res, f["N"]).clone()
        assert tuple(res["dL_dgaussian_normals"].shape) == (f["N"], 3) and "dL_dinv_depths" in res
        assert not bool(acc[:, list(NR.UNTOUCHED)].any())             # G alone: the other columns are what a zero image leaves
        assert bool(torch.isfinite(res["_arena"]).all())
        runs.append((parity.to_np(acc), parity.to_np(res["dL_dgaussian_normals"])))
    return runs


@pytest.mark.parametrize("name", FRAMES)
def test_backward_against_float64(name):
    nr = sub("normal_render")
    f = frame(name)
    H, W, N, r = f["H"], f["W"], f["N"], f["r"]
    nimg = nr.render_normals(f["n"], f["buf"], H, W)
    E32, source = _e_f32(name, f)
    runs = _runs(f, nimg)
    Ek = {k: max(NR.backward_errors(a, d, r)[k] for a, d in runs) for k in NR.OUTPUTS}
    E_s = NR.spread(runs[0], runs[1], r)
    floor = NR.golden()["floor"]
    _row(test="backward", case=name, E_kernel=Ek, E_f32=E32, E_f32_source=source, E_spread=E_s, floor=floor,
         E_f32_here=NR.backward_errors(f["acc32"], f["dn32"], r))
    for k in NR.OUTPUTS:
        assert FWR.criterion(Ek[k], E32[k], E_s, floor), (k, Ek[k], E32[k], E_s)
    assert all(np.abs(runs[0][0][:, c]).max() > 0 for c in NR.TOUCHED) and np.abs(runs[0][1]).max() > 0


@pytest.mark.parametrize("name", ["n300_50x37", "n2000_64x48", "n1500_opaque_48x48", "n2000_antialiased"])
def test_backward_cross_checks_against_the_existing_calls(name):
    """Three independent routes to the stage's outputs, none of which runs the new backward kernel."""
    nr, feat = sub("normal_render"), sub("features")
    f = frame(name)
    H, W, N, r = f["H"], f["W"], f["N"], f["r"]
    nimg = nr.render_normals(f["n"], f["buf"], H, W)
    E32, _ = _e_f32(name, f)
    floor = NR.golden()["floor"]
    runs = _runs(f, nimg)
    E_s = NR.spread(runs[0], runs[1], r)
    # 1. dL/d(normals) is the transposed feature sum of G
    fb = [parity.to_np(feat.render_features_backward(f["Gd"], f["buf"], H, W)).astype(np.float64) for _ in range(2)]
    sc = r["dL_dnormals"]["scale"]
    sel = sc > 0
    s_feat = float((np.abs(fb[0] - fb[1])[sel] / sc[sel]).max()) if sel.any() else 0.0
    d = float((np.abs(runs[0][1] - fb[0])[sel] / sc[sel]).max())
    assert not np.abs(runs[0][1])[~sel].any() and not np.abs(fb[0])[~sel].any()
    _row(test="cross_features_backward", case=name, difference=d, E_f32=E32["dL_dnormals"], spread=E_s + s_feat)
    assert FWR.criterion(d, E32["dL_dnormals"], E_s + s_feat, floor), (d, E_s, s_feat)
    # 2. the six columns are what the existing backward adds for colour := the normals, background 0, dL_dpixels = G
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], f["Gd"])
    kw.update(rgb=f["n"], background=np.zeros(3, np.float32), geom_buffer=dict(kw["geom_buffer"], rgb=f["n"]))
    old = []
    for _ in range(2):
        res = pkg().backward(**kw, **_bwd_extra(f["extra"]))
        old.append((parity.to_np(_accumulators(res, N).clone()), parity.to_np(res["dL_dcolor"]).copy()))
    assert not pkg().backward.last_call_used_forward_records          # (a copy of the frame: the colours are not the forward's)
    s_old = NR.spread(old[0], old[1], r)
    worst = {}
    for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity"):
        scale = r[k]["scale"]
        sel = scale > 0
        worst[k] = float((np.abs(NR.layout(*runs[0], k) - NR.layout(*old[0], k))[sel] / scale[sel]).max())
        assert FWR.criterion(worst[k], E32[k], E_s + s_old, floor), (k, worst[k], E32[k], E_s, s_old)
    _row(test="cross_existing_backward", case=name, difference=worst, spread=E_s + s_old)
    # 3. the untouched columns are bit for bit the plain call's (no colour cotangent: a zero alpha image alone)
    plain = _backward(f, None, dL_dalpha_image=torch.zeros((H, W), device=f["dev"]))
    cols = list(NR.UNTOUCHED)
    assert np.array_equal(parity.to_np(_accumulators(plain, N))[:, cols], runs[0][0][:, cols])


GRAD_KEYS = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dshs")


def _dpix(H, W, seed=3):
    return (np.random.default_rng(seed).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)


def _arena_norm(x, y, offsets, ref):
    worst = 0.0
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        m = np.abs(ref[lo:hi]).max()
        if m > 0:
            worst = max(worst, float(np.abs(x[lo:hi] - y[lo:hi]).max() / m))
    return worst


@pytest.mark.parametrize("name", ["n2000_64x48", "n2000_filter3d"])
def test_arena_is_linear_in_the_two_cotangents(name):
    """As test_gpu_distortion.test_arena_is_linear_in_the_two_cotangents: four runs of each of the three calls, the sums
    dpix-alone + G-alone formed in float64; per arena segment the mean combined arena and the mean sum differ by at most three times
    the combined four-run spread, and the normal term's own share is far above that bound in every segment but SH (the rotation
    segment carries both the stage's columns and gsr_gaussian_normals_backward's addend)."""
    nr = sub("normal_render")
    f = frame(name)
    H, W = f["H"], f["W"]
    nimg = nr.render_normals(f["n"], f["buf"], H, W)
    dpix, G = _dpix(H, W), f["Gd"]
    arena = lambda res: parity.to_np(res["_arena"]).astype(np.float64)
    both = [arena(_backward(f, dpix, G, nimg)) for _ in range(4)]
    alone = [arena(_backward(f, dpix)) for _ in range(4)]
    sums = [a + arena(_backward(f, None, G, nimg)) for a in alone]
    offsets = [int(o) for o in sub("dist").arena_offsets(f["N"])]
    assert offsets[-1] == both[0].size == sums[0].size
    ref, ref_sum, ref_alone = np.mean(both, axis=0), np.mean(sums, axis=0), np.mean(alone, axis=0)
    pairs = [(i, j) for i in range(4) for j in range(i)]
    bad = []
    for k in range(len(offsets) - 1):
        seg = offsets[k:k + 2]
        s_both = max(_arena_norm(both[i], both[j], seg, ref) for i, j in pairs)
        s_sum = max(_arena_norm(sums[i], sums[j], seg, ref) for i, j in pairs)
        d = _arena_norm(ref, ref_sum, seg, ref)
        share = _arena_norm(ref, ref_alone, seg, ref)
        _row(test="linear", case=name, segment=k, difference=d, spread_both=s_both, spread_sum=s_sum, bound=3.0 * (s_both + s_sum), normal_share=share)
        if not (s_both > 0 and d <= 3.0 * (s_both + s_sum)):
            bad.append((k, d, s_both, s_sum))
        assert k == 4 or share > 100.0 * 3.0 * (s_both + s_sum), (k, share)
    assert not bad, f"{name}: (segment, difference, spread_both, spread_sum) {bad}"


def test_keyword_combinations_agree_with_the_dense_call():
    nr = sub("normal_render")
    f = frame("n2000_64x48")
    H, W, N = f["H"], f["W"], f["N"]
    nimg = nr.render_normals(f["n"], f["buf"], H, W)
    dpix, G = _dpix(H, W), f["Gd"]
    dense = _backward(f, dpix, G, nimg)
    cam = _backward(f, dpix, G, nimg, camera_grad=True)
    for k in GRAD_KEYS + ("dL_dmean2D", "dL_dconic", "dL_dinv_depths", "dL_dgaussian_normals"):
        parity.assert_grad(k, cam[k], dense[k])
    plain_cam = _backward(f, dpix, camera_grad=True)
    for k in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"):
        assert bool(torch.isfinite(cam[k]).all()) and bool(cam[k].any())
    assert float((cam["dL_dviewmatrix"] - plain_cam["dL_dviewmatrix"]).abs().max()) > 0       # the camera kernels read the added columns
    seen = []
    fact = _backward(f, dpix, G, nimg, sh_gradient="factored", on_payload=seen.append)
    assert fact["dL_dshs"] is None and len(seen) == 1 and seen[0] is fact["_view_payload"]
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dgaussian_normals"):
        parity.assert_grad(k, fact[k], dense[k])
    plain_fact = _backward(f, dpix, sh_gradient="factored")
    parity.assert_grad("payload", fact["_view_payload"], plain_fact["_view_payload"])             # the colour columns are untouched
    # normal_param_grad=False: everything but dL_drot is the dense call's, and dL_drot differs by gsr_gaussian_normals_backward's addend
    off = _backward(f, dpix, G, nimg, normal_param_grad=False)
    for k in ("dL_dmean3D", "dL_dscale", "dL_dopacity", "dL_dshs", "dL_dgaussian_normals"):
        parity.assert_grad(k, off[k], dense[k])
    sc, q, p = (_dev(f["sc"][k], f["dev"]) for k in ("scales", "rotations", "means"))
    addend = nr.gaussian_normals_backward(off["dL_dgaussian_normals"].contiguous(), sc, q, p, f["view"])
    assert float(addend.abs().max()) > 0
    parity.assert_grad("dL_drot", off["dL_drot"] + addend, dense["dL_drot"])
    # dL_dnormal_image alone, and together with the distortion term (the distortion stage first)
    only = _backward(f, None, G, nimg)
    plain = _backward(f, dpix)
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity"):
        parity.assert_grad(k, only[k] + plain[k], dense[k])
    dist_mod = sub("distortion")
    _, mom = dist_mod.render_distortion(f["buf"], H, W)
    gdist = torch.full((H, W), 100.0 / (W * H), device=f["dev"])
    three = _backward(f, dpix, G, nimg, dL_ddistortion=gdist, distortion_moments=mom)
    d_only = _backward(f, None, dL_ddistortion=gdist, distortion_moments=mom)
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity"):
        parity.assert_grad(k, three[k], dense[k] + d_only[k])


# ---- (e) ----
@pytest.mark.parametrize("name", ["n2000_64x48", "n1500_opaque_48x48", "toy"])
def test_consistency_loss_against_float64(name):
    nr, loss, normals, _lib, _host = sub("normal_render"), sub("loss"), sub("normals"), sub("_lib"), sub("_host")
    f = frame(name)
    H, W, dev = f["H"], f["W"], f["dev"]
    gsr = pkg()
    image, depth, buf = gsr.render_gaussians(**f["kw"], **f["extra"])
    cam = {"tan_fovx": f["kw"]["tan_fovx"], "tan_fovy": f["kw"]["tan_fovy"], "width": W, "height": H}
    nimg = nr.render_normals(f["n"], buf, H, W)
    depth, T = depth.reshape(H, W), buf["final_Ts"].reshape(H, W)
    n_d, valid = normals.normals_from_depth(depth, T, cam)
    m = _dev(np.random.default_rng(2).uniform(0.0, 2.0, (H, W)).astype(np.float32), dev)
    weight = 0.05
    # the entry point itself, for the n_d gradient the wrapper passes on
    L = _lib.lib()
    gN, gnd, sums = torch.full((H, W, 3), float("nan"), device=dev), torch.full((H, W, 3), float("nan"), device=dev), torch.empty(2, device=dev)
    ws = _host.workspace("normals", L.gsr_normals_workspace_bytes(W, H), dev)
    for mask in (None, m):
        _lib.check(L.gsr_normal_consistency_loss(nimg.data_ptr(), n_d.data_ptr(), valid.data_ptr(), _host.ptr(mask), W, H, weight, gN.data_ptr(),
                                                 gnd.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), _host.raw_stream(dev)))
        r = NR.consistency_f64(parity.to_np(nimg), parity.to_np(n_d), parity.to_np(valid), None if mask is None else parity.to_np(mask), weight, W, H)
        s32, gN32, gnd32, counted32 = NR.consistency_f32(parity.to_np(nimg), parity.to_np(n_d), parity.to_np(valid),
                                                         None if mask is None else parity.to_np(mask), weight, W, H)
        keep = ~r["near"]
        assert r["near"].mean() <= FR.MAX_MASKED and np.array_equal(counted32[keep], r["counted"][keep])
        gNk, gndk, sk = parity.to_np(gN), parity.to_np(gnd), parity.to_np(sums).astype(np.float64)
        assert np.isfinite(gNk).all() and np.isfinite(gndk).all()
        assert not gNk[keep & ~r["counted"]].any() and not gndk[keep & ~r["counted"]].any()
        unit_N, unit_d = np.abs(r["gN"]).max() + 1e-300, np.abs(r["gnd"]).max() + 1e-300
        E = {"gN": (float(np.abs(gNk - r["gN"])[keep].max() / unit_N), float(np.abs(gN32 - r["gN"])[keep].max() / unit_N)),
             "gnd": (float(np.abs(gndk - r["gnd"])[keep].max() / unit_d), float(np.abs(gnd32 - r["gnd"])[keep].max() / unit_d))}
        _row(test="consistency", case=name, masked=mask is not None, counted=int(r["counted"].sum()), sums=sk.tolist(), sums_f64=r["sums"].tolist(), E=E)
        for k, (e_k, e_32) in E.items():
            assert e_k <= 3.0 * e_32 + NR.EPS32, (k, e_k, e_32)
        if not (r["near"] & (parity.to_np(valid) != 0)).any():
            # the sums: float32 terms added in float64 and rounded once -- within the terms' own rounding of the float64 value
            scale = np.abs(r["terms"]).sum() + r["sums"][1]
            assert abs(sk[0] - r["sums"][0]) <= 3.0 * abs(float(s32[0]) - r["sums"][0]) + 2.0 * NR.EPS32 * scale, (sk, r["sums"], s32)
            assert abs(sk[1] - r["sums"][1]) <= NR.EPS32 * r["sums"][1]
    # the wrapper: the same bits every call, and its two images are the depth normals' VJP of gnd
    a = loss.normal_consistency_loss_and_gradients(nimg, depth, T, cam, m, weight)
    b = loss.normal_consistency_loss_and_gradients(nimg, depth, T, cam, m, weight)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[0], sums) and torch.equal(a[1], gN)
    gD, gA = normals.normals_from_depth_backward(gnd, depth, T, cam)
    assert torch.equal(a[2], gD) and torch.equal(a[3], gA)
    slot = torch.zeros(2, device=dev)
    c = loss.normal_consistency_loss_and_gradients(nimg, depth, T, cam, m, weight, loss_out=slot)
    assert c[0] is slot and torch.equal(slot, sums)


# ---- the trainer ----
# Hidden scene, --size 100 --views 8 --iterations 300 --report-normal-consistency, with and without --lambda-normal-consistency.  The
# weight is 2DGS's 0.05, chosen once and not tuned.  Three starts, once each on the MI355X; the measured figures are in
# profiles/normal_render/train_three_starts.json and the README.  NC_REDUCTION_MIN is half the smallest of the three measured
# reductions of train_normal_consistency_deg against the run WITHOUT the term (the parent's behaviour); None: the three reductions
# did not share a sign, and the test only holds the runs finite with their summary fields.
# Measured, angle without -> with the term (reduction; PSNR without -> with): --init reference 57.97 -> 17.84 degrees (0.692; 24.44 ->
# 24.07 dB), --init random 41.71 -> 16.12 (0.614; 27.11 -> 26.37 dB), --init knn 57.60 -> 18.00 (0.688; 24.36 -> 23.95 dB).  All three
# starts show the reduction: the test requires half the smallest.
NC_WEIGHT = "0.05"
NC_REDUCTION_MIN = 0.30


def _train(tmp_path, tag, *extra):
    log = tmp_path / f"{tag}.jsonl"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--log", str(log), "--print-interval", "1000", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    for line in open(log):
        rec = json.loads(line)
        if rec["record"] == "summary":
            return rec


def test_trainer_with_the_consistency_term(tmp_path):
    base = ["--size", "100", "--views", "8", "--iterations", "300", "--report-normal-consistency"]
    s0 = _train(tmp_path, "plain", *base)
    s1 = _train(tmp_path, "nc", *base, "--lambda-normal-consistency", NC_WEIGHT)
    for s in (s0, s1):
        assert all(s["parameters_finite"].values()) and np.isfinite(s["train_normal_consistency_deg"]) and np.isfinite(s["train_psnr_mean"])
    reduction = 1.0 - s1["train_normal_consistency_deg"] / s0["train_normal_consistency_deg"]
    _row(test="trainer", weight=NC_WEIGHT, angle_plain=s0["train_normal_consistency_deg"], angle_with=s1["train_normal_consistency_deg"],
         reduction=reduction, psnr_plain=s0["train_psnr_mean"], psnr_with=s1["train_psnr_mean"])
    if NC_REDUCTION_MIN is not None:
        assert reduction >= NC_REDUCTION_MIN, reduction
    plain = _train(tmp_path, "absent", "--size", "100", "--views", "8", "--iterations", "2")
    assert "train_normal_consistency_deg" not in plain
