"""
The ray-plane intersection depth (csrc/plane_depth.hip, include/gsr_plane_depth.h) on the MI355X, against the float64 yardstick and
the float32 restatement of tests/plane_depth_reference.py.

  (a), (d)  N = 1, 63, 64, 65 and 257 with every branch mixed in (zero normal, behind the camera, inside the near plane, grazing,
            round): the kernel follows the float32 branch of every row, the slopes are exactly 0 on the fallback rows and within
            3 E_f32 + eps32 of float64 elsewhere; the backward against torch autograd of the definition under
            distortion_reference.criterion, ADDED over a seeded buffer, the same bits twice.
  (b)       host-built frames of frame_walk_frames.build_frame at 8x8, 16x8, 16x16 and 33x20, list lengths 0, 1, 255, 256, 257 and 640
            (each single-tile shape with each length; 33x20 has six tiles, one per length), out-of-range ids, masks None, "ff" and
            "random": bit-identical to render_features(invd[:, None]) at zero slopes; the same bits across two calls, two streams and
            the three masks; every pixel written over a poisoned output, exact zeros where n_contrib is 0; and BIT-IDENTICAL TO THE
            FLOAT32 RESTATEMENT on the same frames with their conics set to zero.  With a zero conic exp(power) is exp(0) = 1 on both
            sides, alpha is the opacity, and everything the header states -- the n_contrib cut, the 1/255 test, T, the two fused
            multiply-adds and the clamp of m, the accumulation -- is replayed bit for bit; with a non-zero conic the hardware's exp and
            libm's differ in their last bit, which is the one thing no restatement replays, so those frames are held to the restatement
            within 3 E_f32 + eps32 of float64 in (c) instead.  ("random" masks: random bytes OR the bits the forward's promise needs,
            median_depth_reference's rule.)
  (c)       the rendered frames of test_gpu_features._case (the four small scenes, toy at 120x90, one Gaussian over 40x40, n2000
            antialiased, under the 3D filter and in capacity mode), slopes from plane_depth_reference.plane_scales: the image within
            3 E_f32 + eps32; criterion(E_kernel, E_f32, E_spread, floor) per output, E_f32 the CPU record
            (tests/golden/plane_depth_margins.json) or, for a frame the CPU matrix does not have, the restatement's error on the
            frame's own buffers -- never the kernel's; the untouched accumulator columns, column 11 included, bit-equal to the plain
            call's; the arena linear in the cotangent per segment; the closed-form plane frame through the real forward.
  composition: camera_grad, sh_gradient="factored", plane_param_grad=False, dL_dplane_depth alone and a re-packed frame against the dense
            call; all four stages together equal the sum of the single-stage calls.
  the trainer with --lambda-depth 1 --depth-render plane ends finite with its summary fields; fuse_views(plane_depth=True) on the
  64^3 / 8-view flat torus gives a non-empty, finite mesh.  No quality threshold: "mesh_gap_min" stays null.

Every measured figure is printed as a PLANE_DEPTH_ROW JSON line; tools/record_plane_depth_margins.py files the E_kernel of a run in the
golden JSON, as a record only.
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
import frame_walk_reference as FWR
import features_reference as FR
import frame_walk_frames as FW
import median_depth_reference as M
import normal_render_reference as NR
import plane_depth_reference as PD
import parity
from test_gpu_features import _case

pytestmark = pytest.mark.gpu
FRAMES = list(FR.SCENES) + ["toy", "one_gaussian_40x40", "n2000_antialiased", "n2000_filter3d", "n2000_capacity"]
EPS32 = PD.EPS32
f32 = np.float32
_FRAMES = {}


def _row(**kw):
    print("\nPLANE_DEPTH_ROW " + json.dumps(kw))


def _dev(a, dev=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev or torch.device("cuda", torch.cuda.current_device()))


def _bwd_extra(extra):
    return {k: v for k, v in extra.items() if k in ("rasterize_mode", "filter_3d")}


# ---- (a), (d) ----
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_slopes_and_backward_against_float64(N):
    pd = sub("plane_depth")
    cam = lego_camera(sub("cameras"), 0, width=50, height=37)
    view = np.asarray(cam["world_to_camera"], f32)
    tx, ty, W, H = cam["tan_fovx"], cam["tan_fovy"], 50, 37
    n, s, p, special = PD.draw_gaussians(N, view)
    assert PD.branch_margins(n, s, p, view).min() > PD.MARGIN_CAP
    sl32, fb = PD.slopes_f32(n, s, p, view, tx, ty, W, H)
    sl64 = PD.slopes_f64(n, s, p, view, tx, ty, W, H, fb)
    nd, sd, pdev = _dev(n), _dev(s), _dev(p)
    out = torch.full((N, 2), float("nan"), device=nd.device)
    got = pd.plane_slopes(nd, sd, pdev, cam, out=out)
    assert got is out and torch.equal(got, pd.plane_slopes(nd, sd, pdev, cam))
    k = parity.to_np(got)
    assert not k[fb].view(np.uint32).any() and (N < 9 or fb.sum() >= 5)              # exactly 0 on the fallback rows, every branch met
    assert (k[~fb] != 0).any(1).all() or N == 1
    unit = np.abs(sl64).max()
    E_k, E_32 = float(np.abs(k - sl64).max() / unit), float(np.abs(sl32 - sl64).max() / unit)
    _row(test="slopes", N=N, E_kernel=E_k, E_f32=E_32, fallback=int(fb.sum()), bit_equal_to_restatement=bool(np.array_equal(k, sl32)))
    assert E_k <= 3.0 * E_32 + EPS32, (E_k, E_32)
    mom = np.random.default_rng(9).normal(0, 1, (N, 3)).astype(f32) * np.array([1.0, 5.0, 5.0], f32)
    dmean64, dn64, sc_mean, sc_n = PD.slopes_vjp_f64(n, s, p, view, tx, ty, W, H, fb, mom)
    rm, rn = PD.slopes_backward(n, s, p, view, tx, ty, W, H, mom)
    md = _dev(mom)
    a, b = pd.plane_slopes_backward(md, nd, sd, pdev, cam), pd.plane_slopes_backward(md, nd, sd, pdev, cam)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                       # no atomics: the same bits
    E_k = (PD.rows_error(parity.to_np(a[0]), dmean64, sc_mean), PD.rows_error(parity.to_np(a[1]), dn64, sc_n))
    E_32 = (PD.rows_error(rm, dmean64, sc_mean), PD.rows_error(rn, dn64, sc_n))
    _row(test="slopes_backward", N=N, E_kernel=E_k, E_f32=E_32)
    for ek, e32 in zip(E_k, E_32):
        assert FWR.criterion(ek, e32, 0.0, 0.5 * EPS32), (ek, e32)                    # (floor: one rounding of the result in its scale)
    assert not parity.to_np(a[1])[fb].any()
    pre = torch.rand((N, 3), device=nd.device)
    poisoned = torch.full((N, 3), float("nan"), device=nd.device)
    added, dn = pd.plane_slopes_backward(md, nd, sd, pdev, cam, dL_dmean3D=pre.clone(), out=poisoned)
    assert torch.equal(added, pre + a[0]) and dn is poisoned and torch.equal(dn, a[1])          # it ADDS to the means and WRITES the normals' rows


# ---- (b) ----
SHAPES = {"8x8": (8, 8), "16x8": (16, 8), "16x16": (16, 16), "33x20": (33, 20)}
B_CASES = [(tag, (ln,)) for tag in ("8x8", "16x8", "16x16") for ln in FW.LENS] + [("33x20", FW.LENS)]


def _plane_forward(d, slopes, stream=None):
    out = torch.full((d.H, d.W), float("nan"), dtype=torch.float32, device=d.dev)
    FW._lib.check(d.L.gsr_plane_depth_forward(C.byref(d.dframe), FW._host.ptr(slopes), FW._host.ptr(out), d.stream if stream is None else stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _with_masks(fr, masks, need):
    out = dict(fr)
    out["masks"] = (None if masks is None else np.full(fr["D"], 0xFF, np.uint8) if masks == "ff"
                    else np.random.default_rng(77).integers(0, 256, fr["D"]).astype(np.uint8) | need)
    return out


def _draw_slopes(fr, seed):
    """(N, 2) float32: most planes gentle, every seventh steep enough to meet the clamp inside a tile, every fifth exactly zero."""
    rng = np.random.default_rng(seed)
    s = (rng.uniform(-0.02, 0.02, (fr["N"], 2)) * fr["invd"][:, None]).astype(f32)
    s[::7] *= f32(12)
    s[::5] = 0
    return s


@pytest.mark.parametrize("tag,lens", B_CASES, ids=[f"{t}-{'-'.join(map(str, l))}" for t, l in B_CASES])
def test_forward_on_host_built_frames(tag, lens):
    W, H = SHAPES[tag]
    fr = FW.build_frame(21 + len(lens) + lens[0], W, H, lens=lens, N=700)
    need = M.median_f64(fr)["need"]
    slopes = _draw_slopes(fr, 5)
    base = None
    for masks in (None, "ff", "random"):
        d = FW.DeviceFrame(_with_masks(fr, masks, need))
        sd = _dev(slopes, d.dev)
        got = _plane_forward(d, sd)
        assert np.isfinite(got).all(), "every pixel is written"
        base = got if base is None else base
        assert got.tobytes() == base.tobytes(), masks
        assert _plane_forward(d, sd).tobytes() == base.tobytes(), (masks, "a second call")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert _plane_forward(d, sd, FW._host.raw_stream(d.dev)).tobytes() == base.tobytes()
    assert not base[fr["n_contrib"] == 0].view(np.uint32).any()                      # a pixel with n_contrib = 0 is exactly 0
    assert fr["D"] == 0 or fr["bad"].sum() >= 1 or fr["D"] < 30
    assert _plane_forward(FW.DeviceFrame(FW.other_bad_ids(fr, 5)) if fr["bad"].sum() >= 2 else d, sd).tobytes() == base.tobytes()
    # zero slopes: bit for bit gsr_features_forward of the inverse depths at C = 1
    zero = torch.zeros((fr["N"], 2), device=d.dev)
    F = _dev(fr["invd"][:, None], d.dev)
    feat = torch.full((H, W, 1), float("nan"), device=d.dev)
    FW._lib.check(d.L.gsr_features_forward(C.byref(d.frame), 1, FW._host.ptr(F), FW._host.ptr(feat), d.stream))
    torch.cuda.synchronize()
    assert _plane_forward(d, zero).tobytes() == feat.cpu().numpy().tobytes()
    # zero conics: exp(power) = 1 on both sides, and the restatement replays every bit (half of the frames with faint opacities, so
    # that long lists stay open and many entries fall below 1 / 255)
    flat = dict(fr, co=fr["co"].copy())
    flat["co"][:, :3] = 0
    if lens[0] in (255, 640) or tag == "16x16":
        flat["co"][:, 3] *= f32(0.02)
    for masks in (None, "ff"):
        d0 = FW.DeviceFrame(_with_masks(flat, masks, need))
        got0 = _plane_forward(d0, _dev(slopes, d0.dev))
        want, _ = PD.render_f32(flat, slopes)
        assert got0.tobytes() == want.tobytes(), (masks, int((got0 != want).sum()), float(np.abs(got0 - want).max()))
    steep = int((want != PD.render_f32(flat, slopes * f32(1e-3))[0]).sum())
    _row(test="forward_host_frames", case=f"{tag} {lens}", D=fr["D"], nonzero_pixels=int((base != 0).sum()), zero_conic_nonzero=int((want != 0).sum()),
         differs_from_gentle_slopes=steep)
    assert fr["D"] == 0 or (base != 0).any() or max(lens) <= 1


# ---- (c) ----
def frame(name):
    """The kernel forward of a frame (background 0), the kernel's normals and slopes, g, and the yardstick and restatement on its
    buffers, once per session."""
    if name not in _FRAMES:
        gsr = pkg()
        nr, pd, dist = sub("normal_render"), sub("plane_depth"), sub("distortion")
        sc, cam, kw, extra = _case(name)
        H, W = kw["image_height"], kw["image_width"]
        image, inv_depth, buf = gsr.render_gaussians(**kw, **extra)
        dev = image.device
        nb = {k: parity.to_np(buf[k]) for k in ("points_xy_image", "conic_opacity", "point_list", "ranges", "n_contrib")}
        if "capacity" in extra:
            D, over = sub("forward").rendered_count(buf)
            assert not over and 0 < D < extra["capacity"]
            nb["point_list"] = nb["point_list"][:D]
        N = sc["means"].shape[0]
        view = np.asarray(kw["viewmatrix"], f32)
        camd = {"world_to_camera": view, "tan_fovx": kw["tan_fovx"], "tan_fovy": kw["tan_fovy"], "width": W, "height": H}
        n = nr.gaussian_normals(_dev(sc["scales"], dev), _dev(sc["rotations"], dev), _dev(sc["means"], dev), view)
        ps = PD.plane_scales(sc["scales"])
        slopes = pd.plane_slopes(n, _dev(ps, dev), _dev(sc["means"], dev), camd)
        sl32, fb = PD.slopes_f32(parity.to_np(n), ps, sc["means"], view, kw["tan_fovx"], kw["tan_fovy"], W, H)
        k = parity.to_np(slopes)
        assert np.array_equal(k != 0, sl32 != 0) or np.abs(k - sl32).max() <= 8 * EPS32 * np.abs(sl32).max()
        invd = parity.to_np(sub("_frame").inv_depth_of(buf, N, dev)).astype(f32)
        r = PD.yardstick(nb, W, H, invd, k, PD.draw_g(H, W))
        print(f"\n{name}: D {nb['point_list'].shape[0]}, {int(r['mask'].sum())} of {r['mask'].size} pixels masked, plane branch {float((k != 0).any(1).mean()):.2f}, "
              f"clamped pairs {r['clamped']}")
        assert r["mask"].sum() <= FR.MAX_MASKED * r["mask"].size and r["clamp_margin"] > PD.MARGIN_CAP
        g32 = r["g"].astype(f32)                                   # zero at the masked pixels: both sides lose them
        fr = PD.frame_of_buffers(nb, W, H, invd)
        img32, _ = PD.render_f32(fr, k)
        acc32, mom32 = PD.render_backward_f32(fr, k, g32, img32)
        _FRAMES[name] = dict(sc=sc, cam=cam, camd=camd, kw=kw, extra=extra, H=H, W=W, N=N, buf=buf, nb=nb, r=r, g=g32, img32=img32, acc32=acc32, mom32=mom32,
                             n=n, slopes=slopes, slopes32=k, invd=invd, view=view, gd=_dev(g32, dev), dev=dev, depth=inv_depth, plane_scales=ps)
    return _FRAMES[name]


def _accumulators(g, N):
    """The (N, 16) accumulator rows of a backward() result, through the tag densify.DensifyStats.update uses."""
    ws = g["dL_dmean2D"]._gsr_backward_ws[0]
    off = int(sub("_lib").lib().gsr_backward_accumulators_offset(N))
    return ws[off:off + 64 * N].view(torch.float32).view(N, 16)


def _backward(f, dpix=None, g=None, pimg=None, slopes=None, **more):
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], dpix)
    if g is not None:
        kw.update(dL_dplane_depth=g, plane_slopes=f["slopes"] if slopes is None else slopes, plane_depth_image=pimg, gaussian_normals=f["n"])
    return pkg().backward(**kw, **_bwd_extra(f["extra"]), **more)


def _e_f32(name, f):
    """The restatement's errors the criterion uses: the CPU record of the frame, or for a frame the CPU matrix does not have the
    restatement's errors on the frame's own buffers."""
    rec = PD.golden()["E_f32"].get(name)
    if rec is not None:
        return {k: rec[k] for k in PD.OUTPUTS}, "recorded"
    return PD.backward_errors(f["acc32"], f["mom32"], f["r"]), "on the frame's buffers"


def _runs(f, pimg, n_runs=2):
    runs = []
    for _ in range(n_runs):
        res = _backward(f, None, f["gd"], pimg, plane_param_grad=False)
        acc = _accumulators(res, f["N"]).clone()
        assert tuple(res["dL_dplane_moments"].shape) == (f["N"], 3) and "dL_dinv_depths" in res
        assert not bool(acc[:, list(PD.UNTOUCHED)].any())             # g alone: the other columns, 11 included, are what a zero image leaves
        assert bool(torch.isfinite(res["_arena"]).all())
        runs.append((parity.to_np(acc), parity.to_np(res["dL_dplane_moments"])))
    return runs


@pytest.mark.parametrize("name", FRAMES)
def test_image_and_backward_against_float64(name):
    pd, feat = sub("plane_depth"), sub("features")
    f = frame(name)
    H, W, N, r, buf, dev = f["H"], f["W"], f["N"], f["r"], f["buf"], f["dev"]
    a = pd.render_plane_depth(f["slopes"], buf, H, W)
    assert tuple(a.shape) == (H, W) and bool(torch.isfinite(a).all())
    out = torch.full((H, W), float("nan"), device=dev)
    assert pd.render_plane_depth(f["slopes"], buf, H, W, out=out, use_block_masks=False) is out and torch.equal(out, a)
    zero = pd.render_plane_depth(torch.zeros((N, 2), device=dev), buf, H, W)
    assert torch.equal(zero[..., None], feat.render_features(_dev(f["invd"][:, None], dev), buf, H, W))      # bit for bit at C = 1
    E_k, E_32 = PD.image_error(a, r, f["invd"]), PD.image_error(f["img32"], r, f["invd"])
    _row(test="forward", case=name, E_kernel=E_k, E_f32=E_32, differs_from_centre_depth=int((a != zero).sum().item()))
    assert E_k <= 3.0 * E_32 + EPS32, (E_k, E_32)
    E32, source = _e_f32(name, f)
    runs = _runs(f, a)
    Ek = {k: max(PD.backward_errors(ac, mo, r)[k] for ac, mo in runs) for k in PD.OUTPUTS}
    E_s = PD.spread(runs[0], runs[1], r)
    floor = PD.golden()["floor"]
    _row(test="backward", case=name, E_kernel=Ek, E_f32=E32, E_f32_source=source, E_spread=E_s, floor=floor,
         E_f32_here=PD.backward_errors(f["acc32"], f["mom32"], r))
    for k in PD.OUTPUTS:
        assert FWR.criterion(Ek[k], E32[k], E_s, floor), (k, Ek[k], E32[k], E_s)
    assert all(np.abs(runs[0][0][:, c]).max() > 0 for c in PD.TOUCHED) and np.abs(runs[0][1]).max() > 0
    # the untouched columns are bit for bit the plain call's (no colour cotangent: a zero alpha image alone), column 11 included
    plain = _backward(f, None, dL_dalpha_image=torch.zeros((H, W), device=dev))
    cols = list(PD.UNTOUCHED)
    assert 11 in cols and np.array_equal(parity.to_np(_accumulators(plain, N))[:, cols], runs[0][0][:, cols])


def _own_slopes(f):
    """The slopes of the scene's OWN scales: backward() recomputes every Gaussian's branch from the scales it is given, so the calls
    that run its two per-Gaussian kernels take the slopes those scales give (a quarter of the drawn Gaussians are flat)."""
    if "own" not in f:
        dev = f["dev"]
        f["own"] = sub("plane_depth").plane_slopes(f["n"], _dev(f["sc"]["scales"], dev), _dev(f["sc"]["means"], dev), f["camd"])
        share = float((f["own"] != 0).any(1).float().mean())
        assert 0.1 < share < 0.9, share
    return f["own"]


def _dpix(H, W, seed=3):
    return (np.random.default_rng(seed).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(f32)


def _arena_norm(x, y, offsets, ref):
    worst = 0.0
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        m = np.abs(ref[lo:hi]).max()
        if m > 0:
            worst = max(worst, float(np.abs(x[lo:hi] - y[lo:hi]).max() / m))
    return worst


def test_arena_is_linear_in_the_two_cotangents():
    """As test_gpu_normal_render.test_arena_is_linear_in_the_two_cotangents: four runs of each of the three calls, the sums
    dpix-alone + g-alone formed in float64; per arena segment the mean combined arena and the mean sum differ by at most three times the
    combined four-run spread, and the plane term's own share is far above that bound in every segment but SH (which it does not
    reach)."""
    pd = sub("plane_depth")
    f = frame("n2000_64x48")
    H, W = f["H"], f["W"]
    own = _own_slopes(f)
    pimg = pd.render_plane_depth(own, f["buf"], H, W)
    dpix, g = _dpix(H, W), f["gd"]
    arena = lambda res: parity.to_np(res["_arena"]).astype(np.float64)
    both = [arena(_backward(f, dpix, g, pimg, own)) for _ in range(4)]
    alone = [arena(_backward(f, dpix)) for _ in range(4)]
    sums = [a + arena(_backward(f, None, g, pimg, own)) for a in alone]
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
        _row(test="linear", segment=k, difference=d, spread_both=s_both, spread_sum=s_sum, bound=3.0 * (s_both + s_sum), plane_share=share)
        if not (s_both > 0 and d <= 3.0 * (s_both + s_sum)):
            bad.append((k, d, s_both, s_sum))
        assert k == 4 or share > 100.0 * 3.0 * (s_both + s_sum), (k, share)
    assert not bad, f"(segment, difference, spread_both, spread_sum) {bad}"


def test_closed_form_plane_through_the_real_forward():
    gsr = pkg()
    nr, pd = sub("normal_render"), sub("plane_depth")
    sc, cam, kw, th = PD.sheet(sub("scenes"), sub("cameras"))
    W, H = kw["image_width"], kw["image_height"]
    image, depth, buf = gsr.render_gaussians(**kw)
    dev = image.device
    view = np.asarray(kw["viewmatrix"], f32)
    tx, ty = kw["tan_fovx"], kw["tan_fovy"]
    camd = {"world_to_camera": view, "tan_fovx": tx, "tan_fovy": ty, "width": W, "height": H}
    n = nr.gaussian_normals(_dev(sc["scales"], dev), _dev(sc["rotations"], dev), _dev(sc["means"], dev), view)
    slopes = pd.plane_slopes(n, _dev(sc["scales"], dev), _dev(sc["means"], dev), camd)
    assert bool((slopes != 0).any(1).all())
    out = parity.to_np(pd.render_plane_depth(slopes, buf, H, W)).astype(np.float64)
    centre = parity.to_np(depth).reshape(H, W).astype(np.float64)
    cover = 1.0 - parity.to_np(buf["final_Ts"]).reshape(H, W).astype(np.float64)
    V = view.astype(np.float64).reshape(4, 4)
    pv = sc["means"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    n0 = NR.normals_f64(sc["scales"], sc["rotations"], sc["means"], view)["n"][0]
    k0 = int(np.argmin(np.abs(sc["means"]).sum(1)))
    want = PD.plane_inverse_depth(n0, pv[k0], tx, ty, W, H)
    sel = cover >= 0.5
    assert sel.sum() > 0.2 * W * H
    rel = np.abs(out[sel] / cover[sel] / want[sel] - 1.0)
    off = np.abs(centre[sel] / cover[sel] / want[sel] - 1.0)
    sigma_px = 0.2 / pv[:, 2].mean() / (2.0 * tx / W)
    slope = float(np.abs(parity.to_np(slopes).astype(np.float64)).max())
    margin = 0.25 * slope * sigma_px / float(parity.to_np(sub("_frame").inv_depth_of(buf, len(pv), dev)).max())
    _row(test="closed_form", covered=int(sel.sum()), plane_eps32=float(rel.max() / EPS32), centre_off=float(off.max()), margin=margin)
    assert rel.max() <= 16 * EPS32
    assert off.max() >= margin > 1000 * EPS32


# ---- composition ----
GRAD_KEYS = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dshs")


def test_keyword_combinations_agree_with_the_dense_call():
    pd, nr = sub("plane_depth"), sub("normal_render")
    f = frame("n2000_64x48")
    H, W, N, dev = f["H"], f["W"], f["N"], f["dev"]
    own = _own_slopes(f)
    ps = _dev(f["sc"]["scales"], dev)
    pimg = pd.render_plane_depth(own, f["buf"], H, W)
    dpix, g = _dpix(H, W), f["gd"]
    dense = _backward(f, dpix, g, pimg, own)
    plain = _backward(f, dpix)
    assert "dL_dplane_moments" in dense and "dL_dplane_moments" not in plain
    cam = _backward(f, dpix, g, pimg, own, camera_grad=True)
    for k in GRAD_KEYS + ("dL_dmean2D", "dL_dconic", "dL_dinv_depths", "dL_dplane_moments"):
        parity.assert_grad(k, cam[k], dense[k])
    plain_cam = _backward(f, dpix, camera_grad=True)
    for k in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"):
        assert bool(torch.isfinite(cam[k]).all()) and bool(cam[k].any())
    assert float((cam["dL_dviewmatrix"] - plain_cam["dL_dviewmatrix"]).abs().max()) > 0       # the camera kernels read the added columns
    seen = []
    fact = _backward(f, dpix, g, pimg, own, sh_gradient="factored", on_payload=seen.append)
    assert fact["dL_dshs"] is None and len(seen) == 1 and seen[0] is fact["_view_payload"]
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dplane_moments"):
        parity.assert_grad(k, fact[k], dense[k])
    parity.assert_grad("payload", fact["_view_payload"], _backward(f, dpix, sh_gradient="factored")["_view_payload"])
    # plane_param_grad=False: everything but the two kernels' addends is the dense call's
    off = _backward(f, dpix, g, pimg, own, plane_param_grad=False)
    for k in ("dL_dscale", "dL_dopacity", "dL_dshs", "dL_dplane_moments"):
        parity.assert_grad(k, off[k], dense[k])
    p, q = _dev(f["sc"]["means"], dev), _dev(f["sc"]["rotations"], dev)
    dmean, dn = pd.plane_slopes_backward(off["dL_dplane_moments"].contiguous(), f["n"], ps, p, f["camd"])
    drot = nr.gaussian_normals_backward(dn, ps, q, p, f["view"])
    assert float(dmean.abs().max()) > 0 and float(drot.abs().max()) > 0
    parity.assert_grad("dL_dmean3D", off["dL_dmean3D"] + dmean, dense["dL_dmean3D"])
    parity.assert_grad("dL_drot", off["dL_drot"] + drot, dense["dL_drot"])
    # dL_dplane_depth alone
    only = _backward(f, None, g, pimg, own)
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity"):
        parity.assert_grad(k, only[k] + plain[k], dense[k])
    assert not bool(only["dL_dcolor"].any()) and not bool(only["dL_dinv_depths"].any())         # column 11 stays the centre-depth terms' alone
    # without the forward's records the frame is re-packed from the forward's depths
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], dpix)
    kw.update({"means2D": f["buf"]["points_xy_image"].clone(), "conic_opacity": f["buf"]["conic_opacity"].clone(), "rgb": f["buf"]["colors"].clone()},
              dL_dplane_depth=g, plane_slopes=own, plane_depth_image=pimg, gaussian_normals=f["n"])
    with pytest.raises(ValueError, match="depths"):
        pkg().backward(**kw)
    kw["geom_buffer"] = dict(kw["geom_buffer"], depths=f["buf"]["depths"])
    repacked = pkg().backward(**kw)
    assert not pkg().backward.last_call_used_forward_records
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dplane_moments"):
        parity.assert_grad(k, repacked[k], dense[k])


def test_all_four_stages_together_equal_the_sum_of_the_single_stage_calls():
    """Distortion, normals, plane depth and median in one call against the float64 sum of the four single-stage calls, per arena
    segment (in units of the segment's largest sum of the four terms' magnitudes), three runs of each side.  The bound is the
    criterion's shape: three times the two sides' run-to-run spreads plus a floor of 8 eps32 -- in one call the four terms meet in the
    same float32 accumulator columns (at most four additions, half an eps32 of the scale each) before the linear per-Gaussian half and
    its addends (four more), in the other each result is rounded on its own (four times half an eps32) before the float64 sum."""
    pd, nr, dist_mod, med_mod = sub("plane_depth"), sub("normal_render"), sub("distortion"), sub("median_depth")
    f = frame("n2000_64x48")
    H, W, dev, buf = f["H"], f["W"], f["dev"], f["buf"]
    own = _own_slopes(f)
    pimg = pd.render_plane_depth(own, buf, H, W)
    nimg = nr.render_normals(f["n"], buf, H, W)
    _, mom = dist_mod.render_distortion(buf, H, W)
    med, contrib = med_mod.render_median_depth(buf, H, W)
    rng = np.random.default_rng(4)
    stages = {
        "distortion": dict(dL_ddistortion=torch.full((H, W), 100.0 / (W * H), device=dev), distortion_moments=mom),
        "normals": dict(dL_dnormal_image=_dev(NR.draw_G(H, W), dev), gaussian_normals=f["n"], normal_image=nimg),
        "plane": dict(dL_dplane_depth=f["gd"], plane_slopes=own, plane_depth_image=pimg, gaussian_normals=f["n"]),
        "median": dict(dL_dmedian_depth=_dev((rng.normal(0, 1, (H, W)) / (W * H)).astype(f32), dev), median_contributor=contrib),
    }
    arena = lambda res: parity.to_np(res["_arena"]).astype(np.float64)
    together_kw = {}
    for kw in stages.values():
        together_kw.update(kw)
    together = [arena(_backward(f, None, **together_kw)) for _ in range(3)]
    parts = [[arena(_backward(f, None, **kw)) for kw in stages.values()] for _ in range(3)]
    sums = [np.sum(p, axis=0) for p in parts]
    scale = np.sum([np.abs(x) for x in parts[0]], axis=0)
    offsets = [int(o) for o in sub("dist").arena_offsets(f["N"])]
    pairs = [(i, j) for i in range(3) for j in range(i)]
    for k in range(len(offsets) - 2):                              # (the SH segment: no colour cotangent, all zero)
        seg = offsets[k:k + 2]
        s_t = max(_arena_norm(together[i], together[j], seg, scale) for i, j in pairs)
        s_s = max(_arena_norm(sums[i], sums[j], seg, scale) for i, j in pairs)
        d = _arena_norm(np.mean(together, axis=0), np.mean(sums, axis=0), seg, scale)
        shares = [_arena_norm(x, np.zeros_like(x), seg, scale) for x in parts[0]]
        _row(test="four_stages", segment=k, difference=d, spread_together=s_t, spread_sum=s_s, bound=3.0 * (s_t + s_s) + 8 * EPS32, shares=shares)
        assert d <= 3.0 * (s_t + s_s) + 8 * EPS32, (k, d, s_t, s_s)
        assert shares[2] > 0 and (k > 0 or min(shares) > 0)        # the plane stage reaches all four segments, every stage the means (the median only them)
    assert not np.abs(together[0][offsets[4]:]).any()


# ---- the workflow ----
def test_flat_torus_gives_a_mesh_with_plane_depth():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from eval_mesh import demo_torus, flat_discs
    gsr = pkg()
    # the discs' normals are the torus's: the demo's quaternions are built by hand, so hold them to the analytic normal first
    pts = np.array([[0.85, 0, 0], [0.6, 0, 0.25], [0, 0.35, 0], [0.6 / np.sqrt(2), 0.6 / np.sqrt(2), -0.25]], f32)
    P = flat_discs(gsr.point_cloud.gaussians_from_points(np.concatenate([pts, pts * f32(1.0001)]), opacity=0.9, device="cuda"), 0.6, 0.1)
    view = np.eye(4, dtype=f32)
    view[3, 2] = 3.0                                               # the camera three units down the z axis, world axes
    nrm = parity.to_np(gsr.normal_render.gaussian_normals(P["scales"], P["rotations"], P["positions"], view))[:4]
    want = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1]], np.float64)
    assert np.abs(np.abs((nrm * want).sum(1)) - 1.0).max() <= 1e-5, nrm
    rows = {}
    for mode in ("expected", "plane"):
        m = demo_torus(gsr, 64, 8, 20_000, 128, seed=0, log=lambda s: None, depth_mode=mode, flat=0.1)
        assert m["triangles"] > 0 and m["vertices"] > 0 and m["depth_mode"] == mode and m["flat"] == 0.1
        for k in ("accuracy", "completeness", "chamfer", "accuracy_voxels", "completeness_voxels"):
            assert np.isfinite(m[k]) and m[k] >= 0, (mode, k, m[k])
        rows[mode] = {k: m[k] for k in ("accuracy_voxels", "completeness_voxels", "triangles")}
    _row(test="torus", **rows)
    assert PD.golden()["mesh_gap_min"] is None                      # no threshold on the gap until the README's table exists
    with pytest.raises(ValueError, match="plane_depth=True"):
        gsr.tsdf.fuse_views(lambda c: None, [{}], depth_mode="median", plane_depth=True, params=P)


def test_trainer_runs_with_the_plane_depth_term(tmp_path):
    log = tmp_path / "plane.jsonl"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--log", str(log), "--print-interval", "1000", "--size", "100",
                        "--views", "8", "--iterations", "300", "--lambda-depth", "1", "--depth-render", "plane"],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    s = [json.loads(line) for line in open(log)]
    s = [r for r in s if r["record"] == "summary"][0]
    assert all(s["parameters_finite"].values()) and s["depth_render"] == "plane"
    for k in ("train_psnr_mean", "train_depth_l1_mean", "train_plane_depth_l1_mean"):
        assert np.isfinite(s[k]), k
    _row(test="trainer", psnr=s["train_psnr_mean"], depth_l1=s["train_depth_l1_mean"], plane_depth_l1=s["train_plane_depth_l1_mean"])
