"""
The depth-distortion regulariser (csrc/distortion.hip, include/gsr_distortion.h) on the MI355X, against the float64 yardstick and the
float32 restatement of tests/distortion_reference.py, both taken on the KERNEL forward's own buffers (m = the records' 1 / depth).

Frames: the four small scenes of the CPU matrix (50x37 and 64x48 with partial tiles, lists past 256 and 512 entries, early
saturation), the toy scene at 120x90, one Gaussian over 40x40, a frame with D = 0, and the second scene antialiased, under the 3D
filter and in capacity mode.

  (toy and one_gaussian_40x40 have Dist = 0 -- equal depths, one contributor: there dist, every accumulator column and the float64
  side are held to exactly 0, and no relative figure is printed or filed.)

  1. forward against float64 on the unmasked pixels, relative, in units of 1 + mu / sigma (printed in eps32 of it):
     E_kernel <= 3 E_f32 + floor["forward"]; a pixel whose float64 Dist is exactly 0 must be exactly 0;
     moments[..., 0] is bit for bit render_features(ones);
  2. forward determinism: a second call, another stream, without the block masks, into an out= full of NaN;
  3. backward: the accumulator columns 3-4, 6-9, 10 and 11 (= dL_dinv_depths) of backward(dL_dpixels=None, dL_ddistortion=g, ...)
     against float64 per Gaussian in each output's scale:  E_kernel <= 3 max(E_f32, E_spread) + floor["backward"]  -- the kernel
     differs from the restatement by its exp and by the order of its atomics;
     E_f32 is large where late entries of saturated pixels dominate a Gaussian's row (the header's total-minus-prefix suffix sum:
     n1500_opaque 9e-4, n2000 8e-5 on the oracle's buffers), and the bound follows it: that is the stated price of one pass;
  4. columns 0-2, 5, 8 and 12-15 are what they are without the keywords; g = 0 gives the plain call's gradients up to atomic order;
  5. the arena is linear: over four runs each and per arena segment, the mean arena of (dpix + g) and the mean of the float64 sums
     dpix-alone + g-alone differ by at most 3 x (the four-run spread of the one + that of the other), no eps term; the test's
     docstring has the measured figures and says which part of the difference is not atomic noise;
  6. camera_grad and sh_gradient="factored" calls run and agree with the dense call;
  7. the trainer: the hidden scene at --size 100 --views 8 --iterations 300 with and without --lambda-dist, both with
     --report-distortion, ends finite both ways, and the term lowers train_distortion_mean (DIST_GAP_MIN).

Every measured figure is printed as a DISTORTION_ROW JSON line; tools/record_distortion_margins.py files the E_kernel of a run in
tests/golden/distortion_margins.json, and a case on file also fails above 3 x its recorded value.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, sub
import distortion_reference as DR
import features_reference as FR
import parity
from test_gpu_features import _case

pytestmark = pytest.mark.gpu
FRAMES = list(FR.SCENES) + ["toy", "one_gaussian_40x40", "n2000_antialiased", "n2000_filter3d", "n2000_capacity"]
ZERO_FRAMES = ("toy", "one_gaussian_40x40")     # equal depths / one contributor per pixel: Dist = 0 and no gradient, held exactly
_FRAMES = {}


def _row(**kw):
    print("\nDISTORTION_ROW " + json.dumps(kw))


def _recorded(case, key):
    return DR.golden().get("E_kernel", {}).get(case, {}).get(key)


def _bwd_extra(extra):
    return {k: v for k, v in extra.items() if k in ("rasterize_mode", "filter_3d")}


def frame(name):
    """The kernel forward of a frame (background 0), g and the yardstick and restatement on its buffers, once per session."""
    if name not in _FRAMES:
        gsr = pkg()
        sc, cam, kw, extra = _case(name)
        H, W = kw["image_height"], kw["image_width"]
        image, inv_depth, buf = gsr.render_gaussians(**kw, **extra)
        nb = {k: parity.to_np(buf[k]) for k in ("points_xy_image", "conic_opacity", "depths", "point_list", "ranges", "n_contrib")}
        if "capacity" in extra:
            D, over = sub("forward").rendered_count(buf)
            assert not over and 0 < D < extra["capacity"]
            nb["point_list"] = nb["point_list"][:D]
        N = sc["means"].shape[0]
        m32 = parity.to_np(sub("_frame").inv_depth_of(buf, N, image.device)).astype(np.float32)   # what the kernel reads
        r = DR.yardstick(nb, W, H, DR.draw_g(H, W), m=m32.astype(np.float64))
        print(f"\n{name}: D {nb['point_list'].shape[0]}, {int(r['mask'].sum())} of {r['mask'].size} pixels masked")
        assert r["mask"].sum() <= FR.MAX_MASKED * r["mask"].size
        g32 = r["g"].astype(np.float32)                              # zero at the masked pixels: both sides lose them
        dist32, mom32 = DR.forward_f32(nb, W, H, m=m32)
        acc32 = DR.backward_f32(nb, W, H, g32, mom32, m=m32)
        _FRAMES[name] = dict(sc=sc, cam=cam, kw=kw, extra=extra, H=H, W=W, N=N, buf=buf, nb=nb, r=r, g=g32, dist32=dist32, acc32=acc32,
                             gd=torch.as_tensor(g32, device=image.device))
    return _FRAMES[name]


def _accumulators(g, N):
    """The (N, 16) accumulator rows of a backward() result, through the tag densify.DensifyStats.update uses."""
    ws = g["dL_dmean2D"]._gsr_backward_ws[0]
    off = int(sub("_lib").lib().gsr_backward_accumulators_offset(N))
    return ws[off:off + 64 * N].view(torch.float32).view(N, 16)


def _backward(f, dpix=None, g=None, moments=None, **more):
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], dpix)
    if g is not None:
        kw.update(dL_ddistortion=g, distortion_moments=moments)
    return pkg().backward(**kw, **_bwd_extra(f["extra"]), **more)


@pytest.mark.parametrize("name", FRAMES)
def test_forward_against_float64(name):
    dist_mod, feat = sub("distortion"), sub("features")
    f = frame(name)
    H, W, r = f["H"], f["W"], f["r"]
    dist, mom = dist_mod.render_distortion(f["buf"], H, W)
    assert tuple(dist.shape) == (H, W) and tuple(mom.shape) == (H, W, 4)
    assert bool(torch.isfinite(dist).all()) and bool(torch.isfinite(mom).all()) and not bool(mom[..., 3].any())
    assert torch.equal(dist, mom[..., 0] * mom[..., 2]) and bool((dist >= 0).all())
    ones = torch.ones((f["N"], 1), device=dist.device)
    assert torch.equal(mom[..., 0], feat.render_features(ones, f["buf"], H, W)[..., 0])      # A: bit for bit the blended ones
    if name in ZERO_FRAMES:                                          # nothing to measure a relative error against: exactly 0
        assert r["dist"].max() <= 1e-20 and not bool(dist.any()) and not f["dist32"].any()
        return
    E_k, E_32 = DR.forward_error(dist, r), DR.forward_error(f["dist32"], r)
    floor = DR.golden()["floor"]["forward"]
    rec = _recorded(name, "forward")
    _row(test="forward", case=name, E_kernel=E_k, E_f32=E_32, bound=3.0 * E_32 + floor, E_kernel_eps32=E_k / DR.EPS32, E_f32_eps32=E_32 / DR.EPS32,
         recorded=rec)
    assert E_k <= 3.0 * E_32 + floor, (E_k, E_32)
    assert rec is None or E_k <= 3.0 * rec, (E_k, rec)


@pytest.mark.parametrize("name", ["n300_50x37", "n900_faint_48x32", "n1500_opaque_48x48", "behind_n300"])
def test_forward_is_deterministic_and_writes_every_pixel(name):
    dist_mod, feat = sub("distortion"), sub("features")
    if name.startswith("behind"):
        sc, cam, kw, extra = _case(name)
        H, W = kw["image_height"], kw["image_width"]
        buf = pkg().render_gaussians(**kw)[2]
        assert int(buf["point_list"].shape[0]) == 0
    else:
        f = frame(name)
        buf, H, W = f["buf"], f["H"], f["W"]
        assert sub("_frame").masks_of(buf, int(buf["point_list"].shape[0]), buf["ranges"].device) is not None   # the masks are this forward's
    a = dist_mod.render_distortion(buf, H, W)
    b = dist_mod.render_distortion(buf, H, W)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = dist_mod.render_distortion(buf, H, W)
    s.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    d = dist_mod.render_distortion(buf, H, W, use_block_masks=False)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])
    dev = a[0].device
    out = (torch.full((H, W), float("nan"), device=dev), torch.full((H, W, 4), float("nan"), device=dev))
    got = dist_mod.render_distortion(buf, H, W, out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], a[0]) and torch.equal(out[1], a[1])
    if name.startswith("behind"):
        assert not bool(a[0].any()) and not bool(a[1].any())       # a frame without lists: every pixel 0
        g = torch.ones((H, W), device=dev)
        f0 = dict(sc=sc, cam=cam, kw=kw, buf=buf, extra={})
        res = _backward(f0, None, g, a[1])
        assert "dL_dinv_depths" in res and not bool(res["dL_dmean3D"].any()) and not bool(res["dL_dinv_depths"].any())


@pytest.mark.parametrize("name", FRAMES)
def test_backward_against_float64(name):
    dist_mod = sub("distortion")
    f = frame(name)
    H, W, N, r = f["H"], f["W"], f["N"], f["r"]
    _, mom = dist_mod.render_distortion(f["buf"], H, W)
    if name in ZERO_FRAMES:                                          # the gradient of 0: the seven columns, and all the others, exactly 0
        assert r["dist"].max() <= 1e-20 and not f["acc32"].any()      # (Dist >= 0 is at its minimum: its gradient is 0)
        res = _backward(f, None, f["gd"], mom)
        assert not bool(_accumulators(res, N).any()) and not bool(res["dL_dinv_depths"].any())
        return
    E32 = DR.backward_errors(f["acc32"], r)
    E_32 = max(E32.values())
    runs = []
    for _ in range(2):                                               # two like calls for the spread, both held to the bound
        res = _backward(f, None, f["gd"], mom)
        acc = _accumulators(res, N).clone()
        assert torch.equal(res["dL_dinv_depths"], acc[:, 11]) and tuple(res["dL_dinv_depths"].shape) == (N,)
        assert not bool(acc[:, list(DR.UNTOUCHED)].any())           # g alone: the other columns are what a zero image leaves
        assert bool(torch.isfinite(res["_arena"]).all())
        runs.append(parity.to_np(acc))
    Ek = {k: max(DR.backward_errors(a, r)[k] for a in runs) for k in DR.OUTPUTS}
    E_k, E_s = max(Ek.values()), DR.spread(runs[0], runs[1], r)
    floor = DR.golden()["floor"]["backward"]
    rec = _recorded(name, "backward")
    _row(test="backward", case=name, E_kernel=E_k, E_f32=E_32, E_spread=E_s, bound=3.0 * max(E_32, E_s) + floor, per_output=Ek, per_output_f32=E32,
         recorded=rec)
    assert DR.criterion(E_k, E_32, E_s, floor), (Ek, E32, E_s)
    assert rec is None or E_k <= 3.0 * rec, (E_k, rec)
    assert all(np.abs(runs[0][:, c]).max() > 0 for c in DR.TOUCHED)


GRAD_KEYS = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dshs")


def _norm_diff(a, b, keys=GRAD_KEYS):
    """The largest max-norm difference of two results over the optimizer gradients, each relative to its own largest entry."""
    worst = 0.0
    for k in keys:
        x, y = parity.to_np(a[k]).astype(np.float64), parity.to_np(b[k]).astype(np.float64)
        m = max(np.abs(x).max(), np.abs(y).max())
        if m > 0:
            worst = max(worst, float(np.abs(x - y).max() / m))
    return worst


def _dpix(H, W, seed=3):
    return (np.random.default_rng(seed).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)


@pytest.mark.parametrize("name", ["n2000_64x48", "n2000_antialiased"])
def test_other_columns_and_zero_gradient_are_the_plain_calls(name):
    dist_mod = sub("distortion")
    f = frame(name)
    H, W, N = f["H"], f["W"], f["N"]
    _, mom = dist_mod.render_distortion(f["buf"], H, W)
    dpix = _dpix(H, W)
    plain = [_backward(f, dpix, absgrad=True) for _ in range(4)]
    accs = [parity.to_np(_accumulators(p, N)).astype(np.float64) for p in plain]
    spread = np.max([np.abs(accs[i] - accs[j]).max(0) for i in range(4) for j in range(i)], axis=0)   # per column, the six pairs
    with_g = _backward(f, dpix, 100.0 * f["gd"], mom, absgrad=True)
    acc_g = parity.to_np(_accumulators(with_g, N)).astype(np.float64)
    cols = list(DR.UNTOUCHED)
    d = np.abs(acc_g - accs[0]).max(0)
    _row(test="other_columns", case=name, difference=[float(d[c]) for c in cols], spread=[float(spread[c]) for c in cols])
    assert all(d[c] <= 3.0 * spread[c] for c in cols)
    assert all(d[c] > 3.0 * spread[c] for c in (3, 4, 6, 7, 9, 10, 11))                        # ... and the seven it adds to do move
    assert torch.equal(with_g["dL_dmean2D_abs"], _accumulators(with_g, N)[:, 12:14])
    zero = _backward(f, dpix, torch.zeros_like(f["gd"]), mom, absgrad=True)
    s = max(_norm_diff(plain[i], plain[j]) for i in range(4) for j in range(i))
    dz = _norm_diff(zero, plain[0])
    _row(test="zero_gradient", case=name, difference=dz, spread=s)
    assert dz <= 3.0 * s
    assert "dL_dinv_depths" in zero and "dL_dinv_depths" not in plain[0]


def _arena_norm(x, y, offsets, ref):
    """The largest max-norm difference of two float64 arenas over the arena's segments (mean3D | scale | rot | opacity | shs), each
    relative to the largest entry of `ref` in that segment."""
    worst = 0.0
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        m = np.abs(ref[lo:hi]).max()
        if m > 0:
            worst = max(worst, float(np.abs(x[lo:hi] - y[lo:hi]).max() / m))
    return worst


@pytest.mark.parametrize("name", ["n2000_64x48", "n2000_filter3d"])
def test_arena_is_linear_in_the_two_cotangents(name):
    """Four runs of each of the three calls; the sums dpix-alone + g-alone are formed in float64.  Per arena segment, the mean of the
    four combined arenas and the mean of the four sums are compared with the combined spread: the four-run spread of the one plus
    that of the other (two more calls bring their own atomic noise), times the factor 3 this suite gives every four-run range
    (test_gpu_features.py (7): a range of four underestimates what a further run may do).  No eps term.
    Why not the plain spread: part of the difference is not noise.  Measured with eight runs each on n2000_64x48, the rotation
    segment's means differ by 5.857e-7 of its largest entry in every session (17 ulp of the element itself, which is 0.28 of the
    largest), whichever path forms the colour-only arena, against spreads of 9.2e-7 (combined call) and 8.4e-7 (g alone); the
    opacity and SH segments, which the per-Gaussian kernel forms without cancellation, differ by 4e-8.  The per-Gaussian kernel's
    chain from dL_dconic to dL_drot and dL_dscale rounds against intermediates larger than its results, and f32(f(a + b)) is not
    f32(f(a)) + f32(f(b)); the same chain amplifies the accumulators' atomic noise, which is why the spread is its unit."""
    dist_mod = sub("distortion")
    f = frame(name)
    H, W = f["H"], f["W"]
    _, mom = dist_mod.render_distortion(f["buf"], H, W)
    dpix, g = _dpix(H, W), 100.0 * f["gd"]                            # (scaled so that neither term drowns the other)
    arena = lambda res: parity.to_np(res["_arena"]).astype(np.float64)
    both = [arena(_backward(f, dpix, g, mom)) for _ in range(4)]
    alone = [arena(_backward(f, dpix)) for _ in range(4)]
    sums = [a + arena(_backward(f, None, g, mom)) for a in alone]
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
        share = _arena_norm(ref, ref_alone, seg, ref)                 # what the distortion term contributes, in the same norm
        _row(test="linear", case=name, segment=k, difference=d, spread_both=s_both, spread_sum=s_sum, bound=3.0 * (s_both + s_sum), distortion_share=share)
        if not (s_both > 0 and d <= 3.0 * (s_both + s_sum)):
            bad.append((k, d, s_both, s_sum))
        assert k == 4 or share > 100.0 * 3.0 * (s_both + s_sum), (k, share)   # (the SH segment has no distortion term: colour columns)
    assert not bad, f"{name}: (segment, difference, spread_both, spread_sum) {bad}"


def test_camera_grad_and_factored_calls_agree_with_the_dense_call():
    dist_mod = sub("distortion")
    f = frame("n2000_64x48")
    H, W, N = f["H"], f["W"], f["N"]
    _, mom = dist_mod.render_distortion(f["buf"], H, W)
    dpix, g = _dpix(H, W), 100.0 * f["gd"]
    dense = _backward(f, dpix, g, mom)
    cam = _backward(f, dpix, g, mom, camera_grad=True)
    for k in GRAD_KEYS + ("dL_dmean2D", "dL_dconic", "dL_dinv_depths"):
        parity.assert_grad(k, cam[k], dense[k])
    plain_cam = _backward(f, dpix, camera_grad=True)
    for k in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"):
        assert bool(torch.isfinite(cam[k]).all()) and bool(cam[k].any())
    assert float((cam["dL_dviewmatrix"] - plain_cam["dL_dviewmatrix"]).abs().max()) > 0       # the camera kernels read the added columns
    seen = []
    fact = _backward(f, dpix, g, mom, sh_gradient="factored", on_payload=seen.append)
    assert fact["dL_dshs"] is None and len(seen) == 1 and seen[0] is fact["_view_payload"]
    for k in ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dinv_depths"):
        parity.assert_grad(k, fact[k], dense[k])
    plain_fact = _backward(f, dpix, sh_gradient="factored")
    parity.assert_grad("payload", fact["_view_payload"], plain_fact["_view_payload"])             # the colour columns are untouched
    both = _backward(f, dpix, g, mom, sh_gradient="both")
    parity.assert_grad("dL_dshs", both["dL_dshs"], dense["dL_dshs"])
    # without the forward's records the frame is re-packed from the forward's depths
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], dpix)
    packed = {"means2D": f["buf"]["points_xy_image"].clone(), "conic_opacity": f["buf"]["conic_opacity"].clone(), "rgb": f["buf"]["colors"].clone()}
    kw.update(packed, dL_ddistortion=g, distortion_moments=mom)
    with pytest.raises(ValueError, match="depths"):
        pkg().backward(**kw)
    kw["geom_buffer"] = dict(kw["geom_buffer"], depths=f["buf"]["depths"])
    repacked = pkg().backward(**kw)
    assert not pkg().backward.last_call_used_forward_records
    for k in GRAD_KEYS + ("dL_dinv_depths",):
        parity.assert_grad(k, repacked[k], dense[k])


# ---- the trainer ----
# Measured on the MI355X (hidden scene, --size 100 --views 8 --iterations 300; train_distortion_mean without the term -> with it,
# PSNR cost), on three starts, the trainer having no seed flag: --init reference 1.420e-3 -> 9.72e-5 (gap 0.932, -1.05 dB), --init
# random 1.857e-3 -> 1.463e-4 (gap 0.921, -2.56 dB), --init knn 1.416e-3 -> 9.38e-5 (gap 0.934, -1.34 dB).  The weight was chosen
# from {100, 1000} on the first start before the comparison: 1000 lowers the distortion further (5.7e-5) but the render falls to
# 13.3 dB, so 100.  All three starts show the gap: the test requires half the smallest.
DIST_WEIGHT = "100"
DIST_GAP_MIN = 0.46


def _train(tmp_path, tag, *extra):
    log = tmp_path / f"{tag}.jsonl"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--log", str(log), "--print-interval", "1000", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    for line in open(log):
        rec = json.loads(line)
        if rec["record"] == "summary":
            return rec


def test_trainer_lowers_the_distortion(tmp_path):
    base = ["--size", "100", "--views", "8", "--iterations", "300", "--report-distortion"]
    s0 = _train(tmp_path, "plain", *base)
    s1 = _train(tmp_path, "dist", *base, "--lambda-dist", DIST_WEIGHT)
    for s in (s0, s1):
        assert all(s["parameters_finite"].values()) and np.isfinite(s["train_distortion_mean"]) and np.isfinite(s["train_psnr_mean"])
    gap = 1.0 - s1["train_distortion_mean"] / s0["train_distortion_mean"]
    _row(test="trainer", weight=DIST_WEIGHT, distortion_plain=s0["train_distortion_mean"], distortion_with=s1["train_distortion_mean"], gap=gap,
         psnr_plain=s0["train_psnr_mean"], psnr_with=s1["train_psnr_mean"])
    assert gap >= DIST_GAP_MIN, gap
    plain = _train(tmp_path, "absent", "--size", "100", "--views", "8", "--iterations", "2")
    assert "train_distortion_mean" not in plain
