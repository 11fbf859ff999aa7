"""
Absolute screen-space gradients and the densification statistics (include/gsr_densify_stats.h) on the MI355X: `dL_dmean2D_abs`
against the float64 yardstick tests/absgrad_reference.py under parity.assert_grad's contract (SH degree 0 and 3, ragged sizes,
single-tile lists of 12 .. 100 entries so the last bucket takes the <= 16- and <= 32-entry paths, both block shapes in child runs,
masks present and absent, depth + alpha cotangents, capacity mode, D = 0, N = 0; margins printed); properties that need no
reference; the statistics kernels against numpy; GaussianModel(densify_statistic="screen") against the oracle's density control
fed the same averages; a shortened real schedule.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, sub
import absgrad_reference as AR
import f64_reference as F
import parity
import test_f64_reference as R
import test_gpu_f64_reference as G

pytestmark = pytest.mark.gpu

_CUSTOM = {}


def _custom_case(oracle, cameras, key, mk, opacity_scale=1.0):
    """A case dict like test_f64_reference.oracle_case's (without the oracle's backward) for make_case arguments `mk`."""
    if key not in _CUSTOM:
        sc, cam, kw = R.make_case(cameras, **mk)
        if opacity_scale != 1.0:
            sc["opacities"] = (sc["opacities"] * np.float32(opacity_scale)).astype(np.float32)
            kw["opacity"] = sc["opacities"]
        _, _, buf = oracle.render_gaussians(**kw)
        pre = F.preprocess_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
        _CUSTOM[key] = dict(sc=sc, cam=cam, kw=kw, buf=buf, pre=pre)
    return _CUSTOM[key]


def _single_tile(n):
    # faint, wide splats over one 16x16 tile: nearly every entry contributes at every pixel and T stays far above 1e-4, so the
    # whole list is replayed and the compacted stream has ~n entries
    return dict(W=16, H=16, n=n, degree=1, train=True, bg=(0.3, 0.1, 0.2), sm=1.0, seed=100 + n, outside=0.0, behind=0.0, scale=0.35,
                aniso=3.0), 0.04


def _cotangents(H, W, seed, aux):
    rng = np.random.default_rng(seed)
    dpix = (rng.normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)
    if not aux:
        return dpix, None, None
    return dpix, (rng.normal(0, 1, (H, W)) / (H * W)).astype(np.float32), (rng.normal(0, 1, (H, W)) / (H * W)).astype(np.float32)


def _bkw(c, buf, dpix, depths=None):
    b = backward_kwargs(c["sc"], c["cam"], c["kw"], buf, dpix)
    if depths is not None:
        b["geom_buffer"] = dict(b["geom_buffer"], depths=depths)
    return b


def _against_yardstick(c, label, own_chain, aux=False, capacity=False):
    gsr = pkg()
    kw = c["kw"]
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, gA = _cotangents(H, W, 17, aux)
    ref = AR.of_case(c["pre"], c["buf"]["point_list"], c["buf"]["ranges"], dpix, gD, gA)
    if own_chain or capacity:
        extra = {}
        if capacity:
            Dn = int(np.asarray(c["buf"]["point_list"]).shape[0])
            extra = dict(capacity=Dn, capacity_hint=Dn)
        _, _, buf = sub("forward").render_gaussians(**kw, **extra) if capacity else gsr.render_gaussians(**kw)
        for k in ("radii", "ranges"):                                      # the lists the float64 side was given
            parity.assert_exact(k, buf[k], c["buf"][k])
        if not capacity:
            parity.assert_exact("point_list", buf["point_list"], c["buf"]["point_list"])
    else:
        buf = c["buf"]
    g = gsr.backward(**_bkw(c, buf, dpix, depths=buf["depths"] if aux else None), dL_ddepth_image=gD, dL_dalpha_image=gA, absgrad=True)
    bwd = sub("backward").backward
    if not capacity:
        assert bwd.last_call_used_forward_masks is bool(own_chain)
    assert g["dL_dmean2D_abs"].shape == (c["pre"]["N"], 2)
    m_abs = parity.assert_grad("dL_dmean2D_abs", g["dL_dmean2D_abs"], ref["abs"])
    m_sgn = parity.assert_grad("dL_dmean2D", g["dL_dmean2D"][:, :2], ref["signed"])
    print(f"  {label:34s} abs: {m_abs[0]:.6f} within the tight band, max err {m_abs[1]:.3e} max|g|;  signed: {m_sgn[0]:.6f}, {m_sgn[1]:.3e}"
          f"   (max|abs| {np.abs(ref['abs']).max():.3e}, max|signed| {np.abs(ref['signed']).max():.3e})")
    return g


MATRIX = [  # (case name or single-tile n, own chain (masks) / oracle buffers (no masks), depth + alpha cotangents)
    ("16x16_n1", True, False), ("37x29_n63", False, False), ("37x29_n63", True, True), ("64x48_n700_deg0", True, False),
    ("64x48_n700_deg0", False, True), ("64x48_n65", True, True), ("200x136_n3000", True, True), ("200x136_n3000", False, False),
    (12, True, False), (12, False, True), (28, True, True), (28, False, False), (40, True, False), (40, False, True),
    (60, True, True), (60, False, False), (100, True, False), (100, False, True),
]


def _get_case(oracle, cameras, name):
    if isinstance(name, int):
        mk, osc = _single_tile(name)
        return _custom_case(oracle, cameras, f"tile{name}", mk, osc)
    return G._case(oracle, cameras, name)


def test_abs_gradients_against_yardstick(oracle, cameras):
    print(f"\nGSR_BWD_BLOCK = {os.environ.get('GSR_BWD_BLOCK', '(per frame)')}")
    for name, own, aux in MATRIX:
        c = _get_case(oracle, cameras, name)
        if isinstance(name, int):                                          # the list really is that long, and replayed to its end
            assert int(np.asarray(c["buf"]["point_list"]).shape[0]) >= name - 2
            assert int(np.asarray(c["buf"]["n_contrib"]).max()) >= name - 4
        _against_yardstick(c, f"{name} {'masks' if own else 'no masks'}{' +depth+alpha' if aux else ''}", own, aux)
    _against_yardstick(G._case(oracle, cameras, "200x136_n3000"), "200x136_n3000 capacity mode", False, True, capacity=True)


@pytest.mark.parametrize("px", [32, 64])
def test_abs_gradients_with_each_block_shape(px):
    env = dict(os.environ, GSR_BWD_BLOCK=str(px))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "against_yardstick or other_outputs"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(r"\b2 passed", r.stdout), r.stdout[-2000:]


def test_empty_frames_have_zero_abs_gradients(cameras):
    gsr = pkg()
    sc, cam, kw = R.make_case(cameras, W=64, H=48, n=300, degree=3, train=True, bg=(0, 0, 0), sm=1.0, seed=5)
    from conftest import render_kwargs
    empty = {k: np.asarray(v)[:0] for k, v in sc.items()}
    kw0 = render_kwargs(empty, cam, width=64, height=48)
    _, _, b0 = gsr.render_gaussians(**kw0)
    g0 = gsr.backward(**backward_kwargs(empty, cam, kw0, b0, np.ones((48, 64, 3), np.float32)), absgrad=True)
    assert g0["dL_dmean2D_abs"].shape == (0, 2)
    st = sub("densify").DensifyStats(0, "cuda")
    st.update(b0["radii"], g0, use_abs=True)                                # N = 0: nothing enqueued, no error
    behind = dict(sc)                                                       # every Gaussian behind the camera: D = 0
    c = np.asarray(cam["camera_center"], np.float32)
    fwd_dir = np.asarray(cam["world_to_camera"], np.float64)[:3, 2]
    behind["means"] = (c - 3.0 * fwd_dir + 0.1 * (np.asarray(sc["means"]) - c)).astype(np.float32)
    kw1 = render_kwargs(behind, cam, width=64, height=48)
    _, _, b1 = gsr.render_gaussians(**kw1)
    assert int(b1["point_list"].shape[0]) == 0
    g1 = gsr.backward(**backward_kwargs(behind, cam, kw1, b1, np.ones((48, 64, 3), np.float32)), absgrad=True)
    assert g1["dL_dmean2D_abs"].shape == (300, 2) and not torch.any(g1["dL_dmean2D_abs"]) and not torch.any(g1["dL_dmean2D"])
    st = sub("densify").DensifyStats(300, "cuda")
    st.update(b1["radii"], g1, use_abs=True)
    assert not st.grad_accum.any() and not st.vis_count.any() and not st.max_radii.any()


# ---- 2. properties ----
def _c2_frame(view=0):
    gsr = pkg()
    cfg = dict(gsr.scenes.CONFIGS["C2"])
    W, H = cfg.pop("width"), cfg.pop("height")
    sc = gsr.scenes.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"])
    pose = gsr.scenes.LEGO_FRAME0 if view == 0 else gsr.scenes.orbit_pose(view, 8)
    cam = gsr.cameras.nerf_camera(pose, W, H, gsr.scenes.LEGO_CAMERA_ANGLE_X)
    from conftest import render_kwargs
    return sc, cam, render_kwargs(sc, cam, width=W, height=H, bg=(0.1, 0.2, 0.3))


GRAD_ARRAYS = ("dL_dmean3D", "dL_dcolor", "dL_dshs", "dL_dopacity", "dL_dscale", "dL_drot", "dL_dmean2D", "dL_dconic")


def test_absgrad_leaves_the_other_outputs_alone_and_dominates_the_signed_sum():
    gsr = pkg()
    sc, cam, kw = _c2_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    H, W = kw["image_height"], kw["image_width"]
    dpix, _, _ = _cotangents(H, W, 2, False)
    b = lambda: backward_kwargs(sc, cam, kw, buf, dpix)
    snap = lambda g: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.items()}
    plain = gsr.backward(**b())
    # columns 12-13 (and 14-15) of the accumulator records are exactly zero after an unflagged backward
    ws, _, has_abs, n = plain["dL_dmean2D"]._gsr_backward_ws
    assert has_abs is False and "dL_dmean2D_abs" not in plain
    off = int(sub("_lib").lib().gsr_backward_accumulators_offset(n))
    acc = ws[off:off + 64 * n].view(torch.float32).view(n, 16)
    assert plain["dL_dmean2D"].data_ptr() == acc[:, 3:6].data_ptr()
    assert not torch.any(acc[:, 12:16])
    plain = snap(plain)
    flagged = gsr.backward(**b(), absgrad=True)
    assert set(flagged) == set(plain) | {"dL_dmean2D_abs"}
    for k in GRAD_ARRAYS:                                                  # the existing parity contract, flagged against unflagged
        m = parity.assert_grad(k, flagged[k], plain[k])
        print(f"  {k}: {m[0]:.6f} within the tight band, max {m[1]:.2e} max|g|")
    a, s = flagged["dL_dmean2D_abs"].double(), flagged["dL_dmean2D"][:, :2].double()
    slack = parity.GRAD_ABS * float(a.abs().max()) + parity.GRAD_REL * s.abs()
    assert bool(torch.all(a >= s.abs() - slack)) and bool(torch.all(a >= 0))
    vis = a.sum(1) > 0
    assert float((a[vis] > 1.5 * s.abs()[vis]).double().mean()) > 0.05     # and is no copy of it
    assert float(a.sum()) > 1.2 * float(s.abs().sum())


def test_a_single_pixel_gives_abs_equal_to_the_signed_magnitude():
    gsr = pkg()
    sc, cam, kw = _c2_frame()
    _, _, buf = gsr.render_gaussians(**kw)
    H, W = kw["image_height"], kw["image_width"]
    n_contrib = parity.to_np(buf["n_contrib"]).reshape(H, W)
    y, x = np.unravel_index(int(np.argmax(n_contrib)), n_contrib.shape)
    assert n_contrib[y, x] >= 8
    dpix = np.zeros((H, W, 3), np.float32)
    dpix[y, x] = (0.7, -0.4, 0.2)
    g = gsr.backward(**backward_kwargs(sc, cam, kw, buf, dpix), absgrad=True)
    a, s = parity.to_np(g["dL_dmean2D_abs"]).astype(np.float64), np.abs(parity.to_np(g["dL_dmean2D"][:, :2]).astype(np.float64))
    assert int((s > 0).any(1).sum()) >= 8
    # One term per Gaussian, so abs = |signed| up to rounding.  The kernel forms the signed one as a (h dx) + b (h dy) and the
    # absolute one as |h (a dx + b dy)|: a few float32 roundings of each PRODUCT, i.e. of the sum's value times its cancellation
    # factor kappa = (|a dx| + |b dy|) / |a dx + b dy| (likewise c dy + b dx), taken here from the forward's own records.
    xy = parity.to_np(buf["points_xy_image"]).astype(np.float64)
    con = parity.to_np(buf["conic_opacity"]).astype(np.float64)
    dx, dy = xy[:, 0] - x, xy[:, 1] - y
    tiny = 1e-300
    kx = (np.abs(con[:, 0] * dx) + np.abs(con[:, 1] * dy)) / np.maximum(np.abs(con[:, 0] * dx + con[:, 1] * dy), tiny)
    ky = (np.abs(con[:, 2] * dy) + np.abs(con[:, 1] * dx)) / np.maximum(np.abs(con[:, 2] * dy + con[:, 1] * dx), tiny)
    bound = 8 * 2.0 ** -24 * np.stack([kx, ky], 1) * np.maximum(a, s) + 1e-37
    assert np.all(np.abs(a - s) <= bound), float((np.abs(a - s) / bound).max())


# ---- 3. the statistics update ----
def _three_views(absgrad):
    gsr = pkg()
    outs = []
    for view in (0, 2, 5):
        sc, cam, kw = _c2_frame(view)
        sc["means"][view::40] += np.float32(100.0)                          # a few Gaussians far outside this view (others in the next)
        _, _, buf = gsr.render_gaussians(**kw)
        H, W = kw["image_height"], kw["image_width"]
        dpix, _, _ = _cotangents(H, W, 30 + view, False)
        g = gsr.backward(**backward_kwargs(sc, cam, kw, buf, dpix), absgrad=absgrad)
        outs.append((buf["radii"], g))
    return sc["means"].shape[0], outs


@pytest.mark.parametrize("use_abs", [False, True])
def test_stats_update_over_three_views_matches_numpy(use_abs):
    n, outs = _three_views(True)
    st = sub("densify").DensifyStats(n, "cuda")
    acc = np.zeros(n, np.float32)
    cnt, mr = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for radii, g in outs:
        st.update(radii, g, use_abs=use_abs)
        r = parity.to_np(radii).astype(np.int32)
        v = parity.to_np(g["dL_dmean2D_abs"] if use_abs else g["dL_dmean2D"][:, :2]).astype(np.float32)
        norm = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1], dtype=np.float32)
        vis = r > 0
        acc = np.where(vis, acc + norm, acc).astype(np.float32)
        cnt += vis
        mr = np.maximum(mr, np.where(vis, r, 0))
    torch.cuda.synchronize()
    assert np.array_equal(parity.to_np(st.vis_count), cnt) and np.array_equal(parity.to_np(st.max_radii), mr)
    assert cnt.max() == 3 and cnt.min() < 3                                # visible in all three views, and not
    got = parity.to_np(st.grad_accum)
    # float32 rounding: the kernel may fuse gx*gx + gy*gy (1 ulp of the norm) and adds in the same order as numpy
    ulp = np.spacing(np.maximum(acc, np.float32(1e-30)).astype(np.float32))
    assert np.all(np.abs(got.astype(np.float64) - acc) <= 3 * 2 * ulp), float(np.abs(got - acc).max())
    assert np.all(got[cnt == 0] == 0)
    assert got.max() > 0


def test_two_views_from_two_streams_update_one_statistics_set():
    n, outs = _three_views(False)
    densify = sub("densify")
    serial = densify.DensifyStats(n, "cuda")
    for radii, g in outs[:2]:
        serial.update(radii, g)
    both = densify.DensifyStats(n, "cuda")
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for st, (radii, g) in zip(streams, outs[:2]):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            both.update(radii, g)
    for st in streams:
        torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert torch.equal(both.vis_count, serial.vis_count) and torch.equal(both.max_radii, serial.max_radii)
    a, b = parity.to_np(both.grad_accum).astype(np.float64), parity.to_np(serial.grad_accum)
    ulp = np.spacing(np.maximum(b, np.float32(1e-30)))
    assert np.all(np.abs(a - b) <= 2 * 2 * ulp)                            # two additions in either order: 2 ulp each


# ---- 4. mark and prune ----
def _crafted(n=5000, seed=3):
    rng = np.random.default_rng(seed)
    thr, extent, pd = np.float32(2e-4), np.float32(1.7), np.float32(0.01)
    acc = rng.uniform(0, 1.5e-3, n).astype(np.float32)
    cnt = rng.integers(0, 6, n).astype(np.int32)
    acc[:6] = [np.nan, np.inf, -np.inf, 1e-3, thr, np.nextafter(thr, np.float32(0))]
    cnt[:6] = [2, 1, 1, 0, 1, 1]
    acc[6:9] = np.float32(3) * thr                                        # exactly on the edge through the division: 3 thr / 3
    cnt[6:9] = 3
    mr = rng.integers(0, 60, n).astype(np.int32)
    scales = np.exp(rng.normal(np.log(0.017), 0.6, (n, 3))).astype(np.float32)
    scales[10] = pd * extent                                              # max(scale) exactly on the scale threshold: a clone, not a split
    op = rng.uniform(0, 0.02, n).astype(np.float32)
    op[11] = np.float32(0.005)                                            # exactly the threshold: pruned (> is strict)
    return thr, extent, pd, acc, cnt, mr, scales, op


def _dev_params(n, scales, op):
    densify = sub("densify")
    P = densify.alloc_params(n, torch.device("cuda", torch.cuda.current_device()))
    P["scales"].copy_(torch.as_tensor(scales))
    P["opacities"].copy_(torch.as_tensor(op))
    return P


def _dev_stats(acc, cnt, mr):
    st = sub("densify").DensifyStats(len(acc), "cuda")
    st.grad_accum.copy_(torch.as_tensor(acc))
    st.vis_count.copy_(torch.as_tensor(cnt))
    st.max_radii.copy_(torch.as_tensor(mr))
    return st


def _np_avg(acc, cnt):
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = (acc / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
    return np.where(np.isfinite(avg), avg, np.float32(0))


def test_mark_and_prune_kernels_match_numpy_exactly():
    densify = sub("densify")
    thr, extent, pd, acc, cnt, mr, scales, op = _crafted()
    n = len(acc)
    extra = 137                                                            # rows a clone added since: no statistics, average 0
    rng = np.random.default_rng(9)
    scales_all = np.concatenate([scales, np.exp(rng.normal(np.log(0.017), 0.6, (extra, 3))).astype(np.float32)])
    op_all = np.concatenate([op, rng.uniform(0, 0.02, extra).astype(np.float32)])
    P, st = _dev_params(n + extra, scales_all, op_all), _dev_stats(acc, cnt, mr)
    avg = np.concatenate([_np_avg(acc, cnt), np.zeros(extra, np.float32)])
    mr_all = np.concatenate([mr, np.zeros(extra, np.int32)])
    smax = scales_all.max(1)
    sthr = np.float32(pd * extent)
    for split in (False, True):
        got = parity.to_np(densify.mark_candidates_stats(P, st, thr, extent, pd, split))
        want = ((avg >= thr) & ((smax > sthr) if split else (smax <= sthr))).astype(np.int32)
        assert np.array_equal(got, want), (split, int((got != want).sum()))
        assert want[:n].sum() > 50 and not want[n:].any()
    assert avg[0] == 0 and avg[1] == 0 and avg[2] == 0 and avg[3] == np.float32(1e-3)       # NaN, +-inf -> 0; count 0 divides by 1
    clone = parity.to_np(densify.mark_candidates_stats(P, st, thr, extent, pd, False))
    assert clone[4] == (smax[4] <= sthr) and clone[5] == 0 and clone[10] == (avg[10] >= thr)
    for max_screen, max_world in ((0.0, 0.0), (20.0, 0.0), (0.0, 0.03), (20.0, 0.03), (-1.0, -1.0)):
        got = parity.to_np(densify.prune_mask_stats(P, st, 0.005, max_screen, max_world))
        want = op_all > np.float32(0.005)
        if max_screen > 0:
            want &= ~(mr_all.astype(np.float32) > np.float32(max_screen))
        if max_world > 0:
            want &= ~(smax > np.float32(max_world))
        assert np.array_equal(got, want.astype(np.int32)), (max_screen, max_world)
        assert 0 < want.sum() < len(want)
    base = parity.to_np(densify.prune_mask_stats(P, st, 0.005))
    assert np.array_equal(base, parity.to_np(densify.prune_mask(P, 0.005))) and base[11] == 0       # no size terms: gsr_prune_mark's rule


# ---- 5. the model ----
def test_screen_model_follows_the_oracle_on_the_same_averages():
    """The screen path is the reference sequence on another statistic: fed the oracle's density control a 3D gradient whose norm
    IS the average (g = (avg, 0, 0); sqrt(avg^2) = avg in float32), both must clone, split, remove and prune the same rows."""
    from oracle import densify as od
    from test_gpu_densify import assert_params_equal, to_dev
    from test_oracle_densify import make_params
    densify = sub("densify")
    for n, it, cfg in ((3000, 600, {"max_allowed_prune_ratio": 1.0}), (3000, 3000, {"max_allowed_prune_ratio": 1.0}), (3000, 650, {}),
                       (20000, 1200, {"max_allowed_prune_ratio": 1.0, "densify_grad_threshold": 0.0004, "percent_dense": 0.02})):
        p, g = make_params(n, seed=n + it)
        rng = np.random.default_rng(n + it)
        cnt = rng.integers(0, 5, n).astype(np.int32)
        norm = np.linalg.norm(np.asarray(g, np.float64).reshape(n, 3), axis=1)
        acc = (norm * rng.uniform(0.5, 2.0, n) * np.maximum(cnt, 1)).astype(np.float32)
        avg = _np_avg(acc, cnt)
        g_avg = np.zeros((n, 3), np.float32)
        g_avg[:, 0] = avg
        model = densify.GaussianModel(to_dev(p), config=dict(cfg, densify_statistic="screen"), scene_extent=1.0)
        assert model.stats.n == n and not model.stats.grad_accum.any()
        model.stats.grad_accum.copy_(torch.as_tensor(acc))
        model.stats.vis_count.copy_(torch.as_tensor(cnt))
        old = model.stats
        log = model.densification_and_pruning(it)
        ref, ref_log = od.densification_and_pruning(p, g_avg, it, dict({"background_color": [0.0, 0.0, 0.0]}, **cfg), 1.0)
        assert log == ref_log, (log, ref_log)
        assert_params_equal(model.params, ref)
        ran = it > 500 and it % 100 == 0
        if ran:                                                            # a call that ran: a zeroed set of the new size
            assert log["cloned"] > 0 and log["split"] > 0
            assert model.stats is not old and model.stats.n == model.num_points
            assert not model.stats.grad_accum.any() and not model.stats.vis_count.any() and not model.stats.max_radii.any()
        else:
            assert model.stats is old and torch.equal(old.vis_count.cpu(), torch.as_tensor(cnt))


def test_screen_model_size_terms_and_the_untouched_reference_path():
    from oracle import densify as od
    from test_gpu_densify import assert_params_equal, to_dev
    from test_oracle_densify import make_params
    densify = sub("densify")
    n = 4000
    p, g = make_params(n, seed=77)
    rng = np.random.default_rng(77)
    mr = rng.integers(0, 60, n).astype(np.int32)
    cfg = {"max_allowed_prune_ratio": 1.0, "densify_grad_threshold": 1e9, "densify_statistic": "screen", "prune_screen_size": 40.0,
           "prune_world_size": 0.05, "opacity_reset_interval": 3000}
    scales = np.asarray(od._shape(p)["scales"]).reshape(n, 3)
    op = np.asarray(od._shape(p)["opacities"]).reshape(n)

    def run(it):
        model = densify.GaussianModel(to_dev(p), config=cfg, scene_extent=2.0)
        model.stats.max_radii.copy_(torch.as_tensor(mr))
        model.stats.vis_count.fill_(1)
        log = model.densification_and_pruning(it)
        assert log["cloned"] == 0 and log["split"] == 0
        return model, log

    for it, sized in ((2900, False), (3100, True)):                        # the size terms apply once iteration > opacity_reset_interval
        model, log = run(it)
        valid = op > np.float32(0.005)
        if sized:
            valid &= ~(mr > 40) & ~(scales.max(1) > np.float32(0.05 * 2.0))
        count = int(valid[:-1].sum())                                      # the exclusive scan's last entry (the reference's count)
        assert model.num_points == count and log["pruned"] == n - count
        keep = np.where(valid)[0][:count]
        assert np.array_equal(parity.to_np(model.params["positions"]), np.asarray(od._shape(p)["positions"]).reshape(n, 3)[keep])
        assert model.stats.n == count and not model.stats.max_radii.any()
    # "reference" is today's path: the oracle's sequence on the 3D gradient, and it owns no statistics
    model = densify.GaussianModel(to_dev(p), config={"max_allowed_prune_ratio": 1.0}, scene_extent=1.0)
    assert model.stats is None and model.densify_statistic == "reference"
    model.grads["positions"].copy_(torch.as_tensor(g))
    log = model.densification_and_pruning(600)
    ref, ref_log = od.densification_and_pruning(p, g, 600, {"background_color": [0.0, 0.0, 0.0], "max_allowed_prune_ratio": 1.0}, 1.0)
    assert log == ref_log
    assert_params_equal(model.params, ref)
    with pytest.raises(ValueError, match="densify_statistic"):
        densify.GaussianModel(to_dev(p), config={"densify_statistic": "blurry"})


def test_screen_radius_prune_follows_rows_through_the_split_compaction():
    """With a split in the same call the rows move before the prune: the screen-radius term must still remove the Gaussians whose
    radius was too large (and only those, the opacity rule aside)."""
    from test_gpu_densify import to_dev
    from test_oracle_densify import make_params
    densify = sub("densify")
    n = 3000
    p, _ = make_params(n, seed=5)
    dev_p = to_dev(p)
    dev_p["opacities"].fill_(0.5)                                          # nothing pruned by opacity
    rng = np.random.default_rng(5)
    mr = rng.integers(0, 60, n).astype(np.int32)
    smax = parity.to_np(dev_p["scales"]).reshape(n, 3).max(1)
    acc = np.where(rng.uniform(0, 1, n) < 0.3, 1.0, 0.0).astype(np.float32)   # 30 % above any threshold
    cfg = {"max_allowed_prune_ratio": 1.0, "densify_statistic": "screen", "prune_screen_size": 40.0, "opacity_reset_interval": 100}
    model = densify.GaussianModel(dev_p, config=cfg, scene_extent=1.0)
    model.stats.grad_accum.copy_(torch.as_tensor(acc))
    model.stats.vis_count.fill_(1)
    model.stats.max_radii.copy_(torch.as_tensor(mr))
    pos0 = parity.to_np(dev_p["positions"]).reshape(n, 3).copy()
    log = model.densification_and_pruning(600)
    assert log["split"] > 0 and log["split_removed"] > 0 and log["cloned"] > 0
    split = (acc > 0) & (smax > np.float32(0.01))                          # (the post-clone arrays end in a clone: every flag is counted)
    survivors = ~split & ~(mr > 40)                                        # original rows that stay: not split away, not too large
    got = parity.to_np(model.params["positions"]).reshape(-1, 3)
    want = pos0[survivors]
    assert np.array_equal(got[:len(want)], want)                           # original rows keep their order in front of the added ones
    # + 1: the last valid row is dropped by the count (the exclusive scan's last entry), as in every compaction here
    assert log["pruned"] == int((~split & (mr > 40)).sum()) + 1


# ---- 6. a shortened real schedule ----
def test_screen_absgrad_schedule_on_lego(tmp_path):
    """examples/train.py on the committed Lego views, 900 iterations: density control at 600, 700, 800 on the absolute screen-space
    statistics with the D-SSIM loss."""
    log = tmp_path / "train.jsonl"
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
           "--iterations", "900", "--gaussians", "5000", "--print-interval", "300", "--log", str(log), "--densify-stat", "screen", "--absgrad",
           "--densify-grad-threshold", "0.0006", "--lambda-dssim", "0.2"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    recs = [json.loads(l) for l in open(log)]
    calls = [r for r in recs if r["record"] == "density_control" and r["iteration"] > 0]
    summary = [r for r in recs if r["record"] == "summary"][0]
    curve = np.concatenate([np.asarray(r["l1"], np.float64) for r in recs if r["record"] == "loss"])
    print("\npoints after each density-control call:", " ".join(f"{r['iteration']}:{r['points']}" for r in calls),
          f"; {summary['iterations_per_s']} it/s; L1 first/last hundred {curve[:100].mean():.5f} / {curve[-100:].mean():.5f}")
    assert [r["iteration"] for r in calls] == [600, 700, 800]
    assert all(r["cloned"] + r["split"] > 0 for r in calls), calls
    pts = [r["points"] for r in calls]
    assert pts[-1] > pts[0], pts                                           # N grows
    assert all(summary["parameters_finite"].values()), summary["parameters_finite"]
    assert np.isfinite(curve).all() and curve[-100:].mean() < curve[:100].mean()


def test_statistics_fill_between_density_control_calls_and_clear_after():
    """The trainer's loop in miniature: backward(absgrad=True) + update for a few views, then a density-control call."""
    gsr = pkg()
    densify = sub("densify")
    sc, cam, kw = _c2_frame()
    n = sc["means"].shape[0]
    t = lambda a, shape: torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).cuda()
    P = {"positions": t(sc["means"], (n, 3)), "scales": t(sc["scales"], (n, 3)), "rotations": t(sc["rotations"], (n, 4)),
         "opacities": t(sc["opacities"], (n,)), "shs": t(sc["shs"], (n * 16, 3))}
    model = densify.GaussianModel(P, config={"densify_statistic": "screen", "max_allowed_prune_ratio": 1.0, "densify_grad_threshold": 1e-7},
                                  scene_extent=1.0)
    _, outs = _three_views(True)
    for radii, g in outs:
        model.stats.update(radii, g, use_abs=True)
    assert float(model.stats.grad_accum.max()) > 0 and int(model.stats.vis_count.max()) == 3 and int(model.stats.max_radii.max()) > 0
    log = model.densification_and_pruning(600)
    assert log["cloned"] + log["split"] > 0 and model.num_points != n
    assert model.stats.n == model.num_points and not model.stats.grad_accum.any() and not model.stats.vis_count.any()
