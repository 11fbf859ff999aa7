"""The 3D smoothing filter on the MI355X (include/gsr_filter3d.h) against its float64 yardstick (tests/filter3d_reference.py), on
the case matrix that tests/test_filter3d_reference.py checks on the CPU.

The three bounds K eps32 x (error model) come from tests/golden/filter3d_margins.json: per kernel, the worst ratio measured on the
MI355X on this matrix against the yardstick (`worst`) and the bound, ten times that (`K`).  measure() is the one place that forms
the ratios; the tests print the figures before they assert.

Substitution (item 4): the forward is compared bit for bit.  Two backward calls on one frame differ in the float-atomic order of
the blend stage, so their arrays are held to parity.assert_grad, as everywhere in this suite; what the keyword adds is checked bit
for bit inside ONE call, whose gradients are caught before and after the transpose."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, render_kwargs, sub
import f64_reference as F64
import filter3d_reference as R
import parity

pytestmark = pytest.mark.gpu
EPS = R.EPS32
MARGINS = os.path.join(ROOT, "tests", "golden", "filter3d_margins.json")


def _dev():
    return torch.device("cuda", 0)


def _t(a, shape):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).to(_dev())


@pytest.fixture(scope="module")
def cases(scenes, cameras):
    out = {}
    for name in R.CASE_NAMES:
        c = R.make_case(scenes, cameras, name)
        c["sampling"] = R.sampling_f64(c["scene"]["means"], c["cams"])
        out[name] = c
    return out


def _check_filter(name, got, seen, nu_view, z_cond, excluded):
    """`got` (N,) float32 against the views `seen` (V', N): the seen set through the value, unseen bits, the error ratio."""
    masked = np.where(seen, nu_view, 0.0)
    nu, arg = masked.max(0) if seen.shape[0] else np.zeros(got.shape[0]), masked.argmax(0) if seen.shape[0] else np.zeros(got.shape[0], int)
    any_seen = nu > 0
    if not (any_seen & ~excluded).any():
        if not any_seen.any():
            assert not got.view(np.uint32).any(), name                                  # nothing seen: zeros, exactly
        return 0.0
    keep = any_seen & ~excluded
    exp = np.sqrt(np.float64(np.float32(0.2))) / nu[keep]
    cond = z_cond[arg[keep], np.nonzero(keep)[0]]
    ratio = np.abs(got[keep].astype(np.float64) - exp) / exp / (EPS * cond)
    # a view wrongly seen or missed moves nu by far more than any rounding: the ratio test is the seen-set test
    unseen = ~any_seen & ~excluded
    top = got.max()
    assert (got[unseen].view(np.uint32) == np.float32(top).view(np.uint32)).all(), name   # the bits of the largest seen filter_3d
    assert (got[~unseen] == top).any() and (got > 0).all(), name
    return float(ratio.max())


def measure(cases):
    """{"from_views", "apply", "backward"}: the worst error ratio of each kernel on the matrix, with every exact property asserted."""
    Fm = sub("filter3d")
    worst = {"from_views": 0.0, "apply": 0.0, "backward": 0.0}
    for name, c in cases.items():
        sc, sm = c["scene"], c["sampling"]
        N = sc["means"].shape[0]
        means = _t(sc["means"], (N, 3))
        excl_pairs = R.near_threshold(sm)
        excluded = excl_pairs.any(0)
        assert excluded.sum() <= R.MAX_EXCLUDED * N, name
        f = Fm.compute_filter_3d(means, c["cams"])
        again = Fm.compute_filter_3d(means, c["cams"])
        assert torch.equal(f.view(torch.int32), again.view(torch.int32)), name             # two runs: identical bits
        got = f.cpu().numpy()
        worst["from_views"] = max(worst["from_views"], _check_filter(name, got, sm["seen"], sm["nu_view"], sm["z_cond"], excluded))
        for v in range(len(c["cams"])):                                                    # view by view: which views see a Gaussian
            one = Fm.compute_filter_3d(means, c["cams"][v:v + 1]).cpu().numpy()
            worst["from_views"] = max(worst["from_views"], _check_filter(f"{name} view {v}", one, sm["seen"][v:v + 1], sm["nu_view"][v:v + 1],
                                                                         sm["z_cond"][v:v + 1], excl_pairs[v]))
        # ---- apply ----
        f0 = f.clone()
        f0[::7] = 0.0
        s_t, o_t = _t(sc["scales"], (N, 3)), _t(sc["opacities"], (N,))
        sp, op = Fm.apply_filter_3d(s_t, o_t, f0)
        fz = f0.cpu().numpy()
        e_s, e_o = (t.numpy() for t in R.apply_f64(sc["scales"], sc["opacities"], fz))
        g_s, g_o = sp.cpu().numpy(), op.cpu().numpy()
        off = fz == 0
        assert (g_s[off].view(np.uint32) == sc["scales"][off].view(np.uint32)).all(), name   # f == 0: bit-identical
        assert (g_o[off].view(np.uint32) == sc["opacities"].reshape(-1)[off].view(np.uint32)).all(), name
        sp_abs, op_abs = Fm.apply_filter_3d(s_t.abs(), o_t, f0)
        assert torch.equal(sp[~torch.as_tensor(off)], sp_abs[~torch.as_tensor(off)]) and torch.equal(op, op_abs), name   # a negative scale: its magnitude's s'
        worst["apply"] = max(worst["apply"], float((np.abs(g_s - e_s) / np.abs(e_s)).max() / EPS), float((np.abs(g_o - e_o) / np.abs(e_o)).max() / EPS))
        # ---- backward ----
        rng = np.random.default_rng(N + len(name))
        c_s, c_o = rng.normal(0, 1, (N, 3)).astype(np.float32), rng.normal(0, 1, N).astype(np.float32)
        ds_ref, do_ref = R.transpose_autograd(sc["scales"], sc["opacities"], fz, c_s, c_o)
        _, _, mag = R.transpose_closed(sc["scales"], sc["opacities"], fz, c_s, c_o)
        out = torch.full((N, 3), float("nan"), device=_dev()), torch.full((N,), float("nan"), device=_dev())
        ds, do = Fm.filter_3d_backward(s_t, o_t, f0, _t(c_s, (N, 3)), _t(c_o, (N,)), out=out)
        arena = torch.zeros(4 * N + 8, device=_dev())                                        # in place, in arena-like segments
        a_s, a_o = arena[:3 * N].view(N, 3), arena[(3 * N + 3) & ~3:((3 * N + 3) & ~3) + N]
        a_s.copy_(_t(c_s, (N, 3))), a_o.copy_(_t(c_o, (N,)))
        ver = arena._version
        Fm.filter_3d_backward(s_t, o_t, f0, a_s, a_o)
        assert arena._version > ver                                                          # the write is reported
        assert torch.equal(a_s.view(torch.int32), ds.view(torch.int32)) and torch.equal(a_o.view(torch.int32), do.view(torch.int32)), name
        ds, do = ds.cpu().numpy().astype(np.float64), do.cpu().numpy().astype(np.float64)
        assert (ds[off] == c_s[off]).all() and (do[off] == c_o[off]).all(), name
        nz = mag > 0
        worst["backward"] = max(worst["backward"], float((np.abs(ds - ds_ref)[nz] / mag[nz]).max() / EPS),
                                float((np.abs(do - do_ref) / np.abs(do_ref)).max() / EPS))
    return worst


def test_three_kernels_against_the_yardstick(cases):
    """Items 1-3.  Bounds: K eps32 per kernel, K = ten times the worst ratio measured on the MI355X on this matrix."""
    worst = measure(cases)
    print("\nworst error ratios (units of eps32 x error model):", json.dumps(worst))
    with open(MARGINS) as fh:
        m = json.load(fh)
    for k, w in worst.items():
        assert abs(m[k]["K"] - 10.0 * m[k]["worst"]) <= 1e-9 * m[k]["K"]
        assert w <= m[k]["K"], f"{k}: worst ratio {w:.3f} above K = {m[k]['K']:.3f} (measured {m[k]['worst']:.3f})"


def test_no_view_and_nothing_seen_give_zeros(cases):
    Fm = sub("filter3d")
    c = cases["257-3"]
    means = _t(c["scene"]["means"], (-1, 3))
    assert not Fm.compute_filter_3d(means, []).view(torch.int32).any()                       # V = 0
    assert not Fm.compute_filter_3d(means * 0 + 1e4, c["cams"]).view(torch.int32).any()      # all unseen
    out = torch.full((257,), float("nan"), device=_dev())
    assert Fm.compute_filter_3d(means, [], out=out) is out and not out.view(torch.int32).any()
    assert Fm.compute_filter_3d(means[:0], c["cams"]).shape == (0,)


# ------------------------------------------------------------------------------------------- items 4-6: the keyword
def _render_case(scenes, cameras, n=700, scale=0.03, seed=5, size=(96, 72)):
    sc = scenes.synthetic_scene(n, scale, 0.6, seed)
    cams = R.lego_cameras(cameras, 3, sizes=(size,))
    kw = render_kwargs(sc, cams[0], bg=(0.1, 0.2, 0.3))
    N = n
    dev_sc = {"means": _t(sc["means"], (N, 3)), "scales": _t(sc["scales"], (N, 3)), "rotations": _t(sc["rotations"], (N, 4)),
              "opacities": _t(sc["opacities"], (N,)), "shs": _t(sc["shs"], (N * 16, 3))}
    f = sub("filter3d").compute_filter_3d(dev_sc["means"], cams)
    return sc, dev_sc, cams, kw, f


def _kw_dev(kw, d, scales=None, opacity=None):
    return dict(kw, means3D=d["means"], sh=d["shs"], rotations=d["rotations"], scales=d["scales"] if scales is None else scales,
                opacity=d["opacities"] if opacity is None else opacity)


def _bkw(kw, d, cam, buf, dpix, scales=None, opacity=None):
    sc = {"means": d["means"], "shs": d["shs"], "rotations": d["rotations"], "scales": d["scales"] if scales is None else scales,
          "opacities": d["opacities"] if opacity is None else opacity}
    return backward_kwargs(sc, cam, kw, buf, dpix)


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("capacity", [False, True])
def test_forward_keyword_is_substitution_bit_for_bit(scenes, cameras, mode, capacity):
    gsr, Fm = pkg(), sub("filter3d")
    sc, d, cams, kw, f = _render_case(scenes, cameras)
    s1, o1 = Fm.apply_filter_3d(d["scales"], d["opacities"], f)
    extra = {"rasterize_mode": mode}
    if capacity:
        D = int(gsr.render_gaussians(**_kw_dev(kw, d, s1, o1), **extra)[2]["point_list"].shape[0])
        extra.update(capacity=D + 17, capacity_hint=D)
    got = sub("forward").render_gaussians(**_kw_dev(kw, d), **extra, filter_3d=f)
    ref = sub("forward").render_gaussians(**_kw_dev(kw, d, s1, o1), **extra)
    parity.assert_exact("image", got[0], ref[0])
    parity.assert_exact("inverse depth", got[1], ref[1])
    assert set(got[2]) == set(ref[2])
    Dv = sub("forward").rendered_count(got[2])[0] if capacity else None
    for k in ref[2]:
        a, b = (got[2][k][:Dv], ref[2][k][:Dv]) if (capacity and k == "point_list") else (got[2][k], ref[2][k])
        parity.assert_exact(k, a, b)
    assert int(got[2]["point_list"].shape[0]) > 0
    plain = gsr.render_gaussians(**_kw_dev(kw, d), rasterize_mode=mode)
    assert not torch.equal(plain[0], got[0])


@pytest.mark.parametrize("options", [dict(), dict(absgrad=True, camera_grad=True), dict(rasterize_mode="antialiased"), dict(readback=True)])
def test_backward_keyword_is_substitution(scenes, cameras, monkeypatch, options):
    gsr, Fm, B = pkg(), sub("filter3d"), sub("backward")
    options = dict(options)
    readback = options.pop("readback", False)
    mode = {k: v for k, v in options.items() if k == "rasterize_mode"}
    sc, d, cams, kw, f = _render_case(scenes, cameras)
    H, W = kw["image_height"], kw["image_width"]
    dpix = (np.random.default_rng(3).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)
    s1, o1 = Fm.apply_filter_3d(d["scales"], d["opacities"], f)
    fwd = gsr.render_gaussians(**_kw_dev(kw, d), **mode, filter_3d=f)
    ref_fwd = gsr.render_gaussians(**_kw_dev(kw, d, s1, o1), **mode)
    caught = {}
    real = Fm.filter_3d_backward

    def spy(scales, opacity, filt, g_s, g_o, out=None):
        caught["pre"] = (g_s.clone(), g_o.clone())
        caught["raw"] = (scales, opacity, filt)
        return real(scales, opacity, filt, g_s, g_o, out=out)
    monkeypatch.setattr(Fm, "filter_3d_backward", spy)
    bk = _bkw(kw, d, cams[0], fwd[2], dpix)
    if readback:                                   # cov3D read back: a copy of the forward's tensor carries no recompute tag
        bk["cov3Ds"] = fwd[2]["cov3Ds"].clone()
    got = gsr.backward(**bk, **options, filter_3d=f)
    assert B.backward.last_call_recomputed_sigma3d == (not readback)
    monkeypatch.setattr(Fm, "filter_3d_backward", real)
    # inside the one call: the transpose of what the substituted scene's backward left, bit for bit, on the raw parameters
    assert caught["raw"][0].data_ptr() == d["scales"].data_ptr() and caught["raw"][1].data_ptr() == d["opacities"].data_ptr() and caught["raw"][2] is f
    exp = real(d["scales"], d["opacities"], f, *caught["pre"], out=(torch.empty_like(caught["pre"][0]), torch.empty_like(caught["pre"][1])))
    assert torch.equal(got["dL_dscale"].view(torch.int32), exp[0].view(torch.int32))
    assert torch.equal(got["dL_dopacity"].view(torch.int32), exp[1].view(torch.int32))
    # the frame's scene IS apply_filter_3d's output
    tag = fwd[2]["conic_opacity"]._gsr_filter_3d
    assert torch.equal(tag[0].view(torch.int32), s1.view(torch.int32)) and torch.equal(tag[1].view(torch.int32), o1.view(torch.int32))
    # against a second call on the substituted scene: equal up to the float-atomic order of the blend stage
    rbk = _bkw(kw, d, cams[0], ref_fwd[2], dpix, s1, o1)
    if readback:
        rbk["cov3Ds"] = ref_fwd[2]["cov3Ds"].clone()
    ref = gsr.backward(**rbk, **options)
    for k in ("dL_dmean3D", "dL_drot", "dL_dshs", "dL_dcolor", "dL_dmean2D", "dL_dconic"):
        parity.assert_grad(k, got[k], parity.to_np(ref[k]))
    parity.assert_grad("pre-transpose dL_dscale", caught["pre"][0], parity.to_np(ref["dL_dscale"]))
    parity.assert_grad("pre-transpose dL_dopacity", caught["pre"][1], parity.to_np(ref["dL_dopacity"]))
    for k in ("dL_dmean2D_abs", "dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"):
        assert (k in got) == (k in ref)
        if k in got:
            parity.assert_grad(k, got[k], parity.to_np(ref[k]))
    assert not torch.equal(got["dL_dscale"], caught["pre"][0])


def test_backward_refuses_the_wrong_frame_on_the_gpu(scenes, cameras):
    gsr = pkg()
    sc, d, cams, kw, f = _render_case(scenes, cameras, n=257)
    H, W = kw["image_height"], kw["image_width"]
    dpix = np.zeros((H, W, 3), np.float32)
    plain = gsr.render_gaussians(**_kw_dev(kw, d))
    with pytest.raises(ValueError, match="not an unfiltered frame"):
        gsr.backward(**_bkw(kw, d, cams[0], plain[2], dpix), filter_3d=f)
    fwd = gsr.render_gaussians(**_kw_dev(kw, d), filter_3d=f)
    with pytest.raises(ValueError, match="pass the same tensor"):
        gsr.backward(**_bkw(kw, d, cams[0], fwd[2], dpix))
    with pytest.raises(ValueError, match="another filter tensor"):
        gsr.backward(**_bkw(kw, d, cams[0], fwd[2], dpix), filter_3d=f.clone())
    gsr.backward(**_bkw(kw, d, cams[0], fwd[2], dpix), filter_3d=f)
    d["scales"].mul_(1.0)                                                                    # written in place since the forward
    with pytest.raises(ValueError, match="written in place since"):
        gsr.backward(**_bkw(kw, d, cams[0], fwd[2], dpix), filter_3d=f)


def test_it_is_a_real_change(scenes, cameras):
    """Item 5: 1e-4-scale Gaussians, rendered at a quarter of the training views' focal length."""
    gsr, Fm = pkg(), sub("filter3d")
    sc = scenes.synthetic_scene(500, 1e-4, 0.1, 9)
    sc["scales"] = np.full_like(sc["scales"], 1e-4)
    N = 500
    d = {"means": _t(sc["means"], (N, 3)), "scales": _t(sc["scales"], (N, 3)), "rotations": _t(sc["rotations"], (N, 4)),
         "opacities": _t(sc["opacities"], (N,)), "shs": _t(sc["shs"], (N * 16, 3))}
    train = R.lego_cameras(cameras, 3, sizes=((400, 400),))
    f = Fm.compute_filter_3d(d["means"], train)
    far = R.lego_cameras(cameras, 1, sizes=((100, 100),))[0]                                 # same field of view, a quarter of the focal length
    kw = render_kwargs(sc, far)
    a = gsr.render_gaussians(**_kw_dev(kw, d), filter_3d=f)
    b = gsr.render_gaussians(**_kw_dev(kw, d))
    assert not torch.equal(a[0], b[0])
    vis = (a[2]["radii"] > 0) & (b[2]["radii"] > 0)
    assert vis.sum() > 50
    assert (a[2]["conic_opacity"][:, 3][vis] < b[2]["conic_opacity"][:, 3][vis]).all()       # a smaller effective opacity, every visible one


def test_whole_chain_against_float64(scenes, cameras):
    """Item 6: render -> L1 -> backward(filter_3d=) against f64_reference's backward of the substituted scene with the yardstick's
    autograd transpose in front, under parity.assert_grad's contract."""
    gsr, Fm = pkg(), sub("filter3d")
    sc, d, cams, kw, f = _render_case(scenes, cameras, n=400, size=(64, 48))
    H, W = kw["image_height"], kw["image_width"]
    fwd = gsr.render_gaussians(**_kw_dev(kw, d), filter_3d=f)
    target = torch.full((H, W, 3), 0.5, device=_dev())
    _, dpix = gsr.loss.l1_loss_and_gradients(fwd[0], target)
    got = gsr.backward(**_bkw(kw, d, cams[0], fwd[2], dpix), filter_3d=f)
    s1, o1 = Fm.apply_filter_3d(d["scales"], d["opacities"], f)
    sub_scene = dict(sc, scales=s1.cpu().numpy(), opacities=o1.cpu().numpy().reshape(-1, 1))
    buf = {k: parity.to_np(v) for k, v in fwd[2].items()}
    ref = F64.backward_f64(sub_scene, kw, buf["point_list"], buf["ranges"], parity.to_np(dpix))
    ds, do = R.transpose_autograd(sc["scales"], sc["opacities"], f.cpu().numpy(), ref["dL_dscale"], np.asarray(ref["dL_dopacity"]).reshape(-1))
    ref = dict(ref, dL_dscale=ds, dL_dopacity=do.reshape(np.asarray(ref["dL_dopacity"]).shape))
    for k in parity.GRAD_KEYS:
        parity.assert_grad(k, parity.to_np(got[k]).reshape(np.asarray(ref[k]).shape), ref[k])


# ------------------------------------------------------------------------------------------- item 7: the trainer
def test_trainer_under_the_filter_sized_and_capacity(tmp_path):
    gsr = pkg()
    runs = {}
    for label, extra in (("sized", []), ("capacity", ["--capacity"])):
        log, out = tmp_path / f"{label}.jsonl", tmp_path / label
        cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
               "--size", "100", "--iterations", "700", "--filter-3d", "--lambda-dssim", "0.2", "--eval-scales", "1,2", "--print-interval", "50",
               "--log", str(log), "--output", str(out), "--save-interval", "699", *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
        recs = [json.loads(l) for l in open(log)]
        summary = [r for r in recs if r["record"] == "summary"][0]
        calls = [r for r in recs if r["record"] == "density_control" and r["iteration"] >= 0
                 and (r["cloned"] or r["split"] or r["pruned"] or r["opacity_reset"])]
        filt = [r for r in recs if r["record"] == "filter_3d"]
        curve = np.concatenate([np.asarray(r["l1"], np.float64) for r in recs if r["record"] == "loss"])
        print(f"\n{label}: points {[r['points'] for r in calls]}, filter records {[(r['iteration'], r['why'], r['points']) for r in filt]}, "
              f"{summary['iterations_per_s']} it/s, scales {summary['train_eval_scales']}")
        assert len(calls) >= 2                                                               # two density-control calls
        assert all(summary["parameters_finite"].values())
        assert filt[0]["iteration"] == -1 and filt[0]["why"] == "start"
        by_it = {r["iteration"]: r for r in filt}
        for r in calls:                                                                      # a record per recomputation, its length N
            assert by_it[r["iteration"]]["points"] == r["points"], (r, by_it.get(r["iteration"]))
        assert all(np.isfinite([r["min"], r["median"], r["max"]]).all() and 0 < r["min"] <= r["median"] <= r["max"] for r in filt)
        assert curve[-1] < curve[50]                                                         # test_gpu_train_real.py's criterion
        assert set(summary["train_eval_scales"]) == {"1", "2"} and all(np.isfinite(list(v.values())).all() for v in summary["train_eval_scales"].values())
        assert abs(summary["train_eval_scales"]["1"]["psnr"] - summary["train_psnr_mean"]) < 1e-6
        ply = gsr.point_cloud.load_ply(str(out / "point_cloud" / "iteration_699" / "point_cloud.ply"))
        n = summary["points_final"]
        assert ply["positions"].shape[0] == n == filt[-1]["points"]
        assert (np.abs(ply["scales"]) >= filt[-1]["min"] * (1 - 1e-6)).all()                 # fused: no scale below the smallest filter
        for k in ("positions", "scales", "rotations", "opacities", "shs"):
            assert np.isfinite(np.asarray(ply[k])).all(), k
        runs[label] = (curve, summary)
    # The same trajectory: two sized runs of one command drift apart by float-atomic order alone -- up to 3.9e-3 in a loss line after
    # a density-control call and 1.6 % in the final point count (profiles/capacity_train_lego/README.md) -- so, as in
    # test_gpu_capacity.py, the capacity run is held to 1e-2 in the loss (here the mean of the last 50 lines, which drifts no more
    # than its lines) and 5 % in the point count.  Measured here: 5.2e-3 and 1.2 % (profiles/filter3d/gpu_tests.txt).
    a, b = runs["sized"], runs["capacity"]
    drift = abs(a[0][-50:].mean() - b[0][-50:].mean()) / a[0][-50:].mean()
    print(f"sized against capacity: final points {a[1]['points_final']} / {b[1]['points_final']}, loss drift {drift:.2e}")
    assert abs(a[1]["points_final"] - b[1]["points_final"]) <= 0.05 * a[1]["points_final"]
    assert drift <= 1e-2


def test_trainer_recomputes_on_the_interval_once_density_control_has_ended(tmp_path):
    """--densify-until 100: from iteration 100 on the filter is recomputed every --filter-3d-interval iterations, poses refined or not
    (with --optimize-poses the cameras it is computed from have moved in between)."""
    for label, extra in (("fixed", []), ("poses", ["--optimize-poses"])):
        log = tmp_path / f"{label}.jsonl"
        cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
               "--size", "100", "--iterations", "260", "--filter-3d", "--filter-3d-interval", "50", "--densify-from", "20", "--densify-interval", "40",
               "--densify-until", "100", "--print-interval", "100", "--log", str(log), *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
        recs = [json.loads(l) for l in open(log)]
        summary = [r for r in recs if r["record"] == "summary"][0]
        filt = [r for r in recs if r["record"] == "filter_3d"]
        print(f"\n{label}: filter records {[(r['iteration'], r['why'], r['points']) for r in filt]}")
        assert [r["iteration"] for r in filt if r["why"] == "interval"] == [100, 150, 200, 250]
        assert all(r["iteration"] < 100 for r in filt if r["why"] != "interval")
        assert all(r["points"] == summary["points_final"] for r in filt if r["why"] == "interval")   # the point set is final by then
        assert all(np.isfinite([r["min"], r["median"], r["max"]]).all() and 0 < r["min"] <= r["median"] <= r["max"] for r in filt)
        assert all(summary["parameters_finite"].values())


def test_save_ply_writes_the_fused_values(scenes, cameras, tmp_path):
    gsr, Fm = pkg(), sub("filter3d")
    sc, d, cams, kw, f = _render_case(scenes, cameras, n=257)
    P = {"positions": d["means"], "scales": d["scales"], "rotations": d["rotations"], "opacities": d["opacities"], "shs": d["shs"]}
    gsr.point_cloud.save_ply(P, str(tmp_path / "fused.ply"), 257, filter_3d=f)
    gsr.point_cloud.save_ply(P, str(tmp_path / "raw.ply"), 257)
    fused, raw = gsr.point_cloud.load_ply(str(tmp_path / "fused.ply")), gsr.point_cloud.load_ply(str(tmp_path / "raw.ply"))
    s1, o1 = Fm.apply_filter_3d(d["scales"], d["opacities"], f)
    assert np.array_equal(fused["scales"].view(np.uint32), s1.cpu().numpy().view(np.uint32))
    assert np.array_equal(fused["opacities"].view(np.uint32), o1.cpu().numpy().view(np.uint32))
    assert np.array_equal(raw["scales"], sc["scales"]) and np.array_equal(raw["opacities"], sc["opacities"].reshape(-1))
    for k in ("positions", "rotations", "shs", "colors"):
        assert np.array_equal(fused[k], raw[k]), k
