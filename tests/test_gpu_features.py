"""
N-channel feature rendering (csrc/features.hip, include/gsr_features.h) on the MI355X, against the float64 yardstick and the
float32 restatement of tests/features_reference.py, both taken on the KERNEL forward's own buffers.

Frames: the four small scenes of the CPU matrix, the toy scene, a frame with D = 0 (every Gaussian behind the camera) and one with
N = 1, one Gaussian covering every tile of 40 x 40, and the second scene antialiased, under the 3D filter and in capacity mode.
Channels: C in {1, 3, 4, 5, 16, 17, 64}; F and G from U(-1, 1).  A channel's sums do not depend on the other channels, so the
yardstick is taken once per frame at C = 64 and a call with C channels is held to its first C columns.

  1. forward against float64 on the unmasked pixels, in units of max |F|:  E_kernel <= 3 E_f32 + 2^-23
  2. F = [colours, 1, 1 / depth] on a background-0 frame against the product's own image, 1 - final_Ts and inverse-depth image
     (parity.assert_image's contract)
  3. forward determinism: a second call, another stream, with and without the block masks, into an out= full of NaN
  4. backward against float64 per Gaussian row, in units of the row's sum_p w |G|:  E_kernel <= 3 max(E_f32, E_spread) + floor
  5. C = 3: render_features_backward(G) against backward(dL_dpixels=G)["dL_dcolor"], the same sum made by blend_bwd_splat.hip,
     within twice (4)'s bound
  6. a one-hot G: the column sums to 1 - final_Ts[p], every other channel and every culled Gaussian's row is exactly 0
  7. rasterize_features: torch.autograd.grad is the direct backward call; no gradient is computed when none is required
  8. examples/fit_features.py --size 64 --iterations 100 ends finite with a lower loss

Every measured figure is printed as a FEATURES_ROW JSON line; tools/record_features_margins.py files the E_kernel of a run in
tests/golden/features_margins.json, and a case on file also fails above 3 x its recorded value.

(7) "within E_spread": the autograd call IS a direct call, so it differs from one direct run as two direct runs differ from each
other -- by the order in which the float atomics of a row arrive -- and a further run need not fall inside the spread of one pair.
E_spread is therefore the largest spread among four direct runs (six pairs), and the autograd result may differ from a direct one
by three times that: still a plumbing check, some fifty times tighter than (4)'s accuracy bound.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, lego_camera, pkg, render_kwargs, sub
import features_reference as FR
import parity

pytestmark = pytest.mark.gpu
CHANNELS = (1, 3, 4, 5, 16, 17, 64)
C_REF = 64
FRAMES = list(FR.SCENES) + ["toy", "one_gaussian_40x40", "n2000_antialiased", "n2000_filter3d", "n2000_capacity"]
_FRAMES = {}


def _case(name):
    """(scene, kwargs for render_gaussians, extra keyword arguments)"""
    scenes, cameras = sub("scenes"), sub("cameras")
    if name in FR.SCENES:
        sc, cam, kw = FR.scene(scenes, cameras, name)
        return sc, cam, kw, {}
    if name.startswith("n2000_"):
        sc, cam, kw = FR.scene(scenes, cameras, "n2000_64x48")
        if name == "n2000_antialiased":
            return sc, cam, kw, dict(rasterize_mode="antialiased")
        if name == "n2000_filter3d":
            dev = torch.device("cuda", torch.cuda.current_device())
            means = torch.as_tensor(sc["means"], device=dev)
            return sc, cam, kw, dict(filter_3d=torch.full((means.shape[0],), 0.02, dtype=torch.float32, device=dev))
        return sc, cam, kw, dict(capacity=6000, capacity_hint=4382)
    if name == "toy":
        sc, cam = scenes.toy_scene(), cameras.toy_camera(image_width=120, image_height=90)
        return sc, cam, render_kwargs(sc, cam, train_convention=False), {}
    if name == "one_gaussian_40x40":
        cam = lego_camera(cameras, 0, width=40, height=40)
        sc = scenes.synthetic_scene(1, 0.05, 0.6, 1)
        sc["means"][:] = 0.0
        sc["scales"][:] = 3.0
        sc["opacities"][:] = 0.6
        return sc, cam, render_kwargs(sc, cam, width=40, height=40), {}
    if name in ("behind_n300", "behind_n1"):
        n = 300 if name == "behind_n300" else 1
        cam = lego_camera(cameras, 0, width=50, height=37)
        sc = scenes.synthetic_scene(n, 0.05, 0.6, 5)
        c = np.asarray(cam["camera_center"], np.float32)
        fwd = np.asarray(cam["world_to_camera"], np.float64)[:3, 2]
        sc["means"] = (c - 3.0 * fwd + 0.1 * sc["means"]).astype(np.float32)
        return sc, cam, render_kwargs(sc, cam, width=50, height=37), {}
    raise KeyError(name)


def frame(name):
    """The kernel forward of a frame (background 0), F and G at C = 64 and the yardstick on its buffers, once per session."""
    if name not in _FRAMES:
        gsr = pkg()
        sc, cam, kw, extra = _case(name)
        H, W = kw["image_height"], kw["image_width"]
        image, inv_depth, buf = gsr.render_gaussians(**kw, **extra)
        if "capacity" in extra:
            D, over = sub("forward").rendered_count(buf)
            assert not over and 0 < D < extra["capacity"]
        N = sc["means"].shape[0]
        F, G = FR.draw(N, C_REF, H, W)
        nb = {k: parity.to_np(v) for k, v in buf.items()}
        if "capacity" in extra:
            nb["point_list"] = nb["point_list"][:D]
        r = FR.render(nb, W, H, F, G)
        print(f"\n{name}: D {r['D']}, longest list {r['longest']}, {int(r['mask'].sum())} of {r['mask'].size} pixels masked")
        assert r["mask"].sum() <= FR.MAX_MASKED * r["mask"].size
        dev = image.device
        Gm = G.copy()
        Gm[r["mask"]] = 0                                            # both sides lose the masked pixels
        _FRAMES[name] = dict(sc=sc, cam=cam, kw=kw, extra=extra, H=H, W=W, N=N, image=image, inv_depth=inv_depth, buf=buf, nb=nb, r=r,
                             F=F, G=Gm, Fd=torch.as_tensor(F, device=dev), Gd=torch.as_tensor(Gm, device=dev))
    return _FRAMES[name]


def _cols(r, C):
    """The yardstick's first C channels."""
    out = dict(r)
    for k in ("out64", "out32"):
        out[k] = r[k][..., :C]
    for k in ("dF64", "mag", "dF32"):
        out[k] = r[k][:, :C]
    return out


def _row(**kw):
    print("\nFEATURES_ROW " + json.dumps(kw))                # (a line of its own: pytest -s prints its progress dots without one)


def _recorded(case, key):
    return FR.golden().get("E_kernel", {}).get(case, {}).get(key)


@pytest.mark.parametrize("name", FRAMES)
def test_forward_against_float64(name):
    feat = sub("features")
    f = frame(name)
    worst, bad = 0.0, []
    for C in CHANNELS:
        Fc = f["Fd"][:, :C].contiguous()
        out = feat.render_features(Fc, f["buf"], f["H"], f["W"])
        assert tuple(out.shape) == (f["H"], f["W"], C) and bool(torch.isfinite(out).all())
        rc = _cols(f["r"], C)
        E_k, E_32 = FR.forward_error(out, rc, f["F"][:, :C]), FR.forward_error(rc["out32"], rc, f["F"][:, :C])
        _row(test="forward", case=name, C=C, E_kernel=E_k, E_f32=E_32, bound=3.0 * E_32 + 2.0 ** -23)
        worst = max(worst, E_k)
        if not FR.forward_criterion(E_k, E_32):
            bad.append((C, E_k, E_32))
    assert not bad, f"{name}: (C, E_kernel, E_f32) {bad}"
    rec = _recorded(name, "forward")
    _row(test="forward_worst", case=name, E_kernel=worst, recorded=rec)
    assert rec is None or worst <= 3.0 * rec, (worst, rec)


@pytest.mark.parametrize("name", FRAMES)
def test_colour_alpha_and_depth_channels_are_the_products_own_images(name):
    feat = sub("features")
    f = frame(name)
    buf = f["buf"]
    depths = buf["depths"]
    inv = torch.where(depths > 0, 1.0 / torch.where(depths > 0, depths, torch.ones_like(depths)), torch.zeros_like(depths))
    F5 = torch.cat([buf["colors"], torch.ones_like(inv)[:, None], inv[:, None]], 1).contiguous()
    out = feat.render_features(F5, buf, f["H"], f["W"])
    m = {"image": parity.assert_image("image", out[..., :3], parity.to_np(f["image"]))[1],
         "alpha": parity.assert_image("1 - final_Ts", out[..., 3], 1.0 - parity.to_np(buf["final_Ts"]))[1],
         "inv_depth": parity.assert_image("inv_depth", out[..., 4], parity.to_np(f["inv_depth"]))[1]}
    _row(test="own_images", case=name, **m)
    for k, v in m.items():
        rec = _recorded(name, "own_" + k)
        assert rec is None or v <= max(3.0 * rec, 2.0 ** -22), (k, v, rec)


@pytest.mark.parametrize("name", ["n300_50x37", "n900_faint_48x32", "n1500_opaque_48x48", "behind_n300"])
def test_forward_is_deterministic_and_writes_every_pixel(name):
    feat = sub("features")
    if name.startswith("behind"):
        sc, cam, kw, extra = _case(name)
        H, W, N = kw["image_height"], kw["image_width"], sc["means"].shape[0]
        buf = pkg().render_gaussians(**kw)[2]
        assert int(buf["point_list"].shape[0]) == 0
        Fd = torch.as_tensor(FR.draw(N, 17, H, W)[0], device=buf["ranges"].device)
    else:
        f = frame(name)
        buf, H, W, Fd = f["buf"], f["H"], f["W"], f["Fd"][:, :17].contiguous()
        assert sub("_frame").masks_of(buf, int(buf["point_list"].shape[0]), Fd.device) is not None        # the masks are this forward's
    a = feat.render_features(Fd, buf, H, W)
    b = feat.render_features(Fd, buf, H, W)
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = feat.render_features(Fd, buf, H, W)
    s.synchronize()
    assert torch.equal(a, c)
    assert torch.equal(a, feat.render_features(Fd, buf, H, W, use_block_masks=False))
    for C in (3, 64):
        Fc = Fd[:, :C].contiguous() if C <= 17 else torch.cat([Fd] * 4, 1)[:, :C].contiguous()
        out = torch.full((H, W, C), float("nan"), device=Fd.device)
        got = feat.render_features(Fc, buf, H, W, out=out)
        assert got is out and bool(torch.isfinite(out).all())
        assert torch.equal(out, feat.render_features(Fc, buf, H, W))
    if name.startswith("behind"):
        assert not bool(a.any())                                     # a frame without lists: every pixel 0


def _bound(E_32, E_s):
    return 3.0 * max(E_32, E_s) + FR.golden()["floor"]


@pytest.mark.parametrize("name", FRAMES)
def test_backward_against_float64(name):
    feat = sub("features")
    f = frame(name)
    worst, bad = 0.0, []
    for C in CHANNELS:
        Gc = f["Gd"][..., :C].contiguous()
        rc = _cols(f["r"], C)
        E_32 = FR.backward_error(rc["dF32"], rc)
        for masks in (True, False):                                  # each path: two like calls for the spread, both held to the bound
            a = feat.render_features_backward(Gc, f["buf"], f["H"], f["W"], use_block_masks=masks)
            b = feat.render_features_backward(Gc, f["buf"], f["H"], f["W"], use_block_masks=masks)
            assert tuple(a.shape) == (f["N"], C)
            E_k, E_s = max(FR.backward_error(a, rc), FR.backward_error(b, rc)), FR.spread(a, b, rc)
            _row(test="backward", case=name, C=C, masks=masks, E_kernel=E_k, E_f32=E_32, E_spread=E_s, bound=_bound(E_32, E_s))
            worst = max(worst, E_k)
            if not FR.backward_criterion(E_k, E_32, E_s, FR.golden()["floor"]):
                e = FR.backward_errors(a, rc)
                bad.append((C, masks, E_k, E_32, E_s, int(np.argmax(e))))
    assert not bad, f"{name}: (C, masks, E_kernel, E_f32, E_spread, worst Gaussian) {bad}"
    rec = _recorded(name, "backward")
    _row(test="backward_worst", case=name, E_kernel=worst, recorded=rec)
    assert rec is None or worst <= 3.0 * rec, (worst, rec)


@pytest.mark.parametrize("name", list(FR.SCENES) + ["one_gaussian_40x40"])
def test_three_channels_are_the_blend_backwards_dL_dcolor(name):
    gsr, feat = pkg(), sub("features")
    f = frame(name)
    rc = _cols(f["r"], 3)
    G3 = f["Gd"][..., :3].contiguous()
    a = feat.render_features_backward(G3, f["buf"], f["H"], f["W"])
    b = feat.render_features_backward(G3, f["buf"], f["H"], f["W"])
    g = gsr.backward(**backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], f["G"][..., :3].copy()))
    E_32, E_s = FR.backward_error(rc["dF32"], rc), FR.spread(a, b, rc)
    d = FR.spread(a, g["dL_dcolor"].reshape(-1, 3), rc)
    _row(test="dL_dcolor", case=name, difference=d, bound=2.0 * _bound(E_32, E_s))
    assert d <= 2.0 * _bound(E_32, E_s)
    unused = rc["mag"].max(1) == 0
    assert not bool(a[torch.as_tensor(unused, device=a.device)].any())


@pytest.mark.parametrize("name", ["n300_50x37", "n1500_opaque_48x48"])
def test_one_hot_cotangent(name):
    feat = sub("features")
    f = frame(name)
    H, W, buf = f["H"], f["W"], f["buf"]
    Ts = parity.to_np(buf["final_Ts"]).reshape(H, W)
    radii = parity.to_np(buf["radii"]).reshape(-1)
    ys, xs = np.nonzero(Ts < 0.9)
    for C, ch, j in ((5, 2, 0), (64, 40, len(ys) // 2), (17, 16, len(ys) - 1)):
        y, x = int(ys[j]), int(xs[j])
        G = torch.zeros(H, W, C, device=f["Fd"].device)
        G[y, x, ch] = 1.0
        dF = parity.to_np(feat.render_features_backward(G, buf, H, W))
        total = float(dF[:, ch].astype(np.float64).sum())
        _row(test="one_hot", case=name, C=C, pixel=[y, x], column_sum=total, one_minus_T=float(1.0 - Ts[y, x]))
        assert abs(total - (1.0 - float(Ts[y, x]))) <= parity.IMG_TIGHT
        other = np.delete(dF, ch, 1)
        assert not other.any() and (dF[:, ch] >= 0).all()
        assert not dF[radii == 0].any()


@pytest.mark.parametrize("name", ["n2000_64x48"])
def test_rasterize_features_is_differentiable_in_the_features(name):
    feat = sub("features")
    f = frame(name)
    H, W, buf = f["H"], f["W"], f["buf"]
    C = 16
    rc = _cols(f["r"], C)
    Gc = f["Gd"][..., :C].contiguous()
    direct = [feat.render_features_backward(Gc, buf, H, W) for _ in range(4)]
    E_s = max(FR.spread(direct[i], direct[j], rc) for i in range(4) for j in range(i))     # the largest of the six pairs
    allowed = 3.0 * E_s
    F = f["Fd"][:, :C].clone().requires_grad_(True)
    out = feat.rasterize_features(F, buf, H, W)
    assert out.requires_grad and torch.equal(out.detach(), feat.render_features(F.detach(), buf, H, W))
    (g,) = torch.autograd.grad(out, F, Gc)
    d = FR.spread(g, direct[0], rc)
    _row(test="autograd", case=name, difference=d, E_spread=E_s, allowed=allowed)
    assert d <= allowed
    # through a loss, with an optimiser's view of it
    F2 = f["Fd"][:, :C].clone().requires_grad_(True)
    (feat.rasterize_features(F2, buf, H, W) * Gc).sum().backward()
    assert FR.spread(F2.grad, direct[0], rc) <= allowed
    # no gradient required: none computed
    calls = []
    real = feat.render_features_backward
    feat.render_features_backward = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        plain = feat.rasterize_features(f["Fd"][:, :C].contiguous(), buf, H, W)
        assert not plain.requires_grad
        w = torch.ones((), device=plain.device, requires_grad=True)
        (feat.rasterize_features(f["Fd"][:, :C].contiguous(), buf, H, W) * w).sum().backward()
        assert not calls and w.grad is not None
    finally:
        feat.render_features_backward = real


def test_refused_channel_counts_and_a_single_gaussian():
    feat = sub("features")
    f = frame("n300_50x37")
    dev = f["Fd"].device
    for C in (0, 65):
        with pytest.raises(ValueError, match="channels"):
            feat.render_features(torch.zeros(f["N"], C, device=dev), f["buf"], f["H"], f["W"])
        with pytest.raises(ValueError, match="channels"):
            feat.render_features_backward(torch.zeros(f["H"], f["W"], C, device=dev), f["buf"], f["H"], f["W"])
    # N = 1 behind the camera: D = 0, an image of zeros and a row of zeros
    sc, cam, kw, _ = _case("behind_n1")
    H, W = kw["image_height"], kw["image_width"]
    buf = pkg().render_gaussians(**kw)[2]
    assert int(buf["point_list"].shape[0]) == 0
    out = feat.render_features(torch.ones(1, 4, device=dev), buf, H, W, out=torch.full((H, W, 4), float("nan"), device=dev))
    assert not bool(out.any())
    dF = feat.render_features_backward(torch.ones(H, W, 4, device=dev), buf, H, W, out=torch.full((1, 4), float("nan"), device=dev))
    assert not bool(dF.any())


def test_fit_features_example_lowers_its_loss(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fit_features.py"), "--size", "64", "--iterations", "100", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    s = json.loads(p.stdout.strip().splitlines()[-1])
    print("\nFEATURES_ROW " + json.dumps(dict(test="fit_features", **{k: s[k] for k in ("first_loss", "final_loss", "heldout_accuracy", "heldout_covered_pixels")})))
    for k in ("size", "gaussians", "iterations", "first_loss", "final_loss", "loss_curve", "heldout_accuracy", "heldout_covered_pixels"):
        assert k in s, k
    assert s["size"] == 64 and s["iterations"] == 100 and len(s["loss_curve"]) == 10
    assert np.isfinite([s["first_loss"], s["final_loss"], s["heldout_accuracy"]]).all() and np.isfinite(np.asarray(s["loss_curve"], np.float64)).all()
    assert s["final_loss"] < s["first_loss"]
    for png in ("normals.png", "log_scale.png", "labels.png"):
        assert os.path.getsize(os.path.join(str(tmp_path), png)) > 0
