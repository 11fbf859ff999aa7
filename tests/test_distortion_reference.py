"""
The yardstick of the depth-distortion regulariser (tests/distortion_reference.py) and the float32 restatement of
include/gsr_distortion.h, checked on the CPU oracle's buffers.  No GPU.

  1. the two-pass yardstick (blend_grads_f64 with colour (1, m, m^2)) equals torch float64 autograd of the ordered double sum
     sum_i sum_{j<i} w_i w_j (m_i - m_j)^2 to 1e-10 of each output's scale.  The kernels pass the gradient through the 0.99 cap, so
     autograd does too (STRAIGHT_THROUGH_CAP); with a plain clamp instead a frame with capped entries must fail the same bound;
  2. closed forms: one contributor gives 0, equal depths give 0, two entries give w1 w2 (m1 - m2)^2, Dist >= 0, and a shift of every
     m leaves the float64 value unchanged;
  3. a thin slab, every inverse depth within a relative 1e-4 of one value: per pixel the restatement's running form stays within
     (0.5 n + 1) eps32 (1 + mu / sigma), n the pixel's n_contrib -- the first-order bound n u kappa of the updating algorithm for a
     mean and a central moment (Chan, Golub & LeVeque 1983; u = eps32 / 2), plus one eps32 for the weights and the final product --
     and the A M2 - M1^2 form, whose error is kappa times larger, must fail it (the bound's two numbers are on file);
  4. the restatement's forward and backward errors on the four scenes: their smallest are the `floor` entries of
     tests/golden/distortion_margins.json, which the GPU test's bounds add; the intact restatement passes the criterion.
"""
import numpy as np
import pytest
import torch

import blend_grad_reference as B
import distortion_reference as DR
import features_reference as FR
import frame_walk_reference as FWR

STRAIGHT_THROUGH_CAP = True
_CASES = {}


def oracle_case(oracle, scenes, cameras, name):
    """{buf (the oracle's forward, background 0), W, H, g, r (the yardstick)}, once per session.  "capped": n300 with every opacity
    1, so that alpha = min(0.99, o G) is capped near every centre."""
    if name not in _CASES:
        if name == "capped":
            from conftest import lego_camera, render_kwargs
            args, _, W, H = FR.SCENES["n300_50x37"]
            sc = scenes.synthetic_scene(*args)
            sc["opacities"][:] = 1.0
            kw = render_kwargs(sc, lego_camera(cameras, 0, width=W, height=H), width=W, height=H)
        else:
            sc, cam, kw = FR.scene(scenes, cameras, name)
        H, W = kw["image_height"], kw["image_width"]
        buf = oracle.render_gaussians(**kw)[2]
        g = DR.draw_g(H, W)
        _CASES[name] = dict(buf=buf, W=W, H=H, g=g, r=DR.yardstick(buf, W, H, g))
    return _CASES[name]


def autograd_of_the_double_sum(c, straight_through):
    """{output: (N, width) float64} by torch autograd, in the kernel's units (mean2D x 0.5 (W, H), conic b halved)."""
    buf, W, H, r = c["buf"], c["W"], c["H"], c["r"]
    xy0, co0, _, _ = FWR.arrays(buf)
    xy = torch.tensor(xy0, requires_grad=True)
    con = torch.tensor(co0[:, :3].copy(), requires_grad=True)
    op = torch.tensor(co0[:, 3].copy(), requires_grad=True)
    m = torch.tensor(r["m"], requires_grad=True)
    g = torch.as_tensor(r["g"])
    loss = torch.zeros((), dtype=torch.float64)
    capped = 0
    for _, xs, ys, idx, _, masked, active in r["tiles"]:
        idx_t, act = torch.as_tensor(idx), torch.as_tensor(active)
        dx = xy[idx_t, 0][None, :] - torch.as_tensor(xs, dtype=torch.float64)[:, None]
        dy = xy[idx_t, 1][None, :] - torch.as_tensor(ys, dtype=torch.float64)[:, None]
        A, Bc, C = con[idx_t, 0][None, :], con[idx_t, 1][None, :], con[idx_t, 2][None, :]
        a_raw = op[idx_t][None, :] * torch.exp(-0.5 * (A * dx * dx + C * dy * dy) - Bc * dx * dy)
        cap = torch.clamp(a_raw, max=0.99)
        alpha = a_raw + (cap - a_raw).detach() if straight_through else cap
        capped += int(((a_raw.detach() > 0.99) & act & ~torch.as_tensor(masked)[:, None]).sum())
        om = torch.where(act, 1.0 - alpha, torch.ones_like(alpha))
        T = torch.cumprod(torch.cat([torch.ones(len(xs), 1, dtype=torch.float64), om[:, :-1]], 1), 1)
        w = torch.where(act, alpha * T, torch.zeros_like(alpha))
        pair = (m[idx_t][:, None] - m[idx_t][None, :]) ** 2          # the ordered double sum is half the symmetric one
        dist = 0.5 * ((w @ pair) * w).sum(1)
        loss = loss + (dist * g[ys, xs]).sum()
    dxy, dcon, dop, dm = torch.autograd.grad(loss, (xy, con, op, m))
    dcon = dcon.numpy()
    return {"dL_dmean2D": dxy.numpy() * np.array([0.5 * W, 0.5 * H]),
            "dL_dconic": np.stack([dcon[:, 0], 0.5 * dcon[:, 1], np.zeros(len(dcon)), dcon[:, 2]], 1),
            "dL_dopacity": dop.numpy()[:, None], "dL_dinv_depths": dm.numpy()[:, None]}, capped


@pytest.mark.parametrize("name", ["n300_50x37", "n1500_opaque_48x48", "capped"])
def test_yardstick_is_autograd_of_the_ordered_double_sum(oracle, scenes, cameras, name):
    c = oracle_case(oracle, scenes, cameras, name)
    r = c["r"]
    assert r["mask"].sum() <= FR.MAX_MASKED * r["mask"].size
    got, capped = autograd_of_the_double_sum(c, STRAIGHT_THROUGH_CAP)
    E = {k: B.worst(got[k], r[k]) for k in DR.OUTPUTS}
    print(f"\n{name}: capped (pixel, entry) pairs {capped}; " + ", ".join(f"{k} {v:.2e}" for k, v in E.items()))
    assert max(E.values()) <= 1e-10, E
    assert all(np.abs(r[k]["signed"]).max() > 0 for k in DR.OUTPUTS)
    if name == "capped":
        assert capped > 0
        off, _ = autograd_of_the_double_sum(c, False)               # the switch: a plain clamp stops the gradient at the cap
        E_off = {k: B.worst(off[k], r[k]) for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity")}
        print("plain clamp: " + ", ".join(f"{k} {v:.2e}" for k, v in E_off.items()))
        assert min(E_off.values()) > 1e-10, E_off


def _hand_frame(xy, conic, opacity, depths, W=16, H=16):
    """One 16x16 tile, every Gaussian in its list in the order given, so broad and faint that every pixel applies every entry."""
    n = len(depths)
    co = np.concatenate([np.tile(np.asarray(conic, np.float32), (n, 1)), np.asarray(opacity, np.float32).reshape(n, 1)], 1)
    return {"points_xy_image": np.asarray(xy, np.float32).reshape(n, 2), "conic_opacity": co, "depths": np.asarray(depths, np.float32),
            "point_list": np.arange(n, dtype=np.int32), "ranges": np.array([[0, n]], np.int32), "n_contrib": np.full((H, W), n, np.int32)}


def test_closed_forms():
    rng = np.random.default_rng(3)
    conic = (1e-3, 2e-4, 1.5e-3)

    def frame(n, depths):
        return _hand_frame(rng.uniform(4, 12, (n, 2)), conic, rng.uniform(0.1, 0.5, n), depths)

    one = DR.moments_f64(frame(1, [2.0]), 16, 16)
    assert not one["mask"].any() and (one["A"] > 0).all() and not one["dist"].any()          # one contributor: exactly 0
    same = DR.moments_f64(frame(5, [3.0] * 5), 16, 16)
    assert not same["mask"].any() and np.abs(same["dist"]).max() <= 1e-28                     # equal depths
    two = DR.moments_f64(frame(2, [2.0, 4.0]), 16, 16)
    w = two["tiles"][0][4]
    assert not two["mask"].any() and w.shape == (256, 2) and (w > 0).all()
    want = np.zeros((16, 16))
    want[two["tiles"][0][2], two["tiles"][0][1]] = w[:, 0] * w[:, 1] * (0.5 - 0.25) ** 2
    assert np.abs(two["dist"] - want).max() <= 1e-12 * want.max()
    many_b = frame(12, rng.uniform(1.5, 6.0, 12))
    many = DR.moments_f64(many_b, 16, 16)
    assert not many["mask"].any() and (many["dist"] >= 0).all() and many["dist"].max() > 0
    w, m = many["tiles"][0][4], many["m"]
    pairs = np.zeros(256)
    for i in range(12):                                                                   # the ordered double sum itself
        for j in range(i):
            pairs += w[:, i] * w[:, j] * (m[i] - m[j]) ** 2
    got = many["dist"][many["tiles"][0][2], many["tiles"][0][1]]
    assert np.abs(got - pairs).max() <= 1e-12 * pairs.max()
    shifted = DR.moments_f64(many_b, 16, 16, m=m + 0.5)
    assert np.abs(shifted["dist"] - many["dist"]).max() <= 1e-12 * many["dist"].max()


def test_thin_slab_running_form_holds_and_moment_form_fails(oracle, scenes, cameras):
    c = oracle_case(oracle, scenes, cameras, "n300_50x37")
    buf, W, H = c["buf"], c["W"], c["H"]
    N = np.asarray(buf["points_xy_image"]).reshape(-1, 2).shape[0]
    m32 = (0.25 * (1.0 + 1e-4 * np.random.default_rng(5).uniform(-1, 1, N))).astype(np.float32)
    r = DR.moments_f64(buf, W, H, m=m32.astype(np.float64))                               # float64 on the float32 numbers
    bound = DR.golden()["thin_slab_bound"]
    assert bound == {"per_entry": 0.5, "base": 1.0}
    keep = ~r["mask"] & (r["dist"] > 0)
    kappa = r["mu"][keep] / np.sqrt(r["S"][keep] / r["A"][keep])
    allowed = (bound["per_entry"] * r["n_contrib64"][keep] + bound["base"]) * DR.EPS32 * (1.0 + kappa) * r["dist"][keep]
    worst = {}
    for form in ("running", "moments"):
        dist = DR.forward_f32(buf, W, H, m=m32, form=form)[0].astype(np.float64)
        err = np.abs(dist[keep] - r["dist"][keep])
        worst[form] = float((err / allowed).max())
        print(f"\n{form}: worst error {worst[form]:.3g} of the bound; in eps32 mu / sigma "
              f"{float((err / (DR.EPS32 * (1.0 + kappa) * r['dist'][keep])).max()):.3g}; kappa {kappa.min():.3g} .. {kappa.max():.3g}")
    assert keep.sum() > 500 and kappa.min() > 5e3
    assert worst["running"] <= 1.0
    assert worst["moments"] > 1.0


def _e_f32(c):
    buf, W, H, r = c["buf"], c["W"], c["H"], c["r"]
    if "E_f32" not in c:
        dist, mom = DR.forward_f32(buf, W, H)
        acc = DR.backward_f32(buf, W, H, r["g"].astype(np.float32), mom)
        assert not acc[:, list(DR.UNTOUCHED)].any()
        c["E_f32"] = (DR.forward_error(dist, r), DR.backward_errors(acc, r))
    return c["E_f32"]


def test_floors_on_file_are_the_smallest_f32_margins(oracle, scenes, cameras):
    E = {n: _e_f32(oracle_case(oracle, scenes, cameras, n)) for n in FR.SCENES}
    floor = DR.golden()["floor"]
    for n, (ef, eb) in E.items():
        print(f"\n{n}: E_f32 forward {ef:.3e} ({ef / DR.EPS32:.2f} eps32 (1 + mu / sigma)); backward " + ", ".join(f"{k} {v:.3e}" for k, v in eb.items()))
    fwd = [ef for ef, _ in E.values()]
    bwd = [max(eb.values()) for _, eb in E.values()]
    print(f"floor on file: forward {floor['forward']:.3e}, backward {floor['backward']:.3e}; smallest here {min(fwd):.3e}, {min(bwd):.3e}")
    assert all(np.isfinite(v) and v > 0 for v in fwd + bwd)
    assert floor["forward"] <= 2.0 * min(fwd) and floor["backward"] <= 2.0 * min(bwd)      # (the libm's expf may differ from the one they were recorded with)
    assert floor["forward"] >= 0.5 * min(fwd) and floor["backward"] >= 0.5 * min(bwd)
    for ef, eb in E.values():                                                              # the intact restatement passes
        assert DR.criterion(ef, ef, 0.0, floor["forward"]) and DR.criterion(max(eb.values()), max(eb.values()), 0.0, floor["backward"])


def test_the_criterion_sees_a_dropped_suffix_term(oracle, scenes, cameras):
    """A backward that forgets the suffix term of dL/dalpha (q = T u alone: backward_f32(drop_suffix=True)) is far outside the bound."""
    c = oracle_case(oracle, scenes, cameras, "n300_50x37")
    _, eb = _e_f32(c)
    r, floor = c["r"], DR.golden()["floor"]["backward"]
    _, mom = DR.forward_f32(c["buf"], c["W"], c["H"])
    acc = DR.backward_f32(c["buf"], c["W"], c["H"], r["g"].astype(np.float32), mom, drop_suffix=True)
    E = DR.backward_errors(acc, r)
    print(f"\nE = " + ", ".join(f"{k} {v:.3e}" for k, v in E.items()) + f" against E_f32 {max(eb.values()):.3e}, floor {floor:.3e}")
    assert E["dL_dinv_depths"] <= 3.0 * eb["dL_dinv_depths"] + floor          # (dL/dm does not pass through dL/dalpha)
    for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity"):
        assert not DR.criterion(E[k], max(eb.values()), 0.0, floor) and E[k] > 100 * (3.0 * max(eb.values()) + floor), k
