"""
The yardstick of the ray-plane intersection depth (tests/plane_depth_reference.py) and the float32 restatement of
include/gsr_plane_depth.h, checked on the CPU oracle's buffers.  No GPU.

  1. the restatement against the yardstick on features_reference.SCENES: its errors are on file as E_f32 in
     tests/golden/plane_depth_margins.json, which the GPU test's bounds use; the yardstick equals torch float64 autograd of a dense
     restatement of the image to 1e-10 of each output's scale;
  2. the closed form: 144 equal flat discs whose centres lie on one plane tilted by 45 degrees, their normals the plane's.  Every
     m_k(p) is then the plane's inverse depth at p whatever the weights are, so out / (1 - final_T) is (n . r(p)) / (n . mu0) within a
     few eps32 on the covered pixels, while the centre-depth image of the same frame is off by more than a margin computed from
     slope x footprint;
  3. each fallback branch (zero normal, behind the camera, inside the near plane, grazing, round) and the clamp on a large, near,
     steep Gaussian;
  4. the margin cap: the smallest distance of any input kept here from a branch or clamp threshold is printed and exceeds 100 eps32 of
     the compared quantity, so that float32 and float64 cannot decide differently;
  5. the header's (d) formulas in float64 against autograd of (a) and (b), and their float32 restatement against both.
"""
import json

import numpy as np
import pytest
import torch

import blend_grad_reference as B
import frame_walk_reference as FWR
import features_reference as FR
import normal_render_reference as NR
import plane_depth_reference as PD

_CASES = {}
f32 = np.float32


def oracle_case(oracle, scenes, cameras, name):
    """{fr, nb, W, H, slopes, fallback, r (the yardstick), ...} on the oracle's forward (background 0), once per session."""
    if name not in _CASES:
        sc, cam, kw = FR.scene(scenes, cameras, name)
        H, W = kw["image_height"], kw["image_width"]
        nb = oracle.render_gaussians(**kw)[2]
        view = np.asarray(kw["viewmatrix"], f32)
        n32, _, _ = NR.normals_f32(sc["scales"], sc["rotations"], sc["means"], view)
        sl, fb = PD.slopes_f32(n32, PD.plane_scales(sc["scales"]), sc["means"], view, kw["tan_fovx"], kw["tan_fovy"], W, H)
        invd = PD.inv_depth_of_buffers(nb)
        r = PD.yardstick(nb, W, H, invd, sl, PD.draw_g(H, W))
        _CASES[name] = dict(sc=sc, cam=cam, kw=kw, nb=nb, W=W, H=H, view=view, n=n32, slopes=sl, fallback=fb, invd=invd, r=r,
                            fr=PD.frame_of_buffers(nb, W, H, invd))
    return _CASES[name]


def _e_f32(c):
    if "E_f32" not in c:
        r = c["r"]
        img, _ = PD.render_f32(c["fr"], c["slopes"])
        acc, mom = PD.render_backward_f32(c["fr"], c["slopes"], r["g"].astype(f32), img)
        assert not acc[:, list(PD.UNTOUCHED)].any()
        c["img32"], c["acc32"], c["mom32"] = img, acc, mom
        c["E_f32"] = (PD.image_error(img, r, c["invd"]), PD.backward_errors(acc, mom, r))
    return c["E_f32"]


def test_restatement_errors_are_the_ones_on_file(oracle, scenes, cameras):
    for name in PD.CPU_FRAMES:                           # every row first: tools/record_plane_depth_margins.py files them
        print("\nPLANE_DEPTH_F32 " + json.dumps({"case": name, "E_f32": _e_f32(oracle_case(oracle, scenes, cameras, name))[1]}))
    gold = PD.golden()
    floor_seen = []
    for name in PD.CPU_FRAMES:
        c = oracle_case(oracle, scenes, cameras, name)
        r = c["r"]
        assert r["mask"].mean() <= FR.MAX_MASKED, name
        # the frame exercises both branches and the clamp, and every kept clamp decision is outside the cap
        assert 0.05 < c["fallback"].mean() < 0.95 and r["clamp_margin"] > PD.MARGIN_CAP, (name, c["fallback"].mean(), r["clamp_margin"])
        ef, eb = _e_f32(c)
        print(f"\n{name}: fallback {c['fallback'].mean():.2f}, clamped pairs {r['clamped']}, clamp margin {r['clamp_margin'] / PD.EPS32:.0f} eps32, "
              f"masked {int(r['mask'].sum())}; image {ef:.3e}; " + ", ".join(f"{k} {v:.3e}" for k, v in eb.items()))
        rec = gold["E_f32"][name]
        assert ef <= 8 * PD.EPS32                       # a sum of weights <= 1 times inverse depths within [invd / 4, 4 invd]
        for k, v in eb.items():
            # (the libm's expf may differ from the recorded one; a tenth of eps32 of slack for the outputs whose errors are below eps32)
            assert np.isfinite(v) and 0.5 * rec[k] - 0.1 * PD.EPS32 <= v <= 2.0 * rec[k] + 0.1 * PD.EPS32, (name, k, v, rec[k])
        floor_seen.append(max(eb.values()))
    assert 0.5 * min(floor_seen) <= gold["floor"] <= 2.0 * min(floor_seen)
    assert sum(oracle_case(oracle, scenes, cameras, n)["r"]["clamped"] for n in PD.CPU_FRAMES) > 0     # the clamp is met on the matrix


def autograd_dense(c):
    """{output: (N, width) float64} by torch autograd of sum_p g[p] sum_k w_k(p) m_k(p) in the kernel's units: m from leaves
    (invd, gx, gy) and the STAGED xy held constant in it, the float32 clamp decisions of the yardstick's rule."""
    nb, W, H, r = c["nb"], c["W"], c["H"], c["r"]
    xy0, co0, pl, rg = FWR.arrays(nb)
    xy = torch.tensor(xy0, requires_grad=True)
    con = torch.tensor(co0[:, :3].copy(), requires_grad=True)
    op = torch.tensor(co0[:, 3].copy(), requires_grad=True)
    invd = torch.tensor(c["invd"].astype(np.float64))
    sl = torch.tensor(c["slopes"].astype(np.float64))
    m_par = torch.zeros((len(xy0), 3), dtype=torch.float64, requires_grad=True)      # an offset to (invd, gx, gy): its gradient, weighted, is the moments
    g = torch.as_tensor(r["g"])
    tiles = []
    B.blend_grads_f64(xy0, co0[:, :3], co0[:, 3], np.ones((len(xy0), 3)), np.zeros(len(xy0)), pl, rg, np.zeros(3), W, H, np.ones((H, W, 3)),
                      on_tile=lambda tile, xs, ys, idx, active, terms, masked: tiles.append((xs, ys, idx, active)))
    xy32, i32, s32 = c["fr"]["xy"], c["invd"], c["slopes"]
    loss = torch.zeros((), dtype=torch.float64)
    for xs, ys, idx, active in tiles:
        idx_t, act = torch.as_tensor(idx), torch.as_tensor(active)
        px, py = torch.as_tensor(xs, dtype=torch.float64)[:, None], torch.as_tensor(ys, dtype=torch.float64)[:, None]
        dx, dy = xy[idx_t, 0][None, :] - px, xy[idx_t, 1][None, :] - py
        A, Bc, C = con[idx_t, 0][None, :], con[idx_t, 1][None, :], con[idx_t, 2][None, :]
        a_raw = op[idx_t][None, :] * torch.exp(-0.5 * (A * dx * dx + C * dy * dy) - Bc * dx * dy)
        alpha = a_raw + (torch.clamp(a_raw, max=0.99) - a_raw).detach()
        om = torch.where(act, 1.0 - alpha, torch.ones_like(alpha))
        T = torch.cumprod(torch.cat([torch.ones(len(xs), 1, dtype=torch.float64), om[:, :-1]], 1), 1)
        w = torch.where(act, alpha * T, torch.zeros_like(alpha))
        dx32, dy32 = xy32[idx, 0][None, :] - xs[:, None].astype(f32), xy32[idx, 1][None, :] - ys[:, None].astype(f32)
        ib = np.broadcast_to(i32[idx][None, :], dx32.shape)
        mr32 = PD.fma32(-np.broadcast_to(s32[idx, 0][None, :], dx32.shape), dx32, PD.fma32(-np.broadcast_to(s32[idx, 1][None, :], dx32.shape), dy32, ib))
        low, high = torch.as_tensor(mr32 < ib * f32(0.25)), torch.as_tensor(mr32 > ib * f32(4))
        mi = (invd[idx_t] + m_par[idx_t, 0])[None, :]
        mr = mi - (sl[idx_t, 0] + m_par[idx_t, 1])[None, :] * dx.detach() - (sl[idx_t, 1] + m_par[idx_t, 2])[None, :] * dy.detach()
        m = torch.where(low, 0.25 * invd[idx_t][None, :], torch.where(high, 4.0 * invd[idx_t][None, :], mr))
        loss = loss + ((w * m).sum(1) * g[ys, xs]).sum()
    dxy, dcon, dop, dm = torch.autograd.grad(loss, (xy, con, op, m_par))
    dcon = dcon.numpy()
    return {"dL_dmean2D": dxy.numpy() * np.array([0.5 * W, 0.5 * H]),
            "dL_dconic": np.stack([dcon[:, 0], 0.5 * dcon[:, 1], np.zeros(len(dcon)), dcon[:, 2]], 1),
            "dL_dopacity": dop.numpy()[:, None], "dL_dplane_moments": dm.numpy()}


@pytest.mark.parametrize("name", ["n300_50x37", "n1500_opaque_48x48"])
def test_yardstick_is_autograd_of_the_dense_image(oracle, scenes, cameras, name):
    c = oracle_case(oracle, scenes, cameras, name)
    r = c["r"]
    got = autograd_dense(c)
    E = {k: B.worst(got[k], r[k]) for k in PD.OUTPUTS}
    print(f"\n{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in E.items()))
    assert max(E.values()) <= 1e-10, E
    assert all(np.abs(r[k]["signed"]).max() > 0 for k in PD.OUTPUTS)


def test_the_criterion_sees_a_dropped_suffix_term(oracle, scenes, cameras):
    c = oracle_case(oracle, scenes, cameras, "n300_50x37")
    _, eb = _e_f32(c)
    r, floor = c["r"], PD.golden()["floor"]
    acc, mom = PD.render_backward_f32(c["fr"], c["slopes"], r["g"].astype(f32), c["img32"], drop_suffix=True)
    E = PD.backward_errors(acc, mom, r)
    assert E["dL_dplane_moments"] <= 3.0 * eb["dL_dplane_moments"] + floor      # (the moments do not pass through dL/dalpha)
    for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity"):
        assert not PD.criterion(E[k], max(eb.values()), 0.0, floor) and E[k] > 100 * (3.0 * max(eb.values()) + floor), k


# ---- the closed form ----
def test_closed_form_tilted_plane(oracle, scenes, cameras):
    sc, cam, kw, th = PD.sheet(scenes, cameras)
    W, H, N = kw["image_width"], kw["image_height"], len(sc["means"])
    assert 40 <= N <= 200
    nb = oracle.render_gaussians(**kw)[2]
    view = np.asarray(kw["viewmatrix"], f32)
    tx, ty = kw["tan_fovx"], kw["tan_fovy"]
    n32, c, _ = NR.normals_f32(sc["scales"], sc["rotations"], sc["means"], view)
    sl, fb = PD.slopes_f32(n32, sc["scales"], sc["means"], view, tx, ty, W, H)
    margins = PD.branch_margins(n32, sc["scales"], sc["means"], view)
    assert not fb.any() and (c == 2).all() and margins.min() > PD.MARGIN_CAP
    invd = PD.inv_depth_of_buffers(nb)
    fr = PD.frame_of_buffers(nb, W, H, invd)
    out, Tf = PD.render_f32(fr, sl)
    centre, _ = PD.render_f32(fr, np.zeros_like(sl))
    V = view.astype(np.float64).reshape(4, 4)
    pv = sc["means"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    n0 = NR.normals_f64(sc["scales"], sc["rotations"], sc["means"], view)["n"][0]
    k0 = int(np.argmin(np.abs(sc["means"]).sum(1)))                                  # a disc next to the origin, which lies on the plane
    want = PD.plane_inverse_depth(n0, pv[k0], tx, ty, W, H)
    cover = 1.0 - Tf.astype(np.float64)
    sel = cover >= 0.5
    assert sel.sum() > 0.2 * W * H
    # no entry of a covered pixel is clamped, and none is near the clamp: the plane's depth varies by far less than a factor 4 over a disc
    rel = np.abs(out.astype(np.float64)[sel] / cover[sel] / want[sel] - 1.0)
    off = np.abs(centre.astype(np.float64)[sel] / cover[sel] / want[sel] - 1.0)
    # the margin: at the sheet's rim a pixel sees discs on one side only, about one footprint sigma away; a quarter of slope x sigma
    sigma_px = 0.2 / pv[:, 2].mean() / (2.0 * tx / W)
    slope = float(np.abs(sl.astype(np.float64)).max(0).max())
    margin = 0.25 * slope * sigma_px / np.abs(invd).max()
    print(f"\nplane: {int(sel.sum())} covered pixels, plane depth off by {rel.max() / PD.EPS32:.1f} eps32, centre depth by {off.max():.3e} "
          f"(margin {margin:.3e}), slope {slope:.3e} per pixel, footprint {sigma_px:.2f} px, branch margin {margins.min() / PD.EPS32:.0f} eps32")
    assert rel.max() <= 16 * PD.EPS32
    assert off.max() >= margin > 1000 * PD.EPS32


# ---- the branches, the clamp ----
@pytest.mark.parametrize("N", [1, 63, 257])
def test_slopes_branches_and_their_vjp(cameras, N):
    from conftest import lego_camera
    cam = lego_camera(cameras, 0, width=50, height=37)
    view = np.asarray(cam["world_to_camera"], f32)
    tx, ty, W, H = cam["tan_fovx"], cam["tan_fovy"], 50, 37
    n, s, p, special = PD.draw_gaussians(N, view)
    sl, fb = PD.slopes_f32(n, s, p, view, tx, ty, W, H)
    margins = PD.branch_margins(n, s, p, view)
    print(f"\nN = {N}: fallback {int(fb.sum())} of {N}, smallest branch margin {margins.min() / PD.EPS32:.0f} eps32")
    assert margins.min() > PD.MARGIN_CAP                                             # float32 and float64 cannot decide differently
    for row in special:
        assert fb[row] and not sl[row].any(), (row, special[row])
    assert not sl[fb].any() and (N < 9 or 0 < fb.sum() < N) and np.abs(sl[~fb]).min(initial=1.0) > 0
    fb64 = PD.steps(n, s, p, view, tx, ty, W, H, np.float64)["fallback"]
    assert np.array_equal(fb, fb64)
    sl64 = PD.slopes_f64(n, s, p, view, tx, ty, W, H, fb)
    assert np.abs(sl - sl64).max() <= 8 * PD.EPS32 * np.abs(sl64).max()
    # the slopes ARE the plane: m(p) = (n . r(p)) / (n . p_v) at any pixel, from invd at the projected centre
    V = view.astype(np.float64).reshape(4, 4)
    pv = p.astype(np.float64) @ V[:3, :3] + V[3, :3]
    x, y = PD.pixel_of(pv, tx, ty, W, H)
    for px, py in ((0.0, 0.0), (49.0, 36.0), (13.0, 29.0)):
        ray = np.array([((2 * px + 1) / W - 1) * tx, ((2 * py + 1) / H - 1) * ty, 1.0])
        k = ~fb
        want = (n[k].astype(np.float64) @ ray) / (n[k].astype(np.float64) * pv[k]).sum(1)
        got = 1.0 / pv[k, 2] + sl64[k, 0] * (px - x[k]) + sl64[k, 1] * (py - y[k])
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # (d): the header's formulas in float64 are autograd of the definition; the float32 restatement is within a few eps32 of both
    mom = np.random.default_rng(9).normal(0, 1, (N, 3)).astype(f32) * np.array([1.0, 5.0, 5.0], f32)
    dmean64, dn64, sc_mean, sc_n = PD.slopes_vjp_f64(n, s, p, view, tx, ty, W, H, fb, mom)
    hm, hn = PD.slopes_backward(n, s, p, view, tx, ty, W, H, mom, np.float64, fallback=fb)
    assert PD.rows_error(hm, dmean64, sc_mean) <= 1e-10 and PD.rows_error(hn, dn64, sc_n) <= 1e-10
    rm, rn = PD.slopes_backward(n, s, p, view, tx, ty, W, H, mom)
    E = (PD.rows_error(rm, dmean64, sc_mean), PD.rows_error(rn, dn64, sc_n))
    print(f"N = {N}: (d) restatement error {E[0]:.3e} (means), {E[1]:.3e} (normals)")
    assert max(E) <= 32 * PD.EPS32
    assert not rn[fb].any() and (N < 9 or np.abs(rm[3]).max() == 0)                   # behind the camera: invd = 0, no gradient at all
    if N > 8:
        assert np.abs(rm[4]).max() > 0 and np.abs(rm[1]).max() > 0                    # inside the near plane, zero normal: the centre depth's


def _steep_frame(W=16, H=16):
    """One 16x16 tile with one large, near Gaussian whose plane is steep: m falls through invd / 4 inside the tile."""
    nb = {"points_xy_image": np.array([[7.3, 8.1]], f32), "conic_opacity": np.array([[2e-2, 3e-3, 1.5e-2, 0.7]], f32),
          "depths": np.array([0.5], f32), "point_list": np.zeros(1, np.int32), "ranges": np.array([[0, 1]], np.int32),
          "n_contrib": np.ones((H, W), np.int32)}
    return nb, np.array([[0.4, -0.03]], f32)


def test_the_clamp_on_a_large_near_steep_gaussian():
    W = H = 16
    nb, sl = _steep_frame()
    invd = PD.inv_depth_of_buffers(nb)
    fr = PD.frame_of_buffers(nb, W, H, invd)
    g = PD.draw_g(H, W)
    r = PD.yardstick(nb, W, H, invd, sl, g)
    print(f"\nsteep: {r['clamped']} of {W * H} pixels clamped, clamp margin {r['clamp_margin'] / PD.EPS32:.0f} eps32, masked {int(r['mask'].sum())}")
    assert not r["mask"].any() and r["clamp_margin"] > PD.MARGIN_CAP and 30 < r["clamped"] < W * H - 30
    out, Tf = PD.render_f32(fr, sl)
    w = FR.weights_f32(nb, W, H, 0, *(a.ravel() for a in np.meshgrid(np.arange(W), np.arange(H)))).reshape(H, W)
    ratio = out.astype(np.float64) / w / float(invd[0])
    assert ratio.min() == 0.25 and 1.0 < ratio.max() < 4.0 and (ratio == 0.25).sum() == r["clamped"]      # held at invd / 4, exactly
    assert PD.image_error(out, r, invd) <= 4 * PD.EPS32
    acc, mom = PD.render_backward_f32(fr, sl, g, out)
    E = PD.backward_errors(acc, mom, r)
    assert max(E.values()) <= 16 * PD.EPS32, E
    # a clamped pixel contributes through its weight only: the moments are the free pixels' alone
    free = ratio > 0.25
    assert abs(float(mom[0, 0]) - float((w * g)[free].astype(np.float64).sum())) <= 8 * PD.EPS32 * float(np.abs(w * g).sum())
