"""
The float32 restatement and the float64 yardstick of the plane depth under the median rule (tests/plane_median_reference.py), from
the references alone, on the CPU.

  1. invariants on median_depth_reference.CASES, all nine: the restatement's contributor is median_f64's outside the tie mask (it does
     not depend on the slopes); at zero slopes its value is the centre median's bit for bit; a clamped chosen entry gives zero addends,
     an unclamped one (g, g (-dx), g (-dy)); every case keeps at least 2 clamped and 10 unclamped chosen entries with slopes.
  2. the closed form: on plane_depth_reference.sheet() (144 equal discs on one plane tilted by 45 degrees, 48x48) the value at every
     pixel with a contributor and an unclamped entry is the plane's analytic inverse depth, whichever disc the median chose.  The
     restatement's worst relative error is on file in tests/golden/plane_median_margins.json ("closed_form_rel"); 4x that is allowed,
     and the centre median of the same frame is off by at least 100x the plane median's error.
  3. the chain: the moments fed through plane_depth_reference.slopes_vjp_f64 are float64 torch autograd of
     sum_p g[p] (n . r(p)) / (n . mu_c(p)), c held fixed, on a 24-Gaussian case with every fallback branch and the clamp in it, to
     1e-10 of each row's scale -- the criterion test_plane_depth_reference.py holds the header's (d) to.
"""
import json

import numpy as np
import pytest
import torch

import median_depth_reference as M
import normal_render_reference as NR
import plane_depth_reference as PD
import plane_median_reference as PM

f32 = np.float32


@pytest.mark.parametrize("name", list(M.CASES))
def test_restatement_invariants(name):
    c = PM.case(name)                                    # (asserts the clamped / unclamped counts)
    fr, ref = c["fr"], c["ref"]
    keep = ~ref["tie"]
    assert ref["tie"].mean() <= M.MAX_TIES
    assert np.array_equal(c["contrib"][keep], ref["contrib"][keep])
    print("\nPLANE_MEDIAN_CHOSEN " + json.dumps({"case": name, **c["counts"], "tie_share": float(ref["tie"].mean())}))
    ties = int(ref["tie"].sum())                          # (another libm's exp may move the choice at a pixel inside the tie mask, and only there)
    assert all(abs(PM.golden()["chosen"][name][k] - v) <= ties for k, v in c["counts"].items()), (c["counts"], ties)
    # zero slopes: the centre median, bit for bit, and nothing is clamped
    med0, contrib0, clamped0 = PM.forward_f32(fr, np.zeros_like(c["slopes"]))
    assert np.array_equal(contrib0, c["contrib"]) and not clamped0.any()
    assert med0[keep].tobytes() == ref["med"][keep].tobytes()
    sel = contrib0 > 0
    assert med0[sel].tobytes() == fr["invd"][c["ch"]["ids"][sel]].tobytes() and not med0[~sel].view(np.uint32).any()
    # the two routes to m agree bit for bit: the walk's, and chosen() at the walk's contributors
    assert c["ch"]["m"].tobytes() == c["med"].tobytes() and np.array_equal(c["ch"]["clamped"], c["clamped"])
    assert (c["med"][sel] >= fr["invd"][c["ch"]["ids"][sel]] * f32(0.25)).all() and (c["med"][sel] <= fr["invd"][c["ch"]["ids"][sel]] * f32(4)).all()
    # the addends
    g = M.draw_g(fr["H"], fr["W"])
    ids, v = PM.addends_f32(fr, c["slopes"], g, c["contrib"], c["ch"])
    assert not v[c["clamped"] | ~sel].any()
    free = sel & ~c["clamped"]
    assert v[free][:, 0].tobytes() == g[free].tobytes()
    assert np.array_equal(v[free][:, 1], g[free] * (-c["ch"]["dx"][free])) and np.array_equal(v[free][:, 2], g[free] * (-c["ch"]["dy"][free]))
    r = PM.moments_f64(fr, c["slopes"], g, c["contrib"], c["ch"])
    assert int(r["count"].sum()) == int(free.sum()) and not r["abs"][r["count"] == 0].any()
    # the float32 addends summed in float64 lie within the header's bound of the yardstick (its first two terms: dx and the product)
    s32 = np.zeros((fr["N"], 3))
    np.add.at(s32, ids[free], v[free].astype(np.float64))
    assert PM.bound_ratio(s32, r) <= 1.0
    # stale contributors are clipped, never followed out of the list
    wild = np.where(np.random.default_rng(1).random(g.shape) < 0.5, 1 << 30, -5)
    w = PM.chosen(fr, c["slopes"], wild)
    assert (w["c"] <= 640).all() and (w["c"] >= 0).all() and (w["ids"] < fr["N"]).all()


def test_closed_form_tilted_plane(oracle, scenes, cameras):
    sc, cam, kw, th = PD.sheet(scenes, cameras)
    W, H = kw["image_width"], kw["image_height"]
    nb = oracle.render_gaussians(**kw)[2]
    view = np.asarray(kw["viewmatrix"], f32)
    tx, ty = kw["tan_fovx"], kw["tan_fovy"]
    n32, axis, _ = NR.normals_f32(sc["scales"], sc["rotations"], sc["means"], view)
    sl, fb = PD.slopes_f32(n32, sc["scales"], sc["means"], view, tx, ty, W, H)
    assert not fb.any() and (axis == 2).all() and len(sc["means"]) == 144
    invd = PD.inv_depth_of_buffers(nb)
    fr = PD.frame_of_buffers(nb, W, H, invd)
    med, contrib, clamped = PM.forward_f32(fr, sl)
    centre, contrib0, _ = PM.forward_f32(fr, np.zeros_like(sl))
    assert np.array_equal(contrib, contrib0)
    V = view.astype(np.float64).reshape(4, 4)
    pv = sc["means"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    n0 = NR.normals_f64(sc["scales"], sc["rotations"], sc["means"], view)["n"][0]
    k0 = int(np.argmin(np.abs(sc["means"]).sum(1)))                                  # a disc next to the origin, which lies on the plane
    want = PD.plane_inverse_depth(n0, pv[k0], tx, ty, W, H)
    sel = (contrib > 0) & ~clamped
    assert sel.sum() > 0.4 * W * H
    rel = np.abs(med.astype(np.float64)[sel] / want[sel] - 1.0)
    off = np.abs(centre.astype(np.float64)[sel] / want[sel] - 1.0)
    rec = PM.golden()["closed_form_rel"]
    print("\nPLANE_MEDIAN_CLOSED_FORM " + json.dumps({"pixels": int(sel.sum()), "clamped": int(clamped.sum()), "rel": float(rel.max()),
                                                      "rel_eps32": float(rel.max() / PD.EPS32), "recorded": rec, "centre_off": float(off.max())}))
    assert rel.max() <= 4.0 * rec, (rel.max(), rec)
    assert off.max() >= 100.0 * rel.max(), (off.max(), rel.max())


def test_moments_chain_is_autograd_of_the_plane_of_the_chosen_gaussian(cameras):
    from conftest import lego_camera
    N, W, H = 24, 50, 37
    cam = lego_camera(cameras, 0, width=W, height=H)
    view = np.asarray(cam["world_to_camera"], f32)
    tx, ty = cam["tan_fovx"], cam["tan_fovy"]
    n, s, p, special = PD.draw_gaussians(N, view)
    assert PD.branch_margins(n, s, p, view).min() > PD.MARGIN_CAP
    sl, fb = PD.slopes_f32(n, s, p, view, tx, ty, W, H)
    assert 5 <= fb.sum() <= N - 10 and set(special.values()) == {"zero", "behind", "near", "grazing", "round"}
    Vm = view.astype(np.float64).reshape(4, 4)
    pv = p.astype(np.float64) @ Vm[:3, :3] + Vm[3, :3]
    front = pv[:, 2] > 0
    z = np.where(front, pv[:, 2], 1.0)
    x, y = PD.pixel_of(np.stack([pv[:, 0], pv[:, 1], z], 1), tx, ty, W, H)
    rng = np.random.default_rng(8)
    # one tile list per tile holding all 24 Gaussians; every pixel chooses one of them at random: the contributor image is an input
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    fr = dict(W=W, H=H, N=N, D=tiles * N, xy=np.stack([x, y], 1), invd=np.where(front, 1.0 / z, 0.0).astype(f32),
              point_list=np.tile(np.arange(N, dtype=np.int32), tiles), ranges=np.stack([np.arange(tiles) * N, np.arange(1, tiles + 1) * N], 1).astype(np.int32))
    contrib = rng.integers(0, N + 1, (H, W))
    g = rng.normal(0, 1, (H, W))
    ch = PM.chosen(fr, sl, contrib)
    assert np.array_equal(ch["ids"], contrib - 1)
    live = (ch["ids"] >= 0) & ~ch["clamped"]
    assert ch["clamped"].sum() >= 20 and (live & ~fb[np.maximum(ch["ids"], 0)]).sum() >= 500 and (live & fb[np.maximum(ch["ids"], 0)]).sum() >= 100
    r = PM.moments_f64(fr, sl, g, contrib, ch)
    dmean, dn, sc_mean, sc_n = PD.slopes_vjp_f64(n, s, p, view, tx, ty, W, H, fb, r["signed"])
    # autograd of the definition: the plane of the chosen Gaussian at the pixel's ray; its centre depth on the fallback branch
    nt = torch.tensor(n.astype(np.float64), requires_grad=True)
    pt = torch.tensor(p.astype(np.float64), requires_grad=True)
    V = torch.tensor(Vm)
    pvt = pt @ V[:3, :3] + V[3, :3]
    ft = torch.as_tensor(front)
    zt = torch.where(ft, pvt[:, 2], torch.ones_like(pvt[:, 2]))
    invd_t = torch.where(ft, 1.0 / zt, torch.zeros_like(zt))
    ys, xs = np.nonzero(live)
    ids = torch.as_tensor(ch["ids"][live])
    ray = torch.tensor(np.stack([((2.0 * xs + 1.0) / W - 1.0) * tx, ((2.0 * ys + 1.0) / H - 1.0) * ty, np.ones(len(xs))], 1))
    fbt = torch.as_tensor(fb)
    t = torch.where(fbt, torch.ones_like(zt), (nt * pvt).sum(1))
    plane = (nt[ids] * ray).sum(1) / t[ids]
    m = torch.where(fbt[ids], invd_t[ids], plane)
    L = (torch.as_tensor(g[live]) * m).sum()
    an, ap = torch.autograd.grad(L, (nt, pt))
    E = (PD.rows_error(dmean, ap.numpy(), sc_mean), PD.rows_error(dn, an.numpy(), sc_n))
    print(f"\nPLANE_MEDIAN_CHAIN means {E[0]:.3e}, normals {E[1]:.3e}; clamped {int(ch['clamped'].sum())}, live {int(live.sum())}")
    assert max(E) <= 1e-10, E
    assert np.abs(ap.numpy()).max() > 0 and np.abs(an.numpy()).max() > 0
    # the value side: sum_p g m over the unclamped entries is invd S0 + gx Sx + gy Sy per Gaussian, the header's M of (d)
    sl64 = PD.slopes_f64(n, s, p, view, tx, ty, W, H, fb)
    S = r["signed"]
    value = (invd_t.detach().numpy() * S[:, 0] + sl64[:, 0] * S[:, 1] + sl64[:, 1] * S[:, 2]).sum()
    assert abs(value - float(L.detach())) <= 1e-10 * float((np.abs(g[live]) * np.abs(m.detach().numpy())).sum())
