"""
The yardstick of the Gaussians' normals, their image and the consistency term (tests/normal_render_reference.py) and the float32
restatement of include/gsr_normal_render.h, checked on the CPU oracle's buffers.  No GPU.

  1. the yardstick equals torch float64 autograd of a dense restatement (image = weights @ normals per tile, the gradient passing the
     0.99 cap as the kernels have it) to 1e-10 of each output's scale, the figure the distortion yardstick is held to; the header's
     (b) in float64 equals autograd of (a);
  2. the restatement against the yardstick on features_reference.SCENES plus toy, one_gaussian_40x40 and behind_n300: its errors
     are on file as E_f32 in tests/golden/normal_render_margins.json, which the GPU test's bounds use;
  3. closed forms: a flat disc facing the camera, the same disc from behind, a sheet of equal discs tilted by 30 degrees, equal
     scales, a zero quaternion;
  4. the consistency sums and gradients equal normals_reference's yardstick of the normal-prior loss with the rendered image as the
     target, on a frame where no counted pixel is within the length mask;
  5. caps, as conditions: at most FR.MAX_MASKED of the pixels masked and at most 1 % of the Gaussians undecided on every frame.
"""
import numpy as np
import pytest
import torch

import blend_grad_reference as B
import frame_walk_reference as FWR
import features_reference as FR
import normal_render_reference as NR
import normals_reference as NDR

_CASES = {}
MAX_UNDECIDED = 0.01


def oracle_case(oracle, scenes, cameras, name):
    """{buf (the oracle's forward, background 0), W, H, G, normals (float32, the restatement's), r (the yardstick)}, once per session."""
    if name not in _CASES:
        sc, cam, kw = NR.case(scenes, cameras, name)
        H, W = kw["image_height"], kw["image_width"]
        buf = oracle.render_gaussians(**kw)[2]
        view = np.asarray(kw["viewmatrix"], np.float32)
        n32, c, sigma = NR.normals_f32(sc["scales"], sc["rotations"], sc["means"], view)
        G = NR.draw_G(H, W)
        _CASES[name] = dict(sc=sc, cam=cam, kw=kw, buf=buf, W=W, H=H, G=G, view=view, normals=n32, r=NR.yardstick(buf, W, H, n32, G))
    return _CASES[name]


def autograd_dense(c):
    """{output: (N, width) float64} by torch autograd of sum_p G[p] . (w(p) @ normals), in the kernel's units."""
    buf, W, H, r = c["buf"], c["W"], c["H"], c["r"]
    xy0, co0, pl, rg = FWR.arrays(buf)
    xy = torch.tensor(xy0, requires_grad=True)
    con = torch.tensor(co0[:, :3].copy(), requires_grad=True)
    op = torch.tensor(co0[:, 3].copy(), requires_grad=True)
    n = torch.tensor(c["normals"].astype(np.float64), requires_grad=True)
    G = torch.as_tensor(r["G"])
    tiles = []
    B.blend_grads_f64(xy0, co0[:, :3], co0[:, 3], np.ones((len(xy0), 3)), np.zeros(len(xy0)), pl, rg, np.zeros(3), W, H, np.ones((H, W, 3)),
                      on_tile=lambda tile, xs, ys, idx, active, terms, masked: tiles.append((xs, ys, idx, active)))
    loss = torch.zeros((), dtype=torch.float64)
    for xs, ys, idx, active in tiles:
        idx_t, act = torch.as_tensor(idx), torch.as_tensor(active)
        dx = xy[idx_t, 0][None, :] - torch.as_tensor(xs, dtype=torch.float64)[:, None]
        dy = xy[idx_t, 1][None, :] - torch.as_tensor(ys, dtype=torch.float64)[:, None]
        A, Bc, C = con[idx_t, 0][None, :], con[idx_t, 1][None, :], con[idx_t, 2][None, :]
        a_raw = op[idx_t][None, :] * torch.exp(-0.5 * (A * dx * dx + C * dy * dy) - Bc * dx * dy)
        alpha = a_raw + (torch.clamp(a_raw, max=0.99) - a_raw).detach()
        om = torch.where(act, 1.0 - alpha, torch.ones_like(alpha))
        T = torch.cumprod(torch.cat([torch.ones(len(xs), 1, dtype=torch.float64), om[:, :-1]], 1), 1)
        w = torch.where(act, alpha * T, torch.zeros_like(alpha))
        loss = loss + ((w @ n[idx_t]) * G[ys, xs]).sum()
    dxy, dcon, dop, dn = torch.autograd.grad(loss, (xy, con, op, n))
    dcon = dcon.numpy()
    return {"dL_dmean2D": dxy.numpy() * np.array([0.5 * W, 0.5 * H]),
            "dL_dconic": np.stack([dcon[:, 0], 0.5 * dcon[:, 1], np.zeros(len(dcon)), dcon[:, 2]], 1),
            "dL_dopacity": dop.numpy()[:, None], "dL_dnormals": dn.numpy()}


@pytest.mark.parametrize("name", ["n300_50x37", "n1500_opaque_48x48"])
def test_yardstick_is_autograd_of_the_dense_image(oracle, scenes, cameras, name):
    c = oracle_case(oracle, scenes, cameras, name)
    r = c["r"]
    assert r["mask"].sum() <= FR.MAX_MASKED * r["mask"].size
    got = autograd_dense(c)
    E = {k: B.worst(got[k], r[k]) for k in NR.OUTPUTS}
    print(f"\n{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in E.items()))
    assert max(E.values()) <= 1e-10, E
    assert all(np.abs(r[k]["signed"]).max() > 0 for k in NR.OUTPUTS)


def _header_b_f64(s, q, p, view, g):
    """The header's (b) in float64 numpy, term by term."""
    c = NR.axis_index(s)
    q, p, g = q.astype(np.float64), p.astype(np.float64), g.astype(np.float64)
    V = view.astype(np.float64).reshape(4, 4)
    v = np.eye(3)[c]
    x, w = q[:, :3], q[:, 3]
    cs = 2 * w * w - 1
    cr = np.cross(x, v)
    a = v * cs[:, None] + 2 * w[:, None] * cr + 2 * x * (x * v).sum(1, keepdims=True)
    l2 = (a * a).sum(1)
    ok = (l2 >= 1e-24) & (q != 0).any(1)
    s_ = np.sqrt(np.where(ok, l2, 1.0))
    ah = a / s_[:, None]
    nc, pv = ah @ V[:3, :3], p @ V[:3, :3] + V[3, :3]
    sigma = np.where((nc * pv).sum(1) > 0, -1.0, 1.0)
    gw = (sigma[:, None] * g) @ V[:3, :3].T
    ga = (gw - ah * (ah * gw).sum(1, keepdims=True)) / s_[:, None]
    k = (x * ga).sum(1)
    ar = np.arange(len(c))
    dq = 2 * w[:, None] * np.cross(v, ga) + 2 * x[ar, c][:, None] * ga + 2 * k[:, None] * v
    dw = 4 * w * ga[ar, c] + 2 * (ga * cr).sum(1)
    return np.where(ok[:, None], np.concatenate([dq, dw[:, None]], 1), 0.0)


@pytest.mark.parametrize("N", [1, 63, 257])
def test_gaussian_normals_and_their_vjp(cameras, N):
    from conftest import lego_camera
    view = np.asarray(lego_camera(cameras, 0, width=50, height=37)["world_to_camera"], np.float32)
    s, q, p = NR.draw_gaussians(N)
    g = np.random.default_rng(9).normal(0, 1, (N, 3)).astype(np.float32)
    dq64, scale, r = NR.vjp_f64(s, q, p, view, g)
    keep = ~r["undecided"]
    assert r["undecided"].mean() <= MAX_UNDECIDED
    E = NR.rows_error(_header_b_f64(s, q, p, view, g), dq64, scale, keep)
    assert E <= 1e-10, E                                                  # the header's formula IS the derivative
    n32, c, sigma = NR.normals_f32(s, q, p, view)
    assert np.array_equal(c, r["c"]) and np.array_equal(sigma[keep & r["ok"]], r["sigma"][keep & r["ok"]])
    assert np.abs(n32[keep] - r["n"][keep]).max() <= 16 * NR.EPS32
    unit = np.linalg.norm(r["n"][r["ok"]], axis=1)
    assert np.abs(unit - 1).max() <= 1e-6                                 # (V[:3,:3] is a float32 rotation: unit to its rounding)
    pv = p.astype(np.float64) @ view.astype(np.float64)[:3, :3] + view.astype(np.float64)[3, :3]
    assert ((r["n"] * pv).sum(1)[r["ok"]] <= 0).all()                     # facing the camera
    E32 = NR.rows_error(NR.normals_backward_f32(s, q, p, view, g), dq64, scale, keep)
    print(f"\nN = {N}: (b) restatement error {E32:.3e}")
    assert 0 <= E32 <= 32 * NR.EPS32
    if N > 4:
        assert not r["ok"][4] and not n32[4].any() and not NR.normals_backward_f32(s, q, p, view, g)[4].any()   # zero quaternion: 0 and gradient 0
        tie = np.arange(N)[2::7]
        assert (c[tie] == 0).all()                                        # equal scales: c* = 0


def _e_f32(c):
    if "E_f32" not in c:
        buf, W, H, r = c["buf"], c["W"], c["H"], c["r"]
        img = NR.render_f32(buf, W, H, c["normals"])
        acc, dn = NR.render_backward_f32(buf, W, H, c["normals"], r["G"].astype(np.float32), img)
        assert not acc[:, list(NR.UNTOUCHED)].any()
        c["img32"] = img
        c["E_f32"] = (NR.image_error(img, r), NR.backward_errors(acc, dn, r))
    return c["E_f32"]


def test_restatement_errors_are_the_ones_on_file(oracle, scenes, cameras):
    gold = NR.golden()
    floor_seen = []
    for name in NR.CPU_FRAMES:
        c = oracle_case(oracle, scenes, cameras, name)
        r = c["r"]
        assert r["mask"].sum() <= FR.MAX_MASKED * r["mask"].size, name
        ef, eb = _e_f32(c)
        print(f"\n{name}: image {ef:.3e}; " + ", ".join(f"{k} {v:.3e}" for k, v in eb.items()))
        rec = gold["E_f32"][name]
        D = int(np.asarray(c["buf"]["point_list"]).size)
        if name == "behind_n300":
            assert D == 0 and ef == 0 and not any(eb.values()) and not c["img32"].any()
            continue
        assert ef <= 8 * NR.EPS32                                         # a sum of weights <= 1 times unit vectors
        for k, v in eb.items():
            # (the libm's expf may differ from the recorded one; a tenth of eps32 of slack for the frames whose errors are below eps32)
            assert np.isfinite(v) and 0.5 * rec[k] - 0.1 * NR.EPS32 <= v <= 2.0 * rec[k] + 0.1 * NR.EPS32, (name, k, v, rec[k])
        assert NR.criterion(max(eb.values()), max(eb.values()), 0.0, gold["floor"])
        floor_seen.append(max(eb.values()))
    assert 0.5 * min(floor_seen) <= gold["floor"] <= 2.0 * min(floor_seen)


def test_the_criterion_sees_a_dropped_suffix_term(oracle, scenes, cameras):
    c = oracle_case(oracle, scenes, cameras, "n300_50x37")
    _, eb = _e_f32(c)
    r, floor = c["r"], NR.golden()["floor"]
    acc, dn = NR.render_backward_f32(c["buf"], c["W"], c["H"], c["normals"], r["G"].astype(np.float32), c["img32"], drop_suffix=True)
    E = NR.backward_errors(acc, dn, r)
    assert E["dL_dnormals"] <= 3.0 * eb["dL_dnormals"] + floor             # (dL/dn does not pass through dL/dalpha)
    for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity"):
        assert not NR.criterion(E[k], max(eb.values()), 0.0, floor) and E[k] > 100 * (3.0 * max(eb.values()) + floor), k


@pytest.mark.parametrize("name", NR.CPU_FRAMES)
def test_caps_on_masked_pixels_and_undecided_gaussians(oracle, scenes, cameras, name):
    c = oracle_case(oracle, scenes, cameras, name)
    sc = c["sc"]
    r = NR.normals_f64(sc["scales"], sc["rotations"], sc["means"], c["view"])
    assert c["r"]["mask"].mean() <= FR.MAX_MASKED
    if name in ("toy", "one_gaussian_40x40"):
        # hand-placed frames of 3 and 1 Gaussians, where one Gaussian is a third of the frame or all of it and a share means nothing:
        # toy's middle Gaussian sits on the optical axis with its x axis across it, n_c . p_v = 0 EXACTLY.  What is undecided there
        # must be such an exact tie, which float32 and float64 decide alike (t > 0 is false on both sides)
        n32, c32, sigma32 = NR.normals_f32(sc["scales"], sc["rotations"], sc["means"], c["view"])
        assert r["undecided"].sum() <= 1 and np.array_equal(sigma32, r["sigma"]) and np.abs(n32 - r["n"]).max() <= 4 * NR.EPS32
        return
    # a uniformly random orientation has |cos| below 1e-4 with probability 1e-4: the drawn scenes stay inside the cap without help
    assert r["undecided"].mean() <= MAX_UNDECIDED, (name, r["undecided"].mean())


def _disc_frame(view, mean, W=16, H=16):
    """One 16x16 tile with one broad disc in its list (sz smallest, identity rotation)."""
    s = np.array([[0.5, 0.5, 0.01]], np.float32)
    q = np.array([[0, 0, 0, 1]], np.float32)
    p = np.asarray(mean, np.float32).reshape(1, 3)
    buf = {"points_xy_image": np.array([[7.3, 8.1]], np.float32), "conic_opacity": np.array([[2e-2, 3e-3, 1.5e-2, 0.7]], np.float32),
           "depths": np.array([3.0], np.float32), "point_list": np.zeros(1, np.int32), "ranges": np.array([[0, 1]], np.int32),
           "n_contrib": np.ones((H, W), np.int32)}
    return s, q, p, buf


def test_closed_forms_flat_disc_front_and_back():
    front = np.eye(4, dtype=np.float32)
    back = np.diag([-1, 1, -1, 1]).astype(np.float32)                      # the camera turned by 180 degrees about y: the disc seen from behind
    for view, mean in ((front, (0, 0, 3)), (back, (0, 0, -3))):
        s, q, p, buf = _disc_frame(view, mean)
        n32, c, sigma = NR.normals_f32(s, q, p, view)
        assert c[0] == 2 and np.array_equal(n32[0], np.array([0, 0, -1], np.float32))
        assert np.array_equal(NR.normals_f64(s, q, p, view)["n"][0], [0, 0, -1])
        img = NR.render_f32(buf, 16, 16, n32)
        w = FR.weights_f32(buf, 16, 16, 0, *(a.ravel() for a in np.meshgrid(np.arange(16), np.arange(16)))).reshape(16, 16)
        assert (w > 0).all() and np.array_equal(img[..., 2], -w) and not img[..., :2].any()      # N(p) = (0, 0, -1) alpha(p), exactly


def test_closed_form_tilted_sheet(oracle, scenes, cameras):
    """A 24 x 24 sheet of equal flat discs on a plane tilted by 30 degrees about x.  Every Gaussian has the plane's normal, so the
    blended image is A(p) n0 and N / |N| is n0 at every counted pixel; the consistency term against the depth normals is then those
    normals' own error against the plane, which the sheet's finite disc spacing leaves them with."""
    from conftest import lego_camera, render_kwargs
    W = H = 48
    cam = cameras.toy_camera(image_width=W, image_height=H)
    th = np.deg2rad(30.0)
    u, v = np.meshgrid(np.linspace(-1.6, 1.6, 24), np.linspace(-1.6, 1.6, 24))
    pts = np.stack([u.ravel(), v.ravel() * np.cos(th), v.ravel() * np.sin(th)], 1).astype(np.float32)
    N = len(pts)
    sc = scenes.synthetic_scene(N, 0.05, 0.6, 1)
    sc["means"] = pts
    sc["scales"][:] = np.array([0.12, 0.12, 0.004], np.float32)
    sc["rotations"][:] = np.array([np.sin(th / 2), 0, 0, np.cos(th / 2)], np.float32)      # (x, y, z, w): 30 degrees about x
    sc["opacities"][:] = 0.9
    kw = render_kwargs(sc, cam, width=W, height=H)
    image, depth, buf = oracle.render_gaussians(**kw)
    view = np.asarray(kw["viewmatrix"], np.float32)
    n32, c, sigma = NR.normals_f32(sc["scales"], sc["rotations"], sc["means"], view)
    assert (c == 2).all() and np.abs(n32 - n32[0]).max() <= 4 * NR.EPS32
    n0 = NR.normals_f64(sc["scales"], sc["rotations"], sc["means"], view)["n"][0]
    world = np.array([0, -np.sin(th), np.cos(th)])                                         # R_x(30) e_z
    assert np.abs(np.abs(n0 @ np.linalg.inv(view.astype(np.float64)[:3, :3])) - np.abs(world)).max() <= 1e-6 and n0[2] < 0
    img = NR.render_f32(buf, W, H, n32)
    ncam = NDR.camera(W, H, cam["tan_fovx"], cam["tan_fovy"])
    dec = NDR.decide(np.asarray(depth, np.float32).reshape(H, W), np.asarray(buf["final_Ts"], np.float32).reshape(H, W), ncam)
    nd = np.nan_to_num(NDR.normals_from_z(dec["z"].astype(np.float64), ncam))
    r = NR.consistency_f64(img, nd, dec["valid"], None, 1.0, W, H)
    assert r["counted"].sum() > 0.3 * W * H and not (r["near"] & r["counted"]).any()
    assert np.abs(r["th"][r["counted"]] - n0).max() <= 8 * NR.EPS32                        # t^ = the plane normal at every counted pixel
    own = (1.0 - nd[r["counted"]] @ n0).sum()                                              # the depth normals' own error on the sheet
    print(f"\nsheet: {int(r['counted'].sum())} counted pixels, consistency sum {r['sums'][0]:.4e}, depth normals' own error {own:.4e}")
    assert r["sums"][0] <= own * (1 + 1e-5) + 1e-9
    assert r["sums"][0] / r["sums"][1] < 0.05                                              # ... and they do see the tilt: within 18 degrees in the mean


def test_consistency_equals_the_prior_loss_with_the_image_as_target(oracle, scenes, cameras):
    """normals_reference's yardstick of the normal-prior loss, target = the rendered normal image (any length, normalised there):
    the same sums and the same gD, gA come out of the consistency term's n_d gradient sent through the depth normals' VJP."""
    c = oracle_case(oracle, scenes, cameras, "n1500_opaque_48x48")
    W, H, kw = c["W"], c["H"], c["kw"]
    image, depth, buf = oracle.render_gaussians(**kw)
    _e_f32(c)
    img = c["img32"]
    ncam = NDR.camera(W, H, kw["tan_fovx"], kw["tan_fovy"])
    Dinv, T = np.asarray(depth, np.float32).reshape(H, W), np.asarray(buf["final_Ts"], np.float32).reshape(H, W)
    dec = NDR.decide(Dinv, T, ncam)
    weight32 = float(np.float32(0.05 / (W * H)))
    weight = weight32 * W * H
    case = {"name": "consistency", "W": W, "H": H, "cam": ncam, "Dinv": Dinv, "final_T": T, "target": img, "R": None, "mask": None,
            "weight": weight, "weight32": weight32, "dec": dec}
    ref = NDR.reference(case)
    nd = ref["normals"]                                                                    # float64 depth normals, 0 where not valid
    r = NR.consistency_f64(img, nd, dec["valid"], None, weight, W, H)
    assert r["counted"].sum() > 50 and not (r["near"] & dec["valid"]).any()                # no counted pixel within the length mask
    assert (np.linalg.norm(img.astype(np.float64), axis=2)[dec["valid"]] >= 1e-3 + NR.LENGTH_NEAR).all()
    assert abs(ref["sums"][0] - r["sums"][0]) <= 1e-9 * max(1.0, abs(r["sums"][0])) and ref["sums"][1] == r["sums"][1]
    gD, gA = NDR.closed_form_vjp(case, r["gnd"])
    for got, want in ((gD, ref["gD"]), (gA, ref["gA"])):
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    s32, gN32, gnd32, counted32 = NR.consistency_f32(img, nd.astype(np.float32), dec["valid"], None, weight, W, H)
    assert np.array_equal(counted32, r["counted"])
    assert abs(float(s32[0]) - r["sums"][0]) <= 4 * NR.EPS32 * r["sums"][1] and float(s32[1]) == r["sums"][1]
    assert np.abs(gN32 - r["gN"]).max() <= 16 * NR.EPS32 * np.abs(r["gN"]).max() / 1e-3 * 1e-3 + 1e-12
    assert np.abs(gnd32 - r["gnd"]).max() <= 8 * NR.EPS32 * np.abs(r["gnd"]).max()
