"""
The CPU oracle against an independent float64 statement of the reference (tests/f64_reference.py).  No GPU.

Every GPU parity test compares the kernels with the oracle, and the oracle and the kernels share an expression order by
design, so a misreading of the reference common to both passes those tests.  Here the oracle meets float64 arithmetic
written from the mathematics (autograd for every backward step that is a derivative, a closed form for the one that is
not) with each of the reference backward's departures from the true gradient an explicit switch.

Criteria (float64 is the reference in every one):
  * image / inverse depth / final_T: parity.assert_image; n_contrib: parity.assert_counts;
  * radii and tile rectangles exact, except where the float64 value that ceil() / int() rounds lies within NEAR_INT of
    an integer (or a culling test within NEAR_INT of its threshold): those are counted and bounded by NEAR_MAX;
  * per-Gaussian floats: the float32 error model of FWD_TOL (below, with the measured worst case);
  * all eight gradient arrays: parity.assert_grad, and dL_dcov3D all zero;
  * and, sharper, stage by stage: the float64 geometry backward fed with the ORACLE's blend-stage gradients must meet the
    oracle's dL_dmean3D / dL_dshs / local dL_dcov3D, and the float64 cov3d step fed with the oracle's local dL_dcov3D its
    dL_dscale / dL_drot, per Gaussian, within GEOM_REL.  This isolates the per-Gaussian geometry (straight-line float32
    code) from the blend's long sums, so a convention error worth 1e-5 of one Gaussian's gradient is still visible.
"""
import time

import numpy as np
import pytest
import torch

from conftest import render_kwargs, backward_kwargs
import f64_reference as F
import parity

# ---- error models (float32 vs float64, per Gaussian).  The worst case measured on the case matrix and the two large GPU cases
# is in brackets, as a fraction of the limit (oracle; kernel where it differs); the limits sit 2.5x to 30x above it.
#   xy       |d| <= 2e-6 * (ndc_scale + 1) * size / 2, ndc_scale = |p_w| (|[p,1]| |P cols 0,1| + |ndc| |[p,1]| |P col 3|),
#            the first-order bound of p_hom.xy / (p_hom.w + 1e-7)            [0.045]
#   depth    |d| <= 1e-6 * (|depth| + |[p,1]| |V col 2|)                    [0.072]
#   cov3D    |d| <= 2e-6 * max_k |cov3D_k|                                  [0.21]
#   conic    |d| <= 4e-6 * kappa * max_k |conic_k|, kappa = the blurred Sigma2D's condition number   [0.32; kernel 0.41]
#   colour   |d| <= 1e-6 * (1 + sum_k |basis_k * sh_k|)                     [0.19]
FWD_TOL = {"xy": 2e-6, "depth": 1e-6, "cov3D": 2e-6, "conic": 4e-6, "colour": 1e-6}
#   geometry backward, per Gaussian and array, |d|_inf <= GEOM_REL * scale_i:
#     dL_dmean3D  scale_i = max(|projection part| * w_cond^2, |cov2d part| * kappa, |SH direction part|), w_cond = the
#                 projection's 1/w conditioning (|[p,1]| |P col 3| / |w|), kappa = the blurred Sigma2D's condition number
#                                                                              [measured worst 0.03 of the limit]
#     dL_dshs     scale_i = max |dL_dcolor_i|                                  [0.13]
#     dL_dcov3D   scale_i = |T|^2 (a + |b| + c)^2 |dL_dconic_i|_1 / det^2, the magnitude the cov2d step sums before its
#                 cancellations                                                [1.9e-6 of it: 0.37 of the limit, a
#                 frustum-clamped 317 px splat]
#     dL_dcov3D_small  for splats below the blur (det < SMALL_DET) the step is well conditioned: scale_i = kappa *
#                 max |dL_dcov3D_i|; measured worst 3.1e-7 of it, limit 1e-6.  This is what makes denom_eps (the 1e-7 in
#                 1/(det^2 + 1e-7), 1.2e-5 of such a splat's row) visible.
#     dL_dscale / dL_drot  scale_i = max|scale_i| (squared for dL_drot) * max|dL_dcov3D_i| [0.19]
GEOM_REL = {"dL_dmean3D": 1e-5, "dL_dshs": 2e-6, "dL_dcov3D": 5e-6, "dL_dcov3D_small": 1e-6, "dL_dscale": 1e-5,
            "dL_drot": 1e-5}
SMALL_DET = 0.2
NEAR_INT, NEAR_MAX = 1e-5, 0.01


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def camera(cameras, R, c, W, H, fovx=0.8):
    """World-to-camera rotation R (rows: camera axes, z forward, y down), centre c -> the reference's camera dict, through
    the NeRF-synthetic path (cameras.nerf_camera) both conventions come from."""
    c2w = np.eye(4)
    c2w[:3, :3] = np.asarray(R, np.float64).T
    c2w[:3, 3] = c
    c2w[:3, 1:3] *= -1                                   # COLMAP -> Blender axes, undone by nerf_camera
    return cameras.nerf_camera(c2w, W, H, fovx)


def make_case(cameras, *, W, H, n, degree, train, bg, sm, seed, aniso=20.0, outside=0.1, behind=0.05, bright=0.0,
              opaque=0.0, faint=0.0, R=None, scale=0.04):
    """A seeded scene in front of a random camera.  Camera at 3 d looking along d, scene around 7 d: under render.py's
    convention (view = world_to_view, no translation, Q3) the depth is d.p ~ 7, under train.py's 4.  Fractions: `outside`
    with the mean beyond the 1.3 tan limit and a splat large enough to reach into the image, `behind` behind the near plane,
    `bright` with SH x 6 (clamped colours), `opaque` with opacity near 1 (alpha cap, T < 1e-4 stops), `faint` near 1/255."""
    rng = np.random.default_rng(seed)
    R = _rotation(rng) if R is None else np.asarray(R, np.float64)
    d = R[2]
    cam = camera(cameras, R, 3.0 * d, W, H)
    tx, ty = float(cam["tan_fovx"]), float(cam["tan_fovy"])
    z = rng.uniform(2.5, 6.0, n)
    u = rng.uniform(-1.1, 1.1, (n, 2))
    k_out = rng.random(n) < outside
    u[k_out] = rng.choice([-1, 1], (k_out.sum(), 2)) * rng.uniform(1.35, 1.8, (k_out.sum(), 2))
    k_beh = rng.random(n) < behind
    # behind the near plane, but not within 0.05 of the camera plane: there 1/w makes xy (and under render.py's convention,
    # whose near test is on another depth, a rendered splat) arbitrarily ill-conditioned
    zb = rng.uniform(-1.0, 0.14, k_beh.sum())
    z[k_beh] = np.where(zb < -0.05, zb, zb + 0.1)
    pc = np.stack([u[:, 0] * z * tx, u[:, 1] * z * ty, z], 1)
    means = (pc @ R + 3.0 * d).astype(np.float32)        # camera -> world: R^T p_cam + c
    s = np.exp(rng.normal(np.log(scale), 0.4, (n, 1))) * np.concatenate(
        [np.ones((n, 1)), rng.uniform(1.0 / aniso, 1.0, (n, 2))], 1)
    s[k_out] *= 12.0 / scale * 0.05                      # ~0.6 scene units: off-screen splats still reach in
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    op = rng.uniform(0.05, 0.95, (n, 1))
    k = rng.random(n)
    op[k < opaque] = rng.uniform(0.992, 1.0, ((k < opaque).sum(), 1))
    op[(k >= opaque) & (k < opaque + faint)] = rng.uniform(0.0035, 0.006, (((k >= opaque) & (k < opaque + faint)).sum(), 1))
    shs = np.concatenate([rng.normal(0, 0.5, (n, 1, 3)), rng.normal(0, 0.15, (n, 15, 3))], 1)
    shs[rng.random(n) < bright] *= 6.0
    sc = {"means": means, "scales": s.astype(np.float32), "rotations": q.astype(np.float32),
          "opacities": op.astype(np.float32), "shs": shs.astype(np.float32)}
    kw = render_kwargs(sc, cam, width=W, height=H, degree=degree, train_convention=train, bg=bg)
    kw["scale_modifier"] = float(sm)
    return sc, cam, kw


def campos_case(cameras):
    """render.py's convention with a camera whose float32 matrices are exact (a 90-degree turn about z, centre (0,0,3)):
    Gaussian 0 sits exactly at campos (the SH skip, backward.py:107), Gaussian 1 two float32 ulps in front of it (the
    dnormvdv floor, backward.py:53); both are in front of the near plane in that convention (depth d.p = 3).  The view matrix's
    translation column is non-zero there (Q3) and the rotation block is not symmetric (Q1)."""
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    sc, cam, kw = make_case(cameras, W=48, H=40, n=40, degree=3, train=False, bg=(0.1, 0.2, 0.3), sm=1.0, seed=77, R=Rz)
    c = np.asarray(cam["camera_center"], np.float32)
    assert np.array_equal(c, np.float32([0, 0, 3])), c
    sc["means"][0] = c
    sc["means"][1] = c + np.float32([0, 0, 1e-6])                       # 3 + 2 ulp
    sc["scales"][:2] = 0.3
    sc["opacities"][:2] = 0.5
    return sc, cam, kw


# (name, make_case arguments).  Together: every image shape and N of the issue, SH degree 0..3, both conventions, zero and
# non-zero background, scale_modifier 1.0 and 1.3.
CASES = [
    ("16x16_n1", dict(W=16, H=16, n=1, degree=0, train=True, bg=(0, 0, 0), sm=1.0, seed=1, outside=0, behind=0)),
    ("17x17_n2", dict(W=17, H=17, n=2, degree=1, train=False, bg=(0.2, 0.4, 0.6), sm=1.3, seed=2, outside=0, behind=0)),
    ("37x29_n63", dict(W=37, H=29, n=63, degree=2, train=True, bg=(0.5, 0.1, 0.9), sm=1.0, seed=3, bright=0.3)),
    ("64x48_n64", dict(W=64, H=48, n=64, degree=3, train=False, bg=(0, 0, 0), sm=1.3, seed=4, bright=0.5)),
    ("64x48_n65", dict(W=64, H=48, n=65, degree=3, train=True, bg=(0.3, 0.3, 0.3), sm=1.0, seed=5, opaque=0.4, faint=0.3)),
    ("37x29_n257", dict(W=37, H=29, n=257, degree=1, train=True, bg=(0, 0, 0), sm=1.3, seed=6, opaque=0.2, faint=0.2)),
    ("200x136_n700", dict(W=200, H=136, n=700, degree=3, train=False, bg=(0.1, 0.7, 0.2), sm=1.0, seed=7, bright=0.2, opaque=0.1)),
    ("200x136_n3000", dict(W=200, H=136, n=3000, degree=3, train=True, bg=(0.9, 0.8, 0.7), sm=1.3, seed=8, bright=0.1, opaque=0.1, faint=0.1)),
    ("64x48_n700_deg0", dict(W=64, H=48, n=700, degree=0, train=False, bg=(0.2, 0.2, 0.2), sm=1.3, seed=9, opaque=0.3)),
    ("tiny_splats", dict(W=64, H=48, n=300, degree=2, train=True, bg=(0, 0, 0), sm=1.0, seed=10, scale=2e-3, outside=0)),
]
CASE_NAMES = [c[0] for c in CASES] + ["campos"]


def build_case(cameras, name):
    if name == "campos":
        return campos_case(cameras)
    return make_case(cameras, **dict(CASES)[name])


def pixel_grad(H, W, seed=99):
    return np.random.default_rng(seed).normal(0.0, 1.0, (H, W, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- checks
def _near(x, tol=NEAR_INT):
    x = np.asarray(x, np.float64)
    return np.abs(x - np.round(x)) <= tol * np.maximum(1.0, np.abs(x))


def forward_margins(pre, buf):
    """Normalised per-Gaussian forward errors (<= 1 inside FWD_MODEL) and the integer checks.  Returns (margins, n_near)."""
    cam = pre["cam"]
    N = pre["N"]
    vis = (buf["radii"] > 0) & ~pre["culled"]
    # integers: radii (and with them the culling decisions) and the tile rectangles
    ambiguous = _near(pre["radius_f"]) | _near(pre["rect_f"]).any(1) | (np.abs(pre["p_view"][:, 2].detach().numpy() - 0.2) < 1e-5)
    rad_ok = (np.asarray(buf["radii"]) == pre["radii"]) | ambiguous
    assert rad_ok.all(), f"radii differ at {np.where(~rad_ok)[0][:8]}: oracle {buf['radii'][~rad_ok][:8]} f64 {pre['radii'][~rad_ok][:8]}"
    tiles = ((pre["rect"][:, 2] - pre["rect"][:, 0]) * (pre["rect"][:, 3] - pre["rect"][:, 1]))
    touched = np.diff(np.concatenate([[0], buf["point_offsets"]])) if N else np.zeros(0)
    rect_ok = (touched == np.where(pre["culled"], 0, tiles)) | ambiguous
    assert rect_ok.all(), f"tile rectangles differ at {np.where(~rect_ok)[0][:8]}"
    n_near = int((ambiguous & (buf["radii"] > 0)).sum())
    assert n_near <= max(1, NEAR_MAX * N), f"{n_near} Gaussians within {NEAR_INT} of an integer decision"
    m = {}
    if not vis.any():
        return m, n_near
    v = torch.as_tensor(vis)
    g = lambda k: pre[k].detach()[v].numpy()
    size = np.array([cam.W, cam.H], np.float64)
    m["xy"] = np.abs(buf["points_xy_image"][vis] - g("xy")) / (FWD_TOL["xy"] * (pre["ndc_scale"][vis] + 1) * size / 2)
    m["depth"] = np.abs(buf["depths"][vis] - g("depth")) / (FWD_TOL["depth"] * (np.abs(g("depth")) + pre["depth_scale"][vis]))
    c3 = g("cov3D")
    m["cov3D"] = np.abs(buf["cov3Ds"][vis] - c3) / (FWD_TOL["cov3D"] * np.abs(c3).max(1, keepdims=True))
    con = g("conic")
    kappa = pre["kappa"][vis][:, None]
    m["conic"] = np.abs(buf["conic_opacity"][vis][:, :3] - con) / (FWD_TOL["conic"] * kappa * np.abs(con).max(1, keepdims=True))
    m["colour"] = np.abs(buf["colors"][vis] - g("colour")) / (FWD_TOL["colour"] * (1 + pre["colour_scale"][vis]))
    assert np.array_equal(buf["conic_opacity"][vis][:, 3], g("opacity").astype(np.float32))
    clamp_ok = (buf["clamped_state"][vis] == pre["clamped"][vis]) | (np.abs(pre["colour_raw"][vis]) < 1e-5)
    assert clamp_ok.all(), "colour clamp decisions differ"
    return {k: float(x.max()) for k, x in m.items()}, n_near


def _rowmax(x, n):
    return np.abs(np.asarray(x, np.float64).reshape(n, -1)).max(1)


def geometry_margins(sc, kw, buf, g, switches=None):
    """Stage 2 and 3 of the backward, per Gaussian: the float64 geometry fed with the oracle's blend-stage gradients
    against the oracle's geometry outputs.  Returns the worst normalised error per array (<= 1 inside GEOM_REL)."""
    N = buf["radii"].shape[0]
    vis = buf["radii"] > 0
    m3, dshs, dcov6, parts = F.geometry_vjp_f64(sc, kw, int(kw["degree"]), vis, buf["clamped_state"], g["dL_dmean2D"],
                                                g["dL_dconic"], g["dL_dcolor"], switches, cov3D=buf["cov3Ds"])
    # the cov3d step is fed the checked side's own local dL_dcov3D where it exposes it (the oracle), else the float64 one
    local = g["_dL_dcov3D_local"] if "_dL_dcov3D_local" in g else dcov6.numpy()
    dsc, drot = F.cov3d_backward_f64(sc, kw, vis, local, switches)
    pre = F.preprocess_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    kappa, w_cond = pre["kappa"], pre["w_cond"]
    tiny = 1e-30
    out = {}
    p_proj, p_cov, p_sh = [_rowmax(p.numpy(), N) for p in parts[:3]]
    cov_scale = parts[3]["cov_scale"].numpy()
    s_m3 = np.maximum.reduce([p_proj * w_cond ** 2, p_cov * kappa, p_sh]) + tiny
    out["dL_dmean3D"] = _rowmax(g["dL_dmean3D"] - m3.numpy(), N) / (GEOM_REL["dL_dmean3D"] * s_m3)
    out["dL_dshs"] = _rowmax(g["dL_dshs"].reshape(N, -1) - dshs.numpy().reshape(N, -1), N) / (
        GEOM_REL["dL_dshs"] * (_rowmax(g["dL_dcolor"], N) + tiny))
    if "_dL_dcov3D_local" in g:
        err = _rowmax(g["_dL_dcov3D_local"] - dcov6.numpy(), N)
        out["dL_dcov3D"] = err / (GEOM_REL["dL_dcov3D"] * (cov_scale + tiny))
        small = pre["det"].detach().numpy() < SMALL_DET
        out["dL_dcov3D_small"] = np.where(small, err / (GEOM_REL["dL_dcov3D_small"] * kappa * (_rowmax(dcov6.numpy(), N) + tiny)), 0.0)
    sm = np.abs(sc["scales"]).max(1)
    dc = _rowmax(local, N) * (1.0 if "_dL_dcov3D_local" in g else kappa)    # else: the float64 local carries the cov2d error
    out["dL_dscale"] = _rowmax(g["dL_dscale"] - dsc.numpy(), N) / (GEOM_REL["dL_dscale"] * (sm * dc + tiny))
    out["dL_drot"] = _rowmax(g["dL_drot"] - drot.numpy(), N) / (GEOM_REL["dL_drot"] * (sm * sm * dc + tiny))
    return {k: float(v[vis].max()) if vis.any() else 0.0 for k, v in out.items()}


def blend_on_buffers(pre, buf):
    """The float64 blend on the checked side's own per-Gaussian floats widened to float64: their float32 rounding is what
    the per-Gaussian model bounds, and through opaque splats (1 - alpha) amplifies it, so it is not counted twice."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    with torch.no_grad():
        return [x.numpy() for x in F.blend_f64(
            t(buf["points_xy_image"]), t(buf["conic_opacity"][:, :3]), t(buf["conic_opacity"][:, 3]), t(buf["colors"]),
            t(buf["depths"]), buf["point_list"], buf["ranges"], pre["cam"].bg, pre["cam"].W, pre["cam"].H)]


_CACHE = {}


def oracle_case(oracle, cameras, name):
    """The oracle's forward and backward of one case, and the float64 forward (computed once per session)."""
    if name not in _CACHE:
        sc, cam, kw = build_case(cameras, name)
        img, dep, buf = oracle.render_gaussians(**kw)
        dpix = pixel_grad(kw["image_height"], kw["image_width"])
        g = oracle.backward(**backward_kwargs(sc, cam, kw, buf, dpix))
        pre = F.preprocess_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
        _CACHE[name] = dict(sc=sc, cam=cam, kw=kw, img=img, dep=dep, buf=buf, dpix=dpix, g=g, pre=pre, f64=blend_on_buffers(pre, buf))
    return _CACHE[name]


def check_forward(c):
    buf, (i64, d64, T64, n64) = c["buf"], c["f64"]
    rep = {"image": parity.assert_image("image", c["img"], i64),
           "inv_depth": parity.assert_image("inv_depth", c["dep"], d64, tight=2e-5, loose=5e-3, flip_cap=2.5e-2),
           "final_T": parity.assert_image("final_T", buf["final_Ts"], T64),
           "n_contrib": parity.assert_counts("n_contrib", buf["n_contrib"], n64)}
    m, n_near = forward_margins(c["pre"], buf)
    for k, v in m.items():
        assert v <= 1.0, f"{k}: error {v:.2f} x the float32 error model"
    rep.update({k + "_model": v for k, v in m.items()})
    rep["near_integer"] = n_near
    return rep


def check_backward(c, switches=None):
    """Everything the backward must meet against float64 under `switches` (None: the reference's conventions)."""
    g = c["g"]
    r = F.backward_f64(c["sc"], c["kw"], c["buf"]["point_list"], c["buf"]["ranges"], c["dpix"], switches,
                       pre=None if switches else c["pre"])
    rep = {}
    for k in parity.GRAD_KEYS:
        rep[k] = parity.assert_grad(k, g[k], r[k])
    assert not np.any(g["dL_dcov3D"]), "dL_dcov3D is returned unfilled by the reference (backward.py:1119)"
    m = geometry_margins(c["sc"], c["kw"], c["buf"], g, switches)
    for k, v in m.items():
        assert v <= 1.0, f"geometry stage {k}: error {v:.2f} x the float32 error model"
    rep.update({k + "_geom": v for k, v in m.items()})
    return rep


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_against_f64(oracle, cameras, name):
    t0 = time.time()
    c = oracle_case(oracle, cameras, name)
    rep = check_forward(c)
    rep.update(check_backward(c))
    print(f"\n{name} ({time.time() - t0:.1f} s): " + ", ".join(
        f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in rep.items() if not isinstance(v, tuple)))
    print(parity.format_report({k: v for k, v in rep.items() if isinstance(v, tuple)}))


def test_case_matrix_reaches_the_edges(oracle, cameras):
    """The edges the power test relies on are really in the matrix (counted on the float64 forward)."""
    seen = dict(frustum_clamped_visible=0, behind_near_plane=0, clamped_colour=0, alpha_capped=0, T_stopped=0, near_floor=0,
                render_convention=0, scale_modifier_ne_1=0)
    for name in CASE_NAMES:
        c = oracle_case(oracle, cameras, name)
        pre, buf, kw = c["pre"], c["buf"], c["kw"]
        vis = ~pre["culled"]
        t = pre["p_view"].detach().numpy()
        out = (np.abs(t[:, 0] / t[:, 2]) > 1.3 * kw["tan_fovx"]) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * kw["tan_fovy"])
        seen["frustum_clamped_visible"] += int((out & vis & (t[:, 2] > 0)).sum())
        seen["behind_near_plane"] += int(pre["near"].sum())
        seen["clamped_colour"] += int(pre["clamped"][vis].any(1).sum())
        op = np.asarray(c["sc"]["opacities"]).ravel()
        seen["alpha_capped"] += int(((op > 0.99) & vis).sum())
        seen["near_floor"] += int(((op < 0.006) & vis).sum())
        seen["T_stopped"] += int((buf["final_Ts"] < 1e-3).sum())
        seen["render_convention"] += int(not np.array_equal(kw["viewmatrix"], c["cam"]["world_to_camera"]))
        seen["scale_modifier_ne_1"] += int(kw["scale_modifier"] != 1.0)
    print("\nedges in the case matrix:", seen)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("switch", list(F.SWITCHES))
def test_each_reference_convention_is_load_bearing(oracle, cameras, switch):
    """Flip one departure of the reference's backward away from the reference: the oracle must then FAIL the comparison on
    at least one case of the matrix.  A switch no case detects would mean the matrix misses that edge -- and that a kernel
    which got that convention wrong would pass."""
    for name in CASE_NAMES:
        c = oracle_case(oracle, cameras, name)
        try:
            check_backward(c, {switch: not F.SWITCHES[switch]})
        except AssertionError as err:
            print(f"\n{switch}: detected on {name}: {str(err).splitlines()[0][:140]}")
            return
    pytest.fail(f"flipping {switch} is not detected by any case")


def test_symmetric_camera_backward_is_the_gradient(cameras):
    """With a symmetric camera rotation block the forward's Sigma2D (Q1: J W Sigma W^T J^T) and the backward's textbook one
    (J W^T Sigma W J^T) coincide, so there plain end-to-end autograd of preprocess_f64 -> blend_f64 must equal the two-stage
    backward_f64 for dL_dmean3D, dL_dshs, dL_dopacity and dL_dcolor.  This checks the two-stage construction itself.  The
    departures that are not about Q1 are switched to the true gradient (none is active on this scene except the 1e-7 of
    denom_eps and the alpha cap, both switched), and the train.py convention makes Q3's term zero."""
    u = np.array([0.15, -0.1, 1.0])
    u /= np.linalg.norm(u)
    R = 2.0 * np.outer(u, u) - np.eye(3)                   # a 180-degree turn about u: symmetric, orthogonal
    sc, cam, kw = make_case(cameras, W=40, H=32, n=60, degree=3, train=True, bg=(0.3, 0.1, 0.2), sm=1.3, seed=21, R=R,
                            outside=0.0, behind=0.0, opaque=0.2)
    assert np.abs(kw["viewmatrix"][:3, :3] - kw["viewmatrix"][:3, :3].T).max() < 1e-6
    true = {"denom_eps": False, "alpha_cap_passes_grad": False, "frustum_clamp_grad": False}
    # the list order as the oracle's float32 forward makes it (the exact integer tests pin that order)
    from oracle import oracle as o
    buf = o.render_gaussians(**kw)[2]
    dpix = pixel_grad(32, 40, seed=5)
    r = F.backward_f64(sc, kw, buf["point_list"], buf["ranges"], dpix, true)
    N = sc["means"].shape[0]
    leaves = {"means": F._t(sc["means"], (N, 3)).requires_grad_(True), "shs": F._t(sc["shs"], (N, 16, 3)).requires_grad_(True),
              "opacities": F._t(sc["opacities"], (N,)).requires_grad_(True)}
    pre = F.preprocess_f64(dict(sc, **leaves), kw, 3, 1.3)
    col = pre["colour"]
    col.retain_grad()
    img = F.blend_f64(pre["xy"], pre["conic"], pre["opacity"], col, pre["depth"], buf["point_list"], buf["ranges"],
                      pre["cam"].bg, 40, 32, alpha_cap_grad=False)[0]
    (img * torch.as_tensor(dpix, dtype=torch.float64)).sum().backward()
    got = {"dL_dmean3D": leaves["means"].grad, "dL_dshs": leaves["shs"].grad.reshape(N * 16, 3),
           "dL_dopacity": leaves["opacities"].grad, "dL_dcolor": col.grad}
    assert (r["dL_dmean3D"] != 0).any()
    for k, v in got.items():
        np.testing.assert_allclose(v.numpy(), r[k], rtol=1e-9, atol=1e-12 * np.abs(r[k]).max(), err_msg=k)
