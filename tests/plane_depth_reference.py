"""
Float64 yardstick for the ray-plane intersection depth (include/gsr_plane_depth.h) -- the slopes, their image, its gradient stage
and the slopes' gradient -- and a float32 restatement of the header's steps.

Test helper, not a test file.

  (a), (d)  slopes_f64: torch float64, the header's definition with the float32 branch decision of every Gaussian passed in;
            slopes_vjp_f64: torch autograd of the image's dependence on (n, p) with the weights held constant,
                L(n, p) = sum_i  invd_i S0_i + gx_i (A1_i - x_i(p) S0_i) + gy_i (A2_i - y_i(p) S0_i),
            A1 = sum w g p.x = Sx + x_i S0 (a constant), x_i(p), y_i(p) the projected centre, invd = 1 / p_v.z: what (d) must be the
            derivative of.  branch_margins: the relative distance of every float32 decision of step 5 from its threshold.
  (b), (c)  yardstick: a dense (pixels x entries) float64 pass per tile over the structure blend_grad_reference.blend_grads_f64 hands
            out (its active entries, its pixel mask), the closed forms of that file with cd_k = g m_k(p); the CLAMP decision of every
            (pixel, entry) is taken from the header's float32 arithmetic, and a pixel with a decision within CLAMP_NEAR = 100 eps32 of
            invd_k of its threshold joins the pixel mask (its cotangent is zeroed on both sides): the three moments are discontinuous
            there.  Outputs with {"signed", "abs", "scale"} sums per Gaussian, as blend_grad_reference has them.

The float32 restatement (numpy) takes nothing from float64.  Frames are frame_walk_frames dicts (frame_of_buffers turns a forward's
buffers into one); the walk, the fused multiply-add and the backward's body are frame_walk_reference's, and what is written here is
the stage's own: m and its clamp, u = g m, total = g image, and the three moments as the tail.
"""
import numpy as np
import torch

import blend_grad_reference as B
import frame_walk_reference as FWR

f32 = np.float32
EPS32 = FWR.EPS32
MIN_COS, MAX_FLATNESS, NEAR, MAX_RATIO = f32(0.1), f32(0.5), f32(0.2), f32(4.0)
MARGIN_CAP = 100 * EPS32          # every decision a test keeps lies farther than this from its threshold
CLAMP_NEAR = MARGIN_CAP
OUTPUTS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dplane_moments")
COLUMNS = {"dL_dmean2D": (3, 4), "dL_dconic": (6, 7, 8, 9), "dL_dopacity": (10,)}
TOUCHED = (3, 4, 6, 7, 9, 10)
UNTOUCHED = (0, 1, 2, 5, 8, 11, 12, 13, 14, 15)
_np, fma32, criterion, rows_error, frame_of_buffers = FWR.to_np, FWR.fma32, FWR.criterion, FWR.rows_error, FWR.frame_of_buffers


def golden():
    """tests/golden/plane_depth_margins.json: "E_f32" {frame: {output: the restatement's error on the CPU oracle's buffers}}, "floor"
    (the smallest positive one), "E_kernel" (what an MI355X run measured per frame, tools/record_plane_depth_margins.py: a record
    only) and "mesh_gap_min" (null: no threshold on the mesh bias, README "Plane depth")."""
    return FWR.golden("plane_depth_margins")


# ---- (a), (d) ----
def steps(n, s, p, view, tx, ty, W, H, dt):
    """Steps 1-6 of the header in dtype dt, left to right.  dict: pv, t, l, fallback, kx, ky, slopes."""
    n, s, p, V = _np(n, dt), _np(s, dt), _np(p, dt), _np(view, dt).reshape(4, 4)
    with np.errstate(all="ignore"):
        pv = np.stack([((V[0, j] * p[:, 0] + V[1, j] * p[:, 1]) + V[2, j] * p[:, 2]) + V[3, j] for j in range(3)], 1)
        t = (n[:, 0] * pv[:, 0] + n[:, 1] * pv[:, 1]) + n[:, 2] * pv[:, 2]
        l = np.sqrt((pv[:, 0] * pv[:, 0] + pv[:, 1] * pv[:, 1]) + pv[:, 2] * pv[:, 2])
        lo = np.minimum(np.minimum(s[:, 0], s[:, 1]), s[:, 2])
        mid = np.maximum(np.minimum(s[:, 0], s[:, 1]), np.minimum(np.maximum(s[:, 0], s[:, 1]), s[:, 2]))
        fallback = (~n.any(1)) | ~(pv[:, 2] > dt(NEAR)) | ~(-t >= dt(MIN_COS) * l) | ~(lo <= dt(MAX_FLATNESS) * mid)
        kx, ky = (dt(2) * dt(tx)) / dt(W), (dt(2) * dt(ty)) / dt(H)
        td = np.where(fallback, dt(1), t)
        sl = np.stack([(n[:, 0] * kx) / td, (n[:, 1] * ky) / td], 1)
    return dict(n=n, V=V, pv=pv, t=t, l=l, lo=lo, mid=mid, fallback=fallback, kx=kx, ky=ky, slopes=np.where(fallback[:, None], dt(0), sl).astype(dt))


def slopes_f32(n, s, p, view, tx, ty, W, H):
    """(slopes (N, 2) float32, fallback (N,) bool) by the header's (a)."""
    r = steps(n, s, p, view, tx, ty, W, H, f32)
    return r["slopes"], r["fallback"]


def slopes_backward(n, s, p, view, tx, ty, W, H, mom, dt=f32, fallback=None):
    """(the addend to dL_dmean3D (N, 3), dL_dnormals (N, 3)) by the header's (d) in dtype dt (float32: the restatement; float64 with
    the float32 `fallback` passed in: the header's formulas themselves)."""
    r = steps(n, s, p, view, tx, ty, W, H, dt)
    fb = r["fallback"] if fallback is None else np.asarray(fallback, bool)
    pv, t, V, nn = r["pv"], np.where(fb, dt(1), r["t"]), r["V"], r["n"]
    kx, ky = r["kx"], r["ky"]
    S = _np(mom, dt)
    S0, Sx, Sy = S[:, 0], S[:, 1], S[:, 2]
    with np.errstate(all="ignore"):
        invd = np.where(pv[:, 2] > 0, dt(1) / np.where(pv[:, 2] > 0, pv[:, 2], dt(1)), dt(0))
        gx, gy = (nn[:, 0] * kx) / t, (nn[:, 1] * ky) / t
        M = (invd * S0 + gx * Sx) + gy * Sy
        R = np.stack([(pv[:, 0] * invd) * S0 + kx * Sx, (pv[:, 1] * invd) * S0 + ky * Sy, S0], 1)
        dn = (R - M[:, None] * pv) / t[:, None]
        dp = -((M[:, None] * nn) / t[:, None])
        zero = np.zeros_like(S0)
        dn = np.where(fb[:, None], dt(0), dn)
        dp = np.where(fb[:, None], np.stack([zero, zero, -((invd * invd) * S0)], 1), dp)
        dmean = np.stack([(V[r_, 0] * dp[:, 0] + V[r_, 1] * dp[:, 1]) + V[r_, 2] * dp[:, 2] for r_ in range(3)], 1)
    return dmean.astype(dt), dn.astype(dt)


def branch_margins(n, s, p, view):
    """(N,) float64: the smallest relative distance of a Gaussian's step-5 decisions from their thresholds, each in units of the
    magnitudes the float32 comparison rounds against (inf for the exact zero normal, which decides alone)."""
    r = steps(n, s, p, view, 1.0, 1.0, 1, 1, np.float64)
    pv, nn = r["pv"], r["n"]
    with np.errstate(all="ignore"):
        near = np.abs(pv[:, 2] - float(NEAR)) / np.maximum(np.abs(_np(p, np.float64)).max(1) + 1.0, float(NEAR))
        graze = np.abs(-r["t"] - float(MIN_COS) * r["l"]) / ((np.abs(nn) * np.abs(pv)).sum(1) + float(MIN_COS) * r["l"])
        flat = np.abs(r["lo"] - float(MAX_FLATNESS) * r["mid"]) / np.maximum(r["lo"], float(MAX_FLATNESS) * r["mid"])
    m = np.minimum(np.minimum(near, graze), flat)
    return np.where(nn.any(1), m, np.inf)


def pixel_of(pv, tx, ty, W, H):
    return ((pv[:, 0] / (pv[:, 2] * tx) + 1.0) * W - 1.0) * 0.5, ((pv[:, 1] / (pv[:, 2] * ty) + 1.0) * H - 1.0) * 0.5


def slopes_f64(n, s, p, view, tx, ty, W, H, fallback):
    """(N, 2) float64 slopes by the definition, the branch passed in."""
    r = steps(n, s, p, view, tx, ty, W, H, np.float64)
    fb = np.asarray(fallback, bool)
    t = np.where(fb, 1.0, r["t"])
    return np.where(fb[:, None], 0.0, np.stack([r["n"][:, 0] * r["kx"] / t, r["n"][:, 1] * r["ky"] / t], 1))


def slopes_vjp_f64(n, s, p, view, tx, ty, W, H, fallback, mom):
    """(dmean (N, 3), dn (N, 3), scale_mean (N, 3), scale_n (N, 3)) float64: torch autograd of L(n, p) above, and the sums of the
    magnitudes a float32 evaluation of (d) rounds against."""
    fb = torch.as_tensor(np.asarray(fallback, bool))
    nt = torch.tensor(_np(n, np.float64), requires_grad=True)
    pt = torch.tensor(_np(p, np.float64), requires_grad=True)
    V = torch.tensor(_np(view, np.float64).reshape(4, 4))
    S = torch.tensor(_np(mom, np.float64))
    pv = pt @ V[:3, :3] + V[3, :3]
    front = pv[:, 2].detach() > 0
    z = torch.where(front, pv[:, 2], torch.ones_like(pv[:, 2]))
    invd = torch.where(front, 1.0 / z, torch.zeros_like(z))
    t = torch.where(fb, torch.ones_like(z), (nt * pv).sum(1))
    kx, ky = 2.0 * tx / W, 2.0 * ty / H
    gx, gy = nt[:, 0] * kx / t, nt[:, 1] * ky / t
    x, y = pixel_of(torch.stack([pv[:, 0], pv[:, 1], z], 1), tx, ty, W, H)
    A1, A2 = S[:, 1] + x.detach() * S[:, 0], S[:, 2] + y.detach() * S[:, 0]
    plane = invd * S[:, 0] + gx * (A1 - x * S[:, 0]) + gy * (A2 - y * S[:, 0])
    L = torch.where(fb, invd * S[:, 0], plane).sum()
    dn, dmean = torch.autograd.grad(L, (nt, pt))
    # the units: every term of the header's formulas with magnitudes taken
    Sa, Va = np.abs(_np(mom, np.float64)), np.abs(V.numpy()[:3, :3])
    pva, na, ta = np.abs(pv.detach().numpy()), np.abs(_np(n, np.float64)), np.abs(t.detach().numpy())
    ia = invd.detach().numpy()
    Ma = ia * Sa[:, 0] + np.abs(gx.detach().numpy()) * Sa[:, 1] + np.abs(gy.detach().numpy()) * Sa[:, 2]
    Ra = np.stack([pva[:, 0] * ia * Sa[:, 0] + kx * Sa[:, 1], pva[:, 1] * ia * Sa[:, 0] + ky * Sa[:, 2], Sa[:, 0]], 1)
    f = fb.numpy()
    sn = np.where(f[:, None], 0.0, (Ra + Ma[:, None] * pva) / ta[:, None])
    sp = np.where(f[:, None], np.stack([0 * ia, 0 * ia, ia * ia * Sa[:, 0]], 1), Ma[:, None] * na / ta[:, None])
    return dmean.numpy(), dn.numpy(), sp @ Va.T, sn


def draw_gaussians(N, view, seed=5):
    """normals (N, 3), scales (N, 3), means (N, 3) float32 for (a) and (d), and the branch each special row is meant to take
    ({row: name}): random camera-facing unit normals over flat Gaussians in front of the camera, with a zero normal, a Gaussian
    behind the camera, one in front of it but inside the near plane, a grazing one and a round one mixed in where N allows."""
    rng = np.random.default_rng(seed)
    V = np.asarray(view, np.float64).reshape(4, 4)
    p = rng.uniform(-1.5, 1.5, (N, 3))
    s = np.exp(rng.uniform(-4, -1, (N, 3)))
    s[:, 2] = 0.2 * np.minimum(s[:, 0], s[:, 1])                                      # flat: lo / mid = 0.2
    centre = -V[3, :3] @ V[:3, :3].T
    special = {}
    if N > 8:
        special = {1: "zero", 3: "behind", 4: "near", 5: "grazing", 6: "round"}
        p[3] = centre - 1.0 * V[:3, 2] + 0.1 * p[3]
        p[4] = centre + 0.1 * V[:3, 2]
        s[6] = (0.1, 0.08, 0.1)                                                       # lo / mid = 0.8
    p = p.astype(f32)
    pv = p.astype(np.float64) @ V[:3, :3] + V[3, :3]
    n = rng.normal(0, 1, (N, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= np.where((n * pv).sum(1, keepdims=True) > 0, -1.0, 1.0)
    if N > 8:
        n[1] = 0
        d = pv[5] / np.linalg.norm(pv[5])
        e = np.cross(d, [0.3, -0.5, 0.8])
        n[5] = -(0.05 * d + np.sqrt(1 - 0.05 ** 2) * e / np.linalg.norm(e))           # cos = 0.05 < MIN_COS
    return n.astype(f32), s.astype(f32), p, special


# ---- (b), (c): the restatement ----
def inv_depth_of_buffers(nb):
    return FWR.inv_depth(nb, f32)


def _m32(fr, slopes, i, dx, dy):
    """(m, clamped) of the header's (b) for entry i at the pixels."""
    invd = fr["invd"][i]
    mr = fma32(-slopes[i, 0], dx, fma32(-slopes[i, 1], dy, np.full_like(dx, invd)))
    m = np.minimum(np.maximum(mr, invd * f32(0.25)), invd * MAX_RATIO)
    return m, m != mr


def render_f32(fr, slopes):
    """(out (H, W) float32, final_T (H, W) float32) by the header's (b)."""
    W, H = fr["W"], fr["H"]
    sl = _np(slopes, f32).reshape(-1, 2)
    out, Tf = np.zeros((H, W), f32), np.ones((H, W), f32)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        inside = (xs < W) & (ys < H)
        xs_, ys_ = xs[inside], ys[inside]
        acc, T = np.zeros(len(xs_), f32), np.ones(len(xs_), f32)
        for applied, alpha, G, dx, dy, i, *_ in FWR.walk_f32(fr, s, e, xs_, ys_, np.ones(len(xs_), bool)):
            m, _ = _m32(fr, sl, i, dx, dy)
            w = alpha * T
            T = np.where(applied, T * (f32(1) - alpha), T)
            acc = np.where(applied, fma32(w, m, acc), acc)
        out[ys_, xs_], Tf[ys_, xs_] = acc, T
    return out, Tf


def render_backward_f32(fr, slopes, g, image, drop_suffix=False):
    """(acc (N, 16), moments (N, 3)) float32 by the header's (c) (only the six columns it adds to are non-zero).  drop_suffix: a WRONG
    backward that forgets the suffix term of dL/dalpha, for the test that shows the criterion sees it."""
    W, H, N = fr["W"], fr["H"], fr["N"]
    sl, g32, img = _np(slopes, f32).reshape(-1, 2), _np(g, f32).reshape(H, W), _np(image, f32).reshape(H, W)
    acc, mom = np.zeros((N, 16), f32), np.zeros((N, 3), f32)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        for bx, by, inside in FWR.blocks(xs, ys, W, H):
            gg = FWR.block_values(g32, bx, by, inside)

            def entry(i, dx, dy, w):
                m, clamped = _m32(fr, sl, i, dx, dy)
                wg = np.where(clamped, f32(0), w * gg)
                return gg * m, (wg, wg * (-dx), wg * (-dy))

            for i, tail in FWR.backward_block(fr, s, e, bx, by, inside, gg * FWR.block_values(img, bx, by, inside), entry, acc, drop_suffix):
                mom[i] += tail
    return acc, mom


# ---- (b), (c): the yardstick ----
def yardstick(nb, W, H, invd, slopes, g):
    """nb: a forward's buffers; invd (N,), slopes (N, 2): the float32 arrays the kernel reads; g (H, W) dL/d(image), zeroed here at
    the masked pixels (the caller feeds the kernel r["g"]).  Returns dict: image (H, W) float64, coverage (H, W), mask (H, W) bool,
    g, clamped (how many applied (pixel, entry) pairs were clamped), clamp_margin (the smallest kept distance of a clamp decision
    from its threshold, in units of invd), and one {"signed", "abs", "scale"} dict per OUTPUTS key."""
    xy, co, pl, rg = FWR.arrays(nb)
    N = xy.shape[0]
    m0, sl = _np(invd, np.float64).reshape(-1), _np(slopes, np.float64).reshape(-1, 2)
    m032, sl32, xy32 = _np(invd, f32).reshape(-1), _np(slopes, f32).reshape(-1, 2), _np(nb["points_xy_image"], f32).reshape(-1, 2)
    tiles = []
    ref = B.blend_grads_f64(xy, co[:, :3], co[:, 3], np.ones((N, 3)), np.zeros(N), pl, rg, np.zeros(3), W, H, np.ones((H, W, 3)),
                            on_tile=lambda tile, xs, ys, idx, active, terms, masked: tiles.append((xs, ys, idx, active, masked)),
                            forward_n_contrib=nb["n_contrib"])
    mask = ref["mask"].copy()
    g64 = _np(g, np.float64).reshape(H, W)
    image, cover = np.zeros((H, W)), np.zeros((H, W))
    width = {"dL_dmean2D": 2, "dL_dconic": 4, "dL_dopacity": 1, "dL_dplane_moments": 3}
    out = {k: {s_: np.zeros((N, width[k])) for s_ in ("signed", "abs", "scale")} for k in OUTPUTS}
    n_clamped, margin = 0, np.inf
    for xs, ys, idx, active, masked in tiles:
        P, L = len(xs), len(idx)
        dx, dy = xy[idx, 0][None, :] - xs[:, None].astype(np.float64), xy[idx, 1][None, :] - ys[:, None].astype(np.float64)
        A, Bc, C, o = co[idx, 0][None, :], co[idx, 1][None, :], co[idx, 2][None, :], co[idx, 3][None, :]
        G = np.exp(-0.5 * (A * dx * dx + C * dy * dy) - Bc * dx * dy)
        alpha = np.minimum(0.99, o * G)
        om = np.where(active, 1.0 - alpha, 1.0)
        T = np.cumprod(np.concatenate([np.ones((P, 1)), om[:, :-1]], 1), 1)
        w = np.where(active, alpha * T, 0.0)
        # the clamp: decided by the header's float32 arithmetic
        dx32, dy32 = xy32[idx, 0][None, :] - xs[:, None].astype(f32), xy32[idx, 1][None, :] - ys[:, None].astype(f32)
        i32 = np.broadcast_to(m032[idx][None, :], (P, L))
        mr32 = fma32(-np.broadcast_to(sl32[idx, 0][None, :], (P, L)), dx32, fma32(-np.broadcast_to(sl32[idx, 1][None, :], (P, L)), dy32, i32))
        low, high = mr32 < i32 * f32(0.25), mr32 > i32 * MAX_RATIO
        mr = m0[idx][None, :] - sl[idx, 0][None, :] * dx - sl[idx, 1][None, :] * dy
        mi = np.broadcast_to(m0[idx][None, :], (P, L))
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = np.where(active & (mi > 0), np.minimum(np.abs(mr - 0.25 * mi), np.abs(mr - 4.0 * mi)) / np.where(mi > 0, mi, 1.0), np.inf)
        near = (dist < CLAMP_NEAR).any(1)
        bad = masked | near
        mask[ys, xs] = bad
        if (~bad).any():
            margin = min(margin, float(dist[~bad].min(initial=np.inf)))
        m = np.where(low, 0.25 * mi, np.where(high, 4.0 * mi, mr))
        free = active & ~(low | high)
        n_clamped += int((active & (low | high) & ~bad[:, None]).sum())
        w = np.where(bad[:, None], 0.0, w)           # (blend_grads_f64 zeroed its cotangent there; the weights of the kept pixels are untouched)
        active = active & ~bad[:, None]
        image[ys, xs], cover[ys, xs] = (w * m).sum(1), w.sum(1)
        gp = np.where(bad, 0.0, g64[ys, xs])[:, None]
        cd = gp * m
        S = w * cd
        behind = S.sum(1, keepdims=True) - np.cumsum(S, 1)
        Sa = np.abs(S)
        behind_abs = np.cumsum(Sa[:, ::-1], 1)[:, ::-1] - Sa
        dLda = np.where(active, T * cd - behind / (1.0 - alpha), 0.0)
        dLda_s = np.where(active, np.abs(T * cd) + behind_abs / (1.0 - alpha), 0.0)
        h, h_s = o * G * dLda, np.abs(o * G) * dLda_s
        fx, fy = (A * dx + Bc * dy) * (0.5 * W), (C * dy + Bc * dx) * (0.5 * H)
        fa, fb, fc = 0.5 * dx * dx, 0.5 * dx * dy, 0.5 * dy * dy
        z = np.zeros_like(h)
        wg = np.where(free, w * gp, 0.0)
        terms = {"dL_dmean2D": np.stack([-h * fx, -h * fy], 2), "dL_dconic": np.stack([-h * fa, -h * fb, z, -h * fc], 2),
                 "dL_dopacity": (G * dLda)[:, :, None], "dL_dplane_moments": np.stack([wg, wg * -dx, wg * -dy], 2)}
        scales = {"dL_dmean2D": np.stack([h_s * np.abs(fx), h_s * np.abs(fy)], 2), "dL_dconic": np.stack([h_s * fa, h_s * np.abs(fb), z, h_s * fc], 2),
                  "dL_dopacity": (G * dLda_s)[:, :, None], "dL_dplane_moments": np.abs(terms["dL_dplane_moments"])}
        for k in OUTPUTS:
            np.add.at(out[k]["signed"], idx, terms[k].sum(0))
            np.add.at(out[k]["abs"], idx, np.abs(terms[k]).sum(0))
            np.add.at(out[k]["scale"], idx, scales[k].sum(0))
    out.update(image=image, coverage=cover, mask=mask, g=np.where(mask, 0.0, g64), clamped=n_clamped, clamp_margin=margin)
    return out


def layout(acc, mom, key):
    return FWR.layout(acc, key, COLUMNS, mom)


def backward_errors(acc, mom, r):
    """{key: worst per-Gaussian error in the key's scale}."""
    return FWR.backward_errors(acc, r, OUTPUTS, COLUMNS, mom)


def spread(a, b, r):
    """The worst difference of two runs' (acc, moments) in the same units."""
    return FWR.spread(a, b, r, OUTPUTS, COLUMNS)


def image_error(img, r, invd):
    """max |img - image64| / max invd over the unmasked pixels: the image is a sum of weights <= 1 times inverse depths."""
    d = np.abs(_np(img, np.float64).reshape(r["image"].shape) - r["image"])[~r["mask"]]
    return float(d.max() / np.abs(_np(invd, np.float64)).max()) if d.size else 0.0


def draw_g(H, W, seed=7):
    """dL/d(image) from U(-1, 1) / (W H): signed, as a depth loss's gradient is, and uneven, so that a swapped pixel shows."""
    return (np.random.default_rng(seed).uniform(-1, 1, (H, W)) / (W * H)).astype(f32)


def plane_scales(scales):
    """The scales handed to plane_slopes on the frame matrix: the scene's with the smallest axis (the normal's: the same c*) shrunk to
    0.3 of itself, so that most Gaussians are flat and take the plane branch; the drawn scenes' own scales are round three times in four
    and would measure the fallback."""
    s = _np(scales, f32).copy()
    c = np.argmin(s, axis=1)
    s[np.arange(len(s)), c] *= f32(0.3)
    return s


CPU_FRAMES = ("n300_50x37", "n2000_64x48", "n900_faint_48x32", "n1500_opaque_48x48")      # features_reference.SCENES


def sheet(scenes_mod, cameras_mod, degrees=45.0, side=12, W=48, H=48):
    """(scene, camera, render kwargs, th): side x side equal flat discs on a plane through the origin tilted by `degrees` about x,
    seen by the toy camera: the closed form's frame."""
    from conftest import render_kwargs
    cam = cameras_mod.toy_camera(image_width=W, image_height=H)
    th = np.deg2rad(degrees)
    u, v = np.meshgrid(np.linspace(-1.6, 1.6, side), np.linspace(-1.6, 1.6, side))
    pts = np.stack([u.ravel(), v.ravel() * np.cos(th), v.ravel() * np.sin(th)], 1).astype(f32)
    sc = scenes_mod.synthetic_scene(len(pts), 0.05, 0.6, 1)
    sc["means"] = pts
    sc["scales"][:] = np.array([0.2, 0.2, 0.004], f32)
    sc["rotations"][:] = np.array([np.sin(th / 2), 0, 0, np.cos(th / 2)], f32)      # (x, y, z, w): `degrees` about x
    sc["opacities"][:] = 0.9
    return sc, cam, render_kwargs(sc, cam, width=W, height=H), th


def plane_inverse_depth(n, mu0, tx, ty, W, H):
    """(H, W) float64: (n . r(p)) / (n . mu0), the inverse depth at which each pixel's ray meets the plane through mu0 with normal n."""
    n, mu0 = np.asarray(n, np.float64), np.asarray(mu0, np.float64)
    rx = ((2.0 * np.arange(W) + 1.0) / W - 1.0) * tx
    ry = ((2.0 * np.arange(H) + 1.0) / H - 1.0) * ty
    return (n[0] * rx[None, :] + n[1] * ry[:, None] + n[2]) / float(n @ mu0)
