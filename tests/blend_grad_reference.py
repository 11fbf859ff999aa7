"""
Float64 yardstick for EVERY blend-stage gradient (blend_bwd_splat.hip), Gaussian by Gaussian.

Test helper like tests/absgrad_reference.py, which it generalises, not a test file.  A dense (pixels x entries) float64 replay per
16x16 tile over a given point_list / ranges, every per-(pixel, entry) term in CLOSED FORM (no autograd).  Notation of
absgrad_reference.py: pixel p, k-th entry of its tile's list, d = xy_k - p, conic (A, B, C), G = exp(power),
power = -0.5 (A dx^2 + C dy^2) - B dx dy, alpha = min(0.99, o G), T_k = prod_{j<k} (1 - alpha_j) over the contributing entries,
w_k = alpha_k T_k, cd_k = c_k . dpix + gD invd_k, S_j = w_j cd_j, seed = T_final (bg . dpix - gA):

    dL/dalpha_k = T_k cd_k - (sum_{j>k} S_j + seed) / (1 - alpha_k)
    h           = o G dL/dalpha_k                        (the gradient passes the 0.99 cap)
    dL_dcolor      += w_k dpix                           dL_dinv_depths += w_k gD
    dL_dopacity    += G dL/dalpha_k
    dL_dmean2D     += (-h (A dx + B dy) 0.5 W, -h (C dy + B dx) 0.5 H)
    dL_dconic      += (-0.5 dx^2 h, -0.5 dx dy h, 0, -0.5 dy^2 h)      (the kernel's columns: A, B as stored -- half --, unused, C)

for contributing entries (power <= 0, alpha >= 1/255, before the entry at which T (1 - alpha) would fall below 1e-4), else 0.  The
decisions are taken in float64 here, independently of the forward under test.

Three sums per Gaussian and output: `signed` (the gradient), `abs` (the sum of the terms' magnitudes; for dL_dmean2D what
absgrad=True returns) and `scale`: the same expression with T_k cd_k replaced by |T_k cd_k| and (sum_{j>k} S_j + seed) by
(sum_{j>k} |S_j| + |seed|), magnitudes taken of every factor.  dL/dalpha_k is a difference of two such sums, and a float32
evaluation errs relative to their magnitudes, not to their difference: `scale` is the unit a per-Gaussian error is measured in
(what cov_scale is to test_f64_reference.geometry_margins).  For dL_dcolor and dL_dinv_depths a term has no inner cancellation,
so scale = abs.

Per pixel: the float64 n_contrib and a DECISION MARGIN, the smallest relative distance of any decision taken at that pixel from
its threshold, over the entries up to and including the stopping one (behind it no decision is taken):
    power <= 0          |power| / M,              M = 0.5 (|A| dx^2 + |C| dy^2) + |B dx dy| (what a float32 power rounds against)
    alpha >= 1/255      |255 o G - 1| / (1 + M)   (G's relative error is the exp's own plus power's absolute one)
    alpha > 0.99        |o G / 0.99 - 1| / (1 + M)
    T (1 - alpha) < 1e-4   |T (1 - alpha) / 1e-4 - 1| / (k + 1): T is a product of up to k + 1 rounded factors
A test zeroes its cotangents where the margin is below a width NEAR, or where n_contrib differs from the forward's; the backward
is linear in (dL_dpixels, dL_ddepth_image, dL_dalpha_image), so both sides lose exactly those pixels.

`on_tile(tile, xs, ys, idx, active, terms, masked)` is called per non-empty tile with the dense arrays (terms: the dict of
(P, L, n) signed terms; masked: (P,) bool, the tile's pixels whose cotangents were zeroed) for tests that need the terms of one block or one list position.
"""
import numpy as np
import torch

TILE = 16
D = torch.float64
OUTPUTS = ("dL_dcolor", "dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dinv_depths")
WIDTH = {"dL_dcolor": 3, "dL_dmean2D": 2, "dL_dconic": 4, "dL_dopacity": 1, "dL_dinv_depths": 1}
# NEAR = EXP_REL * NEAR_FACTOR.  EXP_REL is the exp error tests/parity.py states (v_exp_f32 against libm expf, 5e-7 relative).
# In the margins' units (relative to 1 + M) a float32 alpha is off by: the exp, 1 x EXP_REL; power's own rounding -- dx, dy, three
# products of three factors and two sums, at most 10 roundings of 2^-24 = 6e-7 M -- 1.2 x; o G and the comparison's constant, 0.2 x:
# 2.4 x EXP_REL.  The factor 8 leaves a bit more than 3 x on that model; test_blend_grad_reference.py shows the oracle's forward
# agreeing with float64 on every decision the mask keeps at this width.
EXP_REL = 5e-7
NEAR_FACTOR = 8.0
NEAR = EXP_REL * NEAR_FACTOR


def _t(a, shape=None):
    t = a.detach().to(D) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float64))
    return t.reshape(shape) if shape is not None else t


def blend_grads_f64(xy, conic, opacity, colour, inv_depth, point_list, ranges, bg, W, H, dL_dpixels=None, dL_dinv_depth=None,
                    dL_dalpha=None, on_tile=None, forward_n_contrib=None, near=NEAR):
    """Returns {output: {"signed", "abs", "scale"}} of (N, width) float64 numpy arrays (OUTPUTS, WIDTH), plus "n_contrib" (H, W)
    int64, "margin" (H, W) float64 (inf where no decision is taken) and "mask" (H, W) bool.  With `forward_n_contrib` (the
    n_contrib of the forward buffers handed to the backward under test) the cotangents are zeroed here at the pixels of
    pixel_mask(), which "mask" then is; the caller zeroes them there as well (masked()).  Without it "mask" is all False."""
    xy, conic, opacity, colour, inv_depth = _t(xy, (-1, 2)), _t(conic, (-1, 3)), _t(opacity, (-1,)), _t(colour, (-1, 3)), _t(inv_depth, (-1,))
    N = xy.shape[0]
    bg = _t(bg, (3,))
    dpix = _t(dL_dpixels, (H, W, 3)) if dL_dpixels is not None else torch.zeros(H, W, 3, dtype=D)
    gD = _t(dL_dinv_depth, (H, W)) if dL_dinv_depth is not None else torch.zeros(H, W, dtype=D)
    gA = _t(dL_dalpha, (H, W)) if dL_dalpha is not None else torch.zeros(H, W, dtype=D)
    pl = torch.as_tensor(np.asarray(point_list, dtype=np.int64)).reshape(-1)
    ranges = np.asarray(ranges).reshape(-1, 2)
    acc = {k: {s: torch.zeros(N, WIDTH[k], dtype=D) for s in ("signed", "abs", "scale")} for k in OUTPUTS}
    n_contrib = torch.zeros(H, W, dtype=torch.int64)
    margin = torch.full((H, W), float("inf"), dtype=D)
    mask = torch.zeros(H, W, dtype=torch.bool)
    fwd_nc = None
    if forward_n_contrib is not None:
        fwd_nc = torch.as_tensor(np.asarray(forward_n_contrib.detach().cpu() if torch.is_tensor(forward_n_contrib) else forward_n_contrib,
                                            dtype=np.int64)).reshape(H, W)
        empty = np.repeat(np.repeat((ranges[:, 1] <= ranges[:, 0]).reshape((H + TILE - 1) // TILE, -1), TILE, 0), TILE, 1)[:H, :W]
        mask |= torch.as_tensor(empty) & (fwd_nc != 0)                  # (a tile without a list: n_contrib is 0, nothing is decided)
    gx = (W + TILE - 1) // TILE
    inf = torch.tensor(float("inf"), dtype=D)
    for tid in range(ranges.shape[0]):
        s, e = int(ranges[tid, 0]), int(ranges[tid, 1])
        if e <= s:
            continue
        tx, ty = tid % gx, tid // gx
        ys, xs = np.meshgrid(np.arange(ty * TILE, min(H, ty * TILE + TILE)), np.arange(tx * TILE, min(W, tx * TILE + TILE)), indexing="ij")
        yt, xt = torch.as_tensor(ys.ravel()), torch.as_tensor(xs.ravel())
        idx = pl[s:e]
        P, L = yt.numel(), idx.numel()
        dx = xy[idx, 0][None, :] - xt.to(D)[:, None]
        dy = xy[idx, 1][None, :] - yt.to(D)[:, None]
        A, B, C = conic[idx, 0][None, :], conic[idx, 1][None, :], conic[idx, 2][None, :]
        o = opacity[idx][None, :]
        power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
        M = 0.5 * (A.abs() * dx * dx + C.abs() * dy * dy) + (B * dx * dy).abs()
        G = torch.exp(power)
        a_raw = o * G
        alpha = torch.clamp(a_raw, max=0.99)
        keep = (power <= 0) & (alpha >= 1.0 / 255.0)
        one_minus = torch.where(keep, 1.0 - alpha, torch.ones_like(alpha))
        ones = torch.ones(P, 1, dtype=D)
        T_in = torch.cumprod(torch.cat([ones, one_minus[:, :-1]], 1), 1)
        stop = keep & (T_in * one_minus < 1e-4)                       # the stopping entry is excluded, and everything behind it
        pos = torch.arange(L)[None, :].expand(P, L)
        first_stop = torch.where(stop, pos, torch.full_like(pos, L)).min(1).values
        active = keep & (pos < first_stop[:, None])
        n_contrib[yt, xt] = torch.where(active, pos + 1, torch.zeros_like(pos)).max(1).values
        # decision margins, over the entries at which a decision is taken
        decided = pos <= first_stop[:, None]
        m_pow = torch.where(M > 0, power.abs() / torch.where(M > 0, M, torch.ones_like(M)), inf)
        m_a = torch.where(power <= 0, torch.minimum((255.0 * a_raw - 1.0).abs(), (a_raw / 0.99 - 1.0).abs()) / (1.0 + M), inf)
        m_T = torch.where(keep, (T_in * one_minus / 1e-4 - 1.0).abs() / (pos + 1).to(D), inf)
        m = torch.minimum(torch.minimum(m_pow, m_a), m_T)
        margin[yt, xt] = torch.where(decided, m, inf).min(1).values
        # the terms
        one_minus = torch.where(active, 1.0 - alpha, torch.ones_like(alpha))
        T_k = torch.cumprod(torch.cat([ones, one_minus[:, :-1]], 1), 1)
        T_final = one_minus.prod(1)
        dp, gd, ga = dpix[yt, xt], gD[yt, xt], gA[yt, xt]
        if fwd_nc is not None:
            bad = (margin[yt, xt] < near) | (n_contrib[yt, xt] != fwd_nc[yt, xt])
            mask[yt, xt] = bad
            good = (~bad).to(D)
            dp, gd, ga = dp * good[:, None], gd * good, ga * good
        else:
            bad = torch.zeros(P, dtype=torch.bool)
        cd = dp @ colour[idx].T + gd[:, None] * inv_depth[idx][None, :]
        zero = torch.zeros_like(cd)
        w = torch.where(active, alpha * T_k, zero)
        S = w * cd
        behind = S.sum(1, keepdim=True) - torch.cumsum(S, 1)           # sum over entries behind k
        Sa = S.abs()
        behind_abs = torch.flip(torch.cumsum(torch.flip(Sa, [1]), 1), [1]) - Sa     # (no cancellation: a plain suffix sum)
        seed = T_final * (dp @ bg - ga)
        dLda = T_k * cd - (behind + seed[:, None]) / (1.0 - alpha)
        dLda_s = (T_k * cd).abs() + (behind_abs + seed.abs()[:, None]) / (1.0 - alpha)
        dLda, dLda_s = torch.where(active, dLda, zero), torch.where(active, dLda_s, zero)
        h, h_s = o * G * dLda, (o * G).abs() * dLda_s
        fx, fy = (A * dx + B * dy) * (0.5 * W), (C * dy + B * dx) * (0.5 * H)
        fa, fb, fc = 0.5 * dx * dx, 0.5 * dx * dy, 0.5 * dy * dy
        z = zero
        terms = {
            "dL_dcolor": torch.stack([w * dp[:, c:c + 1] for c in range(3)], 2),
            "dL_dmean2D": torch.stack([-h * fx, -h * fy], 2),
            "dL_dconic": torch.stack([-h * fa, -h * fb, z, -h * fc], 2),
            "dL_dopacity": (G * dLda)[:, :, None],
            "dL_dinv_depths": (w * gd[:, None])[:, :, None],
        }
        scales = {
            "dL_dcolor": terms["dL_dcolor"].abs(),
            "dL_dmean2D": torch.stack([h_s * fx.abs(), h_s * fy.abs()], 2),
            "dL_dconic": torch.stack([h_s * fa, h_s * fb.abs(), z, h_s * fc], 2),
            "dL_dopacity": (G * dLda_s)[:, :, None],
            "dL_dinv_depths": terms["dL_dinv_depths"].abs(),
        }
        for k in OUTPUTS:
            acc[k]["signed"].index_add_(0, idx, terms[k].sum(0))
            acc[k]["abs"].index_add_(0, idx, terms[k].abs().sum(0))
            acc[k]["scale"].index_add_(0, idx, scales[k].sum(0))
        if on_tile is not None:
            on_tile(tid, xs.ravel(), ys.ravel(), idx.numpy(), active.numpy(), {k: v.numpy() for k, v in terms.items()}, bad.numpy())
    out = {k: {s: v.numpy() for s, v in d.items()} for k, d in acc.items()}
    out["n_contrib"] = n_contrib.numpy()
    out["margin"] = margin.numpy()
    out["mask"] = mask.numpy()
    return out


def _inv_depth(depth):
    depth = _t(depth, (-1,))
    return torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth))


def of_buffers(buf, bg, W, H, dL_dpixels=None, dL_dinv_depth=None, dL_dalpha=None, on_tile=None, point_list=None, mask_against_forward=True):
    """blend_grads_f64 on the checked side's own per-Gaussian float32 buffers widened to float64 (as
    test_f64_reference.blend_on_buffers: their rounding is the per-Gaussian models' business, not counted twice)."""
    n = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    co = n(buf["conic_opacity"]).reshape(-1, 4)
    pl = buf["point_list"] if point_list is None else point_list
    pl = pl.detach().cpu().numpy() if torch.is_tensor(pl) else pl
    rg = buf["ranges"].detach().cpu().numpy() if torch.is_tensor(buf["ranges"]) else buf["ranges"]
    return blend_grads_f64(n(buf["points_xy_image"]), co[:, :3], co[:, 3], n(buf["colors"]), _inv_depth(n(buf["depths"])), pl, rg,
                           n(bg)[:3], W, H, dL_dpixels, dL_dinv_depth, dL_dalpha, on_tile,
                           forward_n_contrib=buf["n_contrib"] if mask_against_forward else None)


def of_case(pre, point_list, ranges, dL_dpixels=None, dL_dinv_depth=None, dL_dalpha=None, on_tile=None):
    """blend_grads_f64 on the float64 per-Gaussian quantities of f64_reference.preprocess_f64 (`pre`)."""
    cam = pre["cam"]
    return blend_grads_f64(pre["xy"], pre["conic"], pre["opacity"], pre["colour"], _inv_depth(pre["depth"]), point_list, ranges, cam.bg,
                           cam.W, cam.H, dL_dpixels, dL_dinv_depth, dL_dalpha, on_tile)


def pixel_mask(ref, forward_n_contrib, near=NEAR):
    """(H, W) bool: the pixels a test must zero its cotangents at -- a decision within `near` of its threshold, or a float64
    n_contrib other than the forward's."""
    nc = np.asarray(forward_n_contrib.detach().cpu() if torch.is_tensor(forward_n_contrib) else forward_n_contrib).reshape(ref["n_contrib"].shape)
    return (ref["margin"] < near) | (ref["n_contrib"] != nc)


def masked(mask, *cotangents):
    """Copies of the cotangent images ((H, W) or (H, W, 3), or None) with the masked pixels zeroed."""
    out = []
    for c in cotangents:
        if c is None:
            out.append(None)
            continue
        c = np.array(c, dtype=np.float32, copy=True)
        c[mask] = 0
        out.append(c)
    return out


def kernel_layout(g, key):
    """The (N, WIDTH[key]) float64 array of a backward()'s result dict (kernel or oracle) that `key`'s sums are compared with."""
    a = g[key]
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    if key == "dL_dmean2D":
        return a.reshape(-1, 3)[:, :2] if a.ndim == 2 and a.shape[1] == 3 else a.reshape(-1, 2)
    return a.reshape(-1, WIDTH[key])


def errors(got, ref_out):
    """Per-Gaussian error of `got` (N, width) against one output's sums, in units of its scale, component by component: (N,)
    float64, the worst component.  A component whose scale is 0 must be exactly 0: it counts as inf otherwise."""
    got = np.asarray(got, np.float64).reshape(ref_out["signed"].shape)
    sc = ref_out["scale"]
    d = np.abs(got - ref_out["signed"])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(sc > 0, d / np.where(sc > 0, sc, 1.0), np.where(got != 0, np.inf, 0.0))
    return e.max(1) if e.size else np.zeros(e.shape[0])


def worst(got, ref_out):
    e = errors(got, ref_out)
    return float(e.max()) if e.size else 0.0
