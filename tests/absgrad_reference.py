"""
Float64 yardstick for the absolute screen-space gradients (include/gsr_densify_stats.h, GSR_BWD_ABSGRAD).

Test helper like tests/f64_reference.py and tests/camera_grad_reference.py, not a test file.  A dense (pixels x entries) float64
blend per 16x16 tile over a given point_list / ranges, with the per-(pixel, entry) term of dL/dmean2D written in CLOSED FORM (no
autograd), so that both its signed sum -- which must be the blend-stage dL_dmean2D of tests/f64_reference.py -- and the sum of its
magnitudes -- what the ABS kernels accumulate -- come out of one expression.  For pixel p and the k-th entry of its tile's list
(front to back), with d = xy_k - p, conic (A, B, C), G = exp(-0.5 (A dx^2 + C dy^2) - B dx dy), alpha = min(0.99, o G),
T_k = prod_{j<k} (1 - alpha_j) over the contributing entries, cd_j = c_j . dpix + gD invd_j:

    dL/dalpha_k = T_k cd_k - (sum_{j>k} alpha_j T_j cd_j + T_final (bg . dpix - gA)) / (1 - alpha_k)
    h           = o G dL/dalpha_k                        (the gradient passes the 0.99 cap, backward.py:683)
    term_x      = -h (A dx + B dy) 0.5 W                 term_y = -h (C dy + B dx) 0.5 H

for contributing entries (power <= 0, alpha >= 1/255, before the entry at which T would fall below 1e-4), else 0.  The discrete
decisions are taken in float64 here, independently of the forward under test.  tests/test_absgrad_abi.py checks this module
against f64_reference's autograd, sum and pixel by pixel.
"""
import numpy as np
import torch

TILE = 16
D = torch.float64


def _t(a, shape=None):
    t = a.detach().to(D) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float64))
    return t.reshape(shape) if shape is not None else t


def mean2d_terms_f64(xy, conic, opacity, colour, inv_depth, point_list, ranges, bg, W, H, dL_dpixels=None, dL_dinv_depth=None,
                     dL_dalpha=None, per_pixel=False):
    """Returns {"signed": (N, 2), "abs": (N, 2)} float64 numpy arrays: the sum over pixels and list entries of term_x / term_y
    and of their magnitudes, per Gaussian; with per_pixel=True also "terms": (H * W, N, 2), the term of every (pixel, Gaussian)."""
    xy, conic, opacity, colour, inv_depth = _t(xy, (-1, 2)), _t(conic, (-1, 3)), _t(opacity, (-1,)), _t(colour, (-1, 3)), _t(inv_depth, (-1,))
    N = xy.shape[0]
    bg = _t(bg, (3,))
    dpix = _t(dL_dpixels, (H, W, 3)) if dL_dpixels is not None else torch.zeros(H, W, 3, dtype=D)
    gD = _t(dL_dinv_depth, (H, W)) if dL_dinv_depth is not None else torch.zeros(H, W, dtype=D)
    gA = _t(dL_dalpha, (H, W)) if dL_dalpha is not None else torch.zeros(H, W, dtype=D)
    pl = torch.as_tensor(np.asarray(point_list, dtype=np.int64)).reshape(-1)
    ranges = np.asarray(ranges).reshape(-1, 2)
    signed, absolute = torch.zeros(N, 2, dtype=D), torch.zeros(N, 2, dtype=D)
    terms = torch.zeros(H * W, N, 2, dtype=D) if per_pixel else None
    gx = (W + TILE - 1) // TILE
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
        G = torch.exp(power)
        alpha = torch.clamp(o * G, max=0.99)
        keep = (power <= 0) & (alpha >= 1.0 / 255.0)
        one_minus = torch.where(keep, 1.0 - alpha, torch.ones_like(alpha))
        T_in = torch.cumprod(torch.cat([torch.ones(P, 1, dtype=D), one_minus[:, :-1]], 1), 1)
        stop = keep & (T_in * one_minus < 1e-4)                       # the stopping entry is excluded, and everything behind it
        pos = torch.arange(L)[None, :].expand(P, L)
        first_stop = torch.where(stop, pos, torch.full_like(pos, L)).min(1).values
        active = keep & (pos < first_stop[:, None])
        one_minus = torch.where(active, 1.0 - alpha, torch.ones_like(alpha))
        T_k = torch.cumprod(torch.cat([torch.ones(P, 1, dtype=D), one_minus[:, :-1]], 1), 1)
        T_final = one_minus.prod(1)
        dp, gd, ga = dpix[yt, xt], gD[yt, xt], gA[yt, xt]
        cd = dp @ colour[idx].T + gd[:, None] * inv_depth[idx][None, :]
        S = torch.where(active, alpha * T_k * cd, torch.zeros_like(cd))
        behind = S.sum(1, keepdim=True) - torch.cumsum(S, 1)           # sum over entries behind k
        seed = T_final * (dp @ bg - ga)
        dL_dalpha_k = T_k * cd - (behind + seed[:, None]) / (1.0 - alpha)
        h = torch.where(active, o * G * dL_dalpha_k, torch.zeros_like(cd))
        t_x = -h * (A * dx + B * dy) * (0.5 * W)
        t_y = -h * (C * dy + B * dx) * (0.5 * H)
        t = torch.stack([t_x, t_y], 2)                                 # (P, L, 2)
        signed.index_add_(0, idx, t.sum(0))
        absolute.index_add_(0, idx, t.abs().sum(0))
        if per_pixel:
            rows = (yt * W + xt)[:, None].expand(P, L).reshape(-1)
            cols = idx[None, :].expand(P, L).reshape(-1)
            terms.index_put_((rows, cols), t.reshape(-1, 2), accumulate=True)
    out = {"signed": signed.numpy(), "abs": absolute.numpy()}
    if per_pixel:
        out["terms"] = terms.numpy()
    return out


def of_case(pre, point_list, ranges, dL_dpixels=None, dL_dinv_depth=None, dL_dalpha=None, per_pixel=False):
    """mean2d_terms_f64 on the float64 per-Gaussian quantities of f64_reference.preprocess_f64 (`pre`)."""
    cam = pre["cam"]
    depth = pre["depth"].detach()
    inv_depth = torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth))
    return mean2d_terms_f64(pre["xy"], pre["conic"], pre["opacity"], pre["colour"], inv_depth, point_list, ranges, cam.bg, cam.W, cam.H,
                            dL_dpixels, dL_dinv_depth, dL_dalpha, per_pixel)
