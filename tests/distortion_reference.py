"""
Float64 yardstick for the depth-distortion regulariser (include/gsr_distortion.h), and a float32 restatement of the header's steps.

Test helper, not a test file.  The yardstick is two passes of blend_grad_reference.blend_grads_f64 over a frame's buffers:

  pass one   colour 1, dL_dpixels = 1, background 0: the `on_tile` callback's terms["dL_dcolor"][:, :, 0] is the weight w_k(p) of
             every (pixel, entry) pair -- zero where the entry does not contribute and at the pixels the module masks -- and from
             the weights, per pixel, A = sum w, mu = sum w m / A, S = sum w (m - mu)^2 and Dist = A S (m = 1 / depth);
  pass two   colour (1, m, m^2), dL_dpixels = g (A mu^2 + S, -2 A mu, A), background 0: c_k . dL_dpixels is then
             dL/dw_k = g (A (m_k - mu)^2 + S), so the pass's dL_dmean2D, dL_dconic and dL_dopacity are the distortion term's, with
             their `scale` units, and dL/dm = dL_dcolor[:, 1] + 2 m dL_dcolor[:, 2] = sum_p 2 g w A (m - mu).

The unit of dL/dm is scale[:, 1] + 2 |m| scale[:, 2] = sum_p w |g| 2 A (mu + |m|): what a float32 (m - mu) errs against is the
magnitude of m and mu (mu is a rounded number), not their difference.

The float32 restatement (numpy) takes nothing from float64: it replays the header on the same buffers, step by step -- weights as
features_reference.weights_f32, the running A, mu, S of the forward, and the backward's total-minus-prefix walk with the block
sums in the header's order (pixels 0-31 of an 8x8 block in order, pixels 32-63 in order, then the two halves) -- and adds the
seven columns per (block, entry) to a float32 (N, 16) array of accumulator rows in tile, block and list order.  form="moments" is
the forward by A M2 - M1^2 instead, which the thin-slab test must see fail.

Errors.  Forward: max over the unmasked pixels of |dist - Dist| / (Dist (1 + mu / sigma)), sigma^2 = S / A -- relative, in units
of 1 + kappa; divided by eps32 it is the "eps32 mu / sigma" figure.  A pixel whose Dist is exactly 0 (one contributor, equal
depths) must be exactly 0.  Backward: blend_grad_reference.errors per output, in its scale.
"""
import json
import os

import numpy as np

import blend_grad_reference as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distortion_margins.json")
f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
OUTPUTS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dinv_depths")
COLUMNS = {"dL_dmean2D": (3, 4), "dL_dconic": (6, 7, 8, 9), "dL_dopacity": (10,), "dL_dinv_depths": (11,)}
TOUCHED = (3, 4, 6, 7, 9, 10, 11)
UNTOUCHED = (0, 1, 2, 5, 8, 12, 13, 14, 15)


def golden():
    """tests/golden/distortion_margins.json: "floor" {"forward", "backward"}, the smallest float32-restatement errors of the CPU
    matrix; "thin_slab_bound", the restatement's bound on a thin slab in eps32 mu / sigma; "E_kernel", what an MI355X run measured
    per frame (tools/record_distortion_margins.py)."""
    with open(GOLDEN) as f:
        return json.load(f)


def _np(a, dtype=None):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def inv_depth(buf, dtype=np.float64):
    d = _np(buf["depths"], dtype).reshape(-1)
    return np.where(d > 0, dtype(1) / np.where(d > 0, d, dtype(1)), dtype(0)).astype(dtype)


def _arrays(buf):
    return (_np(buf["points_xy_image"], np.float64).reshape(-1, 2), _np(buf["conic_opacity"], np.float64).reshape(-1, 4),
            _np(buf["point_list"]).reshape(-1), _np(buf["ranges"]).reshape(-1, 2))


def moments_f64(buf, W, H, m=None):
    """Pass one.  Returns dict: A, mu, S, dist (H, W) float64, mask (H, W) bool, n_contrib64, tiles (tile, xs, ys, idx, w, masked, active)."""
    xy, co, pl, rg = _arrays(buf)
    N = xy.shape[0]
    m = inv_depth(buf) if m is None else np.asarray(m, np.float64)
    A, mu, S = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    tiles = []

    def on_tile(tile, xs, ys, idx, active, terms, masked):
        w = terms["dL_dcolor"][:, :, 0]
        tiles.append((tile, xs, ys, idx, w, masked, active))
        a = w.sum(1)
        mean = np.where(a > 0, (w @ m[idx]) / np.where(a > 0, a, 1.0), 0.0)
        A[ys, xs], mu[ys, xs] = a, mean
        S[ys, xs] = (w * (m[idx][None, :] - mean[:, None]) ** 2).sum(1)

    ref = B.blend_grads_f64(xy, co[:, :3], co[:, 3], np.ones((N, 3)), m, pl, rg, np.zeros(3), W, H, np.ones((H, W, 3)), on_tile=on_tile,
                            forward_n_contrib=buf["n_contrib"])
    return dict(A=A, mu=mu, S=S, dist=A * S, mask=ref["mask"], n_contrib64=ref["n_contrib"], tiles=tiles, m=m)


def yardstick(buf, W, H, g, m=None):
    """Both passes.  g: (H, W) dL/dDist; it is zeroed at the masked pixels on this side (the caller zeroes it there too:
    blend_grad_reference.masked).  Returns pass one's dict plus one {"signed", "abs", "scale"} dict per OUTPUTS key."""
    r = moments_f64(buf, W, H, m)
    xy, co, pl, rg = _arrays(buf)
    m = r["m"]
    g = np.where(r["mask"], 0.0, _np(g, np.float64).reshape(H, W))
    A, mu, S = r["A"], r["mu"], r["S"]
    dpix = np.stack([g * (A * mu * mu + S), g * (-2.0 * A * mu), g * A], 2)
    colour = np.stack([np.ones_like(m), m, m * m], 1)
    ref = B.blend_grads_f64(xy, co[:, :3], co[:, 3], colour, m, pl, rg, np.zeros(3), W, H, dpix, forward_n_contrib=buf["n_contrib"])
    assert np.array_equal(ref["mask"], r["mask"])
    for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity"):
        r[k] = ref[k]
    c = ref["dL_dcolor"]
    r["dL_dinv_depths"] = {"signed": (c["signed"][:, 1] + 2.0 * m * c["signed"][:, 2])[:, None],
                           "abs": (c["abs"][:, 1] + 2.0 * np.abs(m) * c["abs"][:, 2])[:, None],
                           "scale": (c["scale"][:, 1] + 2.0 * np.abs(m) * c["scale"][:, 2])[:, None]}
    r["g"] = g
    return r


def _walk_f32(buf, W, H, tile, xs, ys, m32):
    """The header's weights of one tile, float32: yields per list position k (applied (P,) bool, alpha, G, dx, dy, id, conic')."""
    xy = _np(buf["points_xy_image"], f32).reshape(-1, 2)
    co = _np(buf["conic_opacity"], f32).reshape(-1, 4)
    pl = _np(buf["point_list"]).reshape(-1).astype(np.int64)
    s, e = (int(v) for v in _np(buf["ranges"]).reshape(-1, 2)[tile])
    nc = np.minimum(_np(buf["n_contrib"]).reshape(H, W)[ys, xs].astype(np.int64), e - s)
    idx = pl[s:e]
    px, py = xs.astype(f32), ys.astype(f32)
    a_, b_, c_ = f32(-0.5) * co[idx, 0], -co[idx, 1], f32(-0.5) * co[idx, 2]
    for k in range(int(nc.max()) if len(xs) else 0):
        i = idx[k]
        dx, dy = xy[i, 0] - px, xy[i, 1] - py
        power = (a_[k] * dx * dx + c_[k] * dy * dy) + b_[k] * dx * dy
        with np.errstate(under="ignore", over="ignore"):
            G = np.exp(power, dtype=f32)
            alpha = np.minimum(f32(0.99), co[i, 3] * G)
        applied = (k < nc) & ~(power > 0) & ~(alpha < f32(1.0 / 255.0))
        if applied.any():
            yield applied, alpha, G, dx, dy, int(i), (a_[k], b_[k], c_[k]), co[i, 3], m32[i]


def _tiles(buf, W, H):
    rg = _np(buf["ranges"]).reshape(-1, 2)
    gx = (W + 15) // 16
    for tile in range(rg.shape[0]):
        if rg[tile, 1] <= rg[tile, 0]:
            continue
        tx, ty = tile % gx, tile // gx
        ys, xs = np.meshgrid(np.arange(ty * 16, ty * 16 + 16), np.arange(tx * 16, tx * 16 + 16), indexing="ij")   # the whole tile
        yield tile, xs.ravel(), ys.ravel()


def forward_f32(buf, W, H, m=None, form="running"):
    """(dist, moments) float32 (H, W), (H, W, 4) by the header's forward; form="moments": Dist = A M2 - M1^2 (moments then holds
    A, M1, M2, 0)."""
    m32 = inv_depth(buf, f32) if m is None else np.asarray(m, f32)
    dist, mom = np.zeros((H, W), f32), np.zeros((H, W, 4), f32)
    for tile, xs, ys in _tiles(buf, W, H):
        inside = (xs < W) & (ys < H)
        xs_, ys_ = xs[inside], ys[inside]
        P = len(xs_)
        A, mu, S, T = np.zeros(P, f32), np.zeros(P, f32), np.zeros(P, f32), np.ones(P, f32)
        for applied, alpha, G, dx, dy, i, con, o, mk in _walk_f32(buf, W, H, tile, xs_, ys_, m32):
            w = alpha * T
            T = np.where(applied, T * (f32(1) - alpha), T)
            if form == "moments":
                A = np.where(applied, A + w, A)
                mu = np.where(applied, mu + w * mk, mu)                      # M1
                S = np.where(applied, S + (w * mk) * mk, S)                  # M2
                continue
            A1 = A + w
            d = mk - mu
            with np.errstate(divide="ignore", invalid="ignore"):
                r = w / A1
            S = np.where(applied, S + ((A * r) * d) * d, S)
            mu = np.where(applied, mu + r * d, mu)
            A = np.where(applied, A1, A)
        dist[ys_, xs_] = A * S - mu * mu if form == "moments" else A * S
        mom[ys_, xs_, 0], mom[ys_, xs_, 1], mom[ys_, xs_, 2] = A, mu, S
    return dist, mom


def backward_f32(buf, W, H, g, moments, m=None, drop_suffix=False):
    """(N, 16) float32 accumulator rows by the header's backward (only the seven columns it adds to are non-zero).  drop_suffix: a
    WRONG backward that forgets the suffix term of dL/dalpha (q = T u alone), for the test that shows the criterion sees it."""
    m32 = inv_depth(buf, f32) if m is None else np.asarray(m, f32)
    g32, mom = _np(g, f32).reshape(H, W), _np(moments, f32).reshape(H, W, 4)
    N = _np(buf["points_xy_image"]).reshape(-1, 2).shape[0]
    acc = np.zeros((N, 16), f32)
    half_w, half_h = f32(0.5) * f32(W), f32(0.5) * f32(H)
    for tile, xs, ys in _tiles(buf, W, H):
        for blk in range(4):                                             # the four 8x8 blocks, each with its 64 pixels in order
            sel = ((xs % 16) // 8 == blk % 2) & ((ys % 16) // 8 == blk // 2)
            bx, by = xs[sel], ys[sel]                                    # (row-major inside the block: q = (q & 7, q >> 3))
            inside = (bx < W) & (by < H)
            cx, cy = np.where(inside, bx, 0), np.where(inside, by, 0)
            A = np.where(inside, mom[cy, cx, 0], f32(0))
            mu = np.where(inside, mom[cy, cx, 1], f32(0))
            S = np.where(inside, mom[cy, cx, 2], f32(0))
            gg = np.where(inside, g32[cy, cx], f32(0))
            gA = gg * A
            total = f32(2) * (gA * S)
            Pfx, T = np.zeros(64, f32), np.ones(64, f32)
            # the walk wants in-image pixels only: n_contrib of the others is taken as 0 through `inside`
            for applied, alpha, G, dx, dy, i, con, o, mk in _walk_f32(buf, W, H, tile, cx, cy, m32):
                applied = applied & inside
                if not applied.any():
                    continue
                w = alpha * T
                d = mk - mu
                u = (((A * d) * d) + S) * gg
                Pfx = np.where(applied, Pfx + w * u, Pfx)
                R = total - Pfx
                om = f32(1) - alpha
                q = T * u if drop_suffix else T * u - R / om
                gd = G * q
                h = o * gd
                hx, hy = h * dx, h * dy
                vals = np.stack([hx, hy, hx * dx, hx * dy, hy * dy, gd, ((f32(2) * gA) * w) * d])
                vals = np.where(applied[None, :], vals, f32(0))
                T = np.where(applied, T * om, T)
                # (a float32 cumulative sum adds one term after the other: the ordered sum of each half)
                r = np.cumsum(vals[:, :32], axis=1, dtype=f32)[:, -1] + np.cumsum(vals[:, 32:], axis=1, dtype=f32)[:, -1]
                a_, b_, c_ = con
                acc[i, 3] += (f32(2) * a_ * r[0] + b_ * r[1]) * half_w
                acc[i, 4] += (f32(2) * c_ * r[1] + b_ * r[0]) * half_h
                acc[i, 6] += f32(-0.5) * r[2]
                acc[i, 7] += f32(-0.5) * r[3]
                acc[i, 9] += f32(-0.5) * r[4]
                acc[i, 10] += r[5]
                acc[i, 11] += r[6]
    return acc


def forward_error(dist, r):
    """max over the unmasked pixels of |dist - Dist| / (Dist (1 + mu / sigma)); inf if a pixel whose Dist is 0 is not 0."""
    got = _np(dist, np.float64).reshape(r["dist"].shape)
    keep = ~r["mask"]
    A, mu, S, D = r["A"][keep], r["mu"][keep], r["S"][keep], r["dist"][keep]
    d = np.abs(got[keep] - D)
    pos = D > 0
    if (d[~pos] != 0).any():
        return float("inf")
    if not pos.any():
        return 0.0
    kappa = np.abs(mu[pos]) / np.sqrt(S[pos] / A[pos])
    return float((d[pos] / (D[pos] * (1.0 + kappa))).max())


def layout(acc, key):
    """The (N, width) float64 array of accumulator rows (N, 16) that `key`'s sums are compared with."""
    return _np(acc, np.float64).reshape(-1, 16)[:, list(COLUMNS[key])]


def backward_errors(acc, r):
    """{key: worst per-Gaussian error in the key's scale} of accumulator rows (N, 16)."""
    return {k: B.worst(layout(acc, k), r[k]) for k in OUTPUTS}


def backward_error(acc, r):
    return max(backward_errors(acc, r).values())


def spread(a, b, r):
    """The worst difference of two runs' accumulator rows in the same units."""
    worst = 0.0
    for k in OUTPUTS:
        d, sc = np.abs(layout(a, k) - layout(b, k)), r[k]["scale"]
        sel = sc > 0
        if sel.any():
            worst = max(worst, float((d[sel] / sc[sel]).max()))
    return worst


def criterion(E_kernel, E_f32, E_spread, floor):
    return E_kernel <= 3.0 * max(E_f32, E_spread) + floor


def draw_g(H, W, seed=7):
    """dL/dDist from U(0.5, 1.5) / (W H): positive, as a loss weight's gradient is, and uneven, so that a swapped pixel shows."""
    return (np.random.default_rng(seed).uniform(0.5, 1.5, (H, W)) / (W * H)).astype(f32)
