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

The float32 restatement (numpy) takes nothing from float64: it replays the header on the same buffers, step by step -- the weights of
frame_walk_reference.walk_f32, the running A, mu, S of the forward, and frame_walk_reference.backward_block (the total-minus-prefix
walk and the block sums in the header's order) with this stage's u, total and column-11 value -- and adds the
seven columns per (block, entry) to a float32 (N, 16) array of accumulator rows in tile, block and list order.  form="moments" is
the forward by A M2 - M1^2 instead, which the thin-slab test must see fail.

Errors.  Forward: max over the unmasked pixels of |dist - Dist| / (Dist (1 + mu / sigma)), sigma^2 = S / A -- relative, in units
of 1 + kappa; divided by eps32 it is the "eps32 mu / sigma" figure.  A pixel whose Dist is exactly 0 (one contributor, equal
depths) must be exactly 0.  Backward: blend_grad_reference.errors per output, in its scale.
"""
import numpy as np

import blend_grad_reference as B
import frame_walk_reference as FWR

f32 = np.float32
EPS32 = FWR.EPS32
_np, inv_depth, criterion = FWR.to_np, FWR.inv_depth, FWR.criterion
OUTPUTS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dinv_depths")
COLUMNS = {"dL_dmean2D": (3, 4), "dL_dconic": (6, 7, 8, 9), "dL_dopacity": (10,), "dL_dinv_depths": (11,)}
TOUCHED = (3, 4, 6, 7, 9, 10, 11)
UNTOUCHED = (0, 1, 2, 5, 8, 12, 13, 14, 15)


def golden():
    """tests/golden/distortion_margins.json: "floor" {"forward", "backward"}, the smallest float32-restatement errors of the CPU
    matrix; "thin_slab_bound", the restatement's bound on a thin slab in eps32 mu / sigma; "E_kernel", what an MI355X run measured
    per frame (tools/record_distortion_margins.py)."""
    return FWR.golden("distortion_margins")


def moments_f64(buf, W, H, m=None):
    """Pass one.  Returns dict: A, mu, S, dist (H, W) float64, mask (H, W) bool, n_contrib64, tiles (tile, xs, ys, idx, w, masked, active)."""
    xy, co, pl, rg = FWR.arrays(buf)
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
    xy, co, pl, rg = FWR.arrays(buf)
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


def forward_f32(buf, W, H, m=None, form="running"):
    """(dist, moments) float32 (H, W), (H, W, 4) by the header's forward; form="moments": Dist = A M2 - M1^2 (moments then holds
    A, M1, M2, 0)."""
    fr = FWR.frame_of_buffers(buf, W, H, m)
    dist, mom = np.zeros((H, W), f32), np.zeros((H, W, 4), f32)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        inside = (xs < W) & (ys < H)
        xs_, ys_ = xs[inside], ys[inside]
        P = len(xs_)
        A, mu, S, T = np.zeros(P, f32), np.zeros(P, f32), np.zeros(P, f32), np.ones(P, f32)
        for applied, alpha, G, dx, dy, i, *_ in FWR.walk_f32(fr, s, e, xs_, ys_, np.ones(P, bool)):
            mk = fr["invd"][i]
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
    fr = FWR.frame_of_buffers(buf, W, H, m)
    g32, mom = _np(g, f32).reshape(H, W), _np(moments, f32).reshape(H, W, 4)
    acc = np.zeros((fr["N"], 16), f32)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        for bx, by, inside in FWR.blocks(xs, ys, W, H):
            A, mu, S, _ = FWR.block_values(mom, bx, by, inside).T
            gg = FWR.block_values(g32, bx, by, inside)
            gA = gg * A

            def entry(i, dx, dy, w):
                d = fr["invd"][i] - mu
                return (((A * d) * d) + S) * gg, (((f32(2) * gA) * w) * d,)

            for i, tail in FWR.backward_block(fr, s, e, bx, by, inside, f32(2) * (gA * S), entry, acc, drop_suffix):
                acc[i, 11] += tail[0]
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
    return FWR.layout(acc, key, COLUMNS)


def backward_errors(acc, r):
    """{key: worst per-Gaussian error in the key's scale} of accumulator rows (N, 16)."""
    return FWR.backward_errors(acc, r, OUTPUTS, COLUMNS)


def backward_error(acc, r):
    return max(backward_errors(acc, r).values())


def spread(a, b, r):
    """The worst difference of two runs' accumulator rows in the same units."""
    return FWR.spread((a,), (b,), r, OUTPUTS, COLUMNS)


def draw_g(H, W, seed=7):
    """dL/dDist from U(0.5, 1.5) / (W H): positive, as a loss weight's gradient is, and uneven, so that a swapped pixel shows."""
    return (np.random.default_rng(seed).uniform(0.5, 1.5, (H, W)) / (W * H)).astype(f32)
