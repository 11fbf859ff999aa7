"""
The float32 restatement of csrc/frame_walk.h, written once: the list walk (FrameWalk and blend_forward_weight), the 8x8 blocks in
wave and lane order, the ordered block sum and the value-tile flush (ValueTile), and the helpers the stages' results are judged with.

Test helper, not a test file.  The stage modules (features_reference, distortion_reference, normal_render_reference,
plane_depth_reference, and median_depth_reference for the tiles) keep what is theirs -- their yardsticks, their values per entry --
and take everything else from here.  Every function works on one frame shape, a frame_walk_frames-style dict (W H N D xy co invd
point_list ranges n_contrib), whether it came from a forward's buffers (frame_of_buffers) or from frame_walk_frames.build_frame.
Nothing here is taken from float64: it replays the header on the same arrays, step by step.
"""
import json
import os

import numpy as np

import blend_grad_reference as B

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
_LD = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64


def to_np(a, dtype=None):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return a if dtype is None else a.astype(dtype)


def fma32(a, b, c):
    """fma(a, b, c) in float32: the exact product and the sum in extended precision, rounded once to float32 (x87 long double where
    numpy has it: 64 bits hold the 48-bit product exactly, and the second rounding then changes a result only with probability
    2^-40 per operation)."""
    return (np.asarray(a, f32).astype(_LD) * np.asarray(b, f32).astype(_LD) + np.asarray(c, f32).astype(_LD)).astype(f32)


# ---- frames ----
def inv_depth(buf, dtype=np.float64):
    d = to_np(buf["depths"], dtype).reshape(-1)
    return np.where(d > 0, dtype(1) / np.where(d > 0, d, dtype(1)), dtype(0)).astype(dtype)


def arrays(buf):
    """(xy (N, 2), conic_opacity (N, 4)) float64, point_list, ranges of a forward's buffers: what the float64 yardsticks read."""
    return (to_np(buf["points_xy_image"], np.float64).reshape(-1, 2), to_np(buf["conic_opacity"], np.float64).reshape(-1, 4),
            to_np(buf["point_list"]).reshape(-1), to_np(buf["ranges"]).reshape(-1, 2))


def frame_of_buffers(buf, W, H, invd=None):
    """A frame_walk_frames dict over a forward's buffers (numpy or torch).  invd: the (N,) float32 inverse depths the kernel reads;
    None: 1 / depths of the buffers."""
    pl = to_np(buf["point_list"]).reshape(-1)
    xy = to_np(buf["points_xy_image"], f32).reshape(-1, 2)
    invd = (inv_depth(buf, f32) if "depths" in buf else None) if invd is None else to_np(invd, f32).reshape(-1)
    return dict(W=W, H=H, N=xy.shape[0], D=int(pl.shape[0]), xy=xy, co=to_np(buf["conic_opacity"], f32).reshape(-1, 4), invd=invd,
                point_list=pl, ranges=to_np(buf["ranges"]).reshape(-1, 2), n_contrib=to_np(buf["n_contrib"]).reshape(H, W))


def tile_range(fr, tile):
    """The tile's range clipped to [0, D], as FrameWalk's constructor clips it."""
    s, e = fr["ranges"][tile]
    return min(max(int(s), 0), fr["D"]), min(max(int(e), 0), fr["D"])


def tile_grid(W, tile):
    """(xs, ys) of the whole 16x16 tile, row-major, off-image pixels included."""
    gx = (W + 15) // 16
    tx, ty = tile % gx, tile // gx
    ys, xs = np.meshgrid(np.arange(ty * 16, ty * 16 + 16), np.arange(tx * 16, tx * 16 + 16), indexing="ij")
    return xs.ravel(), ys.ravel()


def tiles(fr):
    """(tile, s, e, xs, ys) of every tile whose clipped range is not empty."""
    for tile in range(len(fr["ranges"])):
        s, e = tile_range(fr, tile)
        if e > s:
            yield (tile, s, e) + tile_grid(fr["W"], tile)


def blocks(xs, ys, W, H):
    """(bx, by, inside) of a tile's four 8x8 blocks in wave order, each with its 64 pixels in lane order (row-major inside the
    block: q = (q & 7, q >> 3)); inside: the lanes on the image."""
    for blk in range(4):
        sel = ((xs % 16) // 8 == blk % 2) & ((ys % 16) // 8 == blk // 2)
        bx, by = xs[sel], ys[sel]
        yield bx, by, (bx < W) & (by < H)


def block_values(image, bx, by, inside):
    """image (H, W[, C]) at a block's lanes, off-image lanes as zeros."""
    v = image[np.where(inside, by, 0), np.where(inside, bx, 0)]
    return np.where(inside.reshape((-1,) + (1,) * (v.ndim - 1)), v, image.dtype.type(0))


# ---- the walk ----
def walk_f32(fr, s, e, xs, ys, inside):
    """The one float32 walk: the list [s, e) (already clipped, see tiles) at the pixels (xs, ys), n_contrib clipped to the range and
    taken as 0 where not `inside`, ids outside [0, N) skipped.  Per list position that some pixel applies it yields
        applied (P,) bool, alpha, G, dx, dy, id, conic' (a', b', c'), opacity, k (the position, 0-based within the range).
    The expressions and their order are blend_forward_weight's in csrc/frame_walk.h (the comment there says that the restatements
    under tests/ replay its lines: this is where): the pre-scaled conic, power, G = exp(power), alpha = min(0.99, o G), and the two
    skip tests, power > 0 and alpha < 1/255."""
    xy, co = fr["xy"], fr["co"]
    idx = fr["point_list"][s:e].astype(np.int64)
    nc = np.where(inside, np.clip(fr["n_contrib"][np.where(inside, ys, 0), np.where(inside, xs, 0)].astype(np.int64), 0, e - s), 0)
    px, py = xs.astype(f32), ys.astype(f32)
    for k in range(int(nc.max()) if len(xs) else 0):
        i = int(idx[k])
        if i < 0 or i >= fr["N"]:
            continue
        a_, b_, c_ = f32(-0.5) * co[i, 0], -co[i, 1], f32(-0.5) * co[i, 2]
        dx, dy = xy[i, 0] - px, xy[i, 1] - py
        power = (a_ * dx * dx + c_ * dy * dy) + b_ * dx * dy
        with np.errstate(under="ignore", over="ignore"):
            G = np.exp(power, dtype=f32)
            alpha = np.minimum(f32(0.99), co[i, 3] * G)
        applied = (k < nc) & ~(power > 0) & ~(alpha < f32(1.0 / 255.0))
        if applied.any():
            yield applied, alpha, G, dx, dy, i, (a_, b_, c_), co[i, 3], k


def weights_f32(fr, tile_range, xs, ys):
    """(P, L) float32 weights w = alpha T of one tile's list at the in-image pixels (xs, ys), dense: zero where not applied."""
    s, e = tile_range
    w, T = np.zeros((len(xs), e - s), f32), np.ones(len(xs), f32)
    for applied, alpha, *_, k in walk_f32(fr, s, e, xs, ys, np.ones(len(xs), bool)):
        w[:, k] = np.where(applied, alpha * T, f32(0))
        T = np.where(applied, T * (f32(1) - alpha), T)
    return w


# ---- the backward's body: ValueTile ----
def ordered_block_sum(vals):
    """(..., 64) float32 -> (...): pixels 0-31 in order, pixels 32-63 in order, then the two halves (a float32 cumulative sum adds one
    term after the other: the ordered sum of each half)."""
    return np.cumsum(vals[..., :32], axis=-1, dtype=f32)[..., -1] + np.cumsum(vals[..., 32:], axis=-1, dtype=f32)[..., -1]


def backward_block(fr, s, e, bx, by, inside, total, entry, acc, drop_suffix=False):
    """One 8x8 block's share of a stage's backward.  total (64,): the block's pixels' sum of w u over the whole list; entry(i, dx, dy,
    w) -> (u (64,), tail: a sequence of (64,) values past the sixth), called per applied list entry in list order.  dL/dalpha is
    total-minus-prefix: Pfx += w u, R = total - Pfx, q = T u - R / (1 - alpha); drop_suffix: a WRONG q = T u alone, for the tests that
    show the criterion sees it.  The six base values' ordered block sums are added to columns 3, 4, 6, 7, 9 and 10 of acc (N, 16);
    the tail's sums come back as [(id, (len(tail),) float32)] in list order."""
    half_w, half_h = f32(0.5) * f32(fr["W"]), f32(0.5) * f32(fr["H"])
    Pfx, T = np.zeros(len(bx), f32), np.ones(len(bx), f32)
    tails = []
    for applied, alpha, G, dx, dy, i, (a_, b_, c_), o, _ in walk_f32(fr, s, e, bx, by, inside):
        with np.errstate(all="ignore"):
            w = alpha * T
            u, tail = entry(i, dx, dy, w)
            Pfx = np.where(applied, Pfx + w * u, Pfx)
            R = total - Pfx
            om = f32(1) - alpha
            q = T * u if drop_suffix else T * u - R / om
            gd = G * q
            h = o * gd
            hx, hy = h * dx, h * dy
            vals = np.stack([hx, hy, hx * dx, hx * dy, hy * dy, gd, *tail])
        r = ordered_block_sum(np.where(applied[None, :], vals, f32(0)))
        T = np.where(applied, T * om, T)
        acc[i, 3] += (f32(2) * a_ * r[0] + b_ * r[1]) * half_w
        acc[i, 4] += (f32(2) * c_ * r[1] + b_ * r[0]) * half_h
        acc[i, 6] += f32(-0.5) * r[2]
        acc[i, 7] += f32(-0.5) * r[3]
        acc[i, 9] += f32(-0.5) * r[4]
        acc[i, 10] += r[5]
        tails.append((i, r[6:]))
    return tails


# ---- judging ----
def golden(name):
    """tests/golden/<name>.json."""
    with open(os.path.join(GOLDEN_DIR, name + ".json")) as f:
        return json.load(f)


def layout(acc, key, columns, extra=None):
    """The (N, width) float64 array that `key`'s sums are compared with: columns[key] of the accumulator rows (N, 16), or the
    stage's extra per-Gaussian array for the key that has no columns."""
    rows = to_np(acc, np.float64).reshape(-1, 16)
    return rows[:, list(columns[key])] if key in columns else to_np(extra, np.float64).reshape(len(rows), -1)


def backward_errors(acc, r, outputs, columns, extra=None):
    """{key: worst per-Gaussian error in the key's scale}."""
    return {k: B.worst(layout(acc, k, columns, extra), r[k]) for k in outputs}


def spread(a, b, r, outputs, columns):
    """The worst difference of two runs' (acc[, extra]) in the same units."""
    worst = 0.0
    for k in outputs:
        d, sc = np.abs(layout(a[0], k, columns, *a[1:]) - layout(b[0], k, columns, *b[1:])), r[k]["scale"]
        sel = sc > 0
        if sel.any():
            worst = max(worst, float((d[sel] / sc[sel]).max()))
    return worst


def criterion(E_kernel, E_f32, E_spread, floor):
    return E_kernel <= 3.0 * max(E_f32, E_spread) + floor


def rows_error(got, want, scale, keep=None):
    """Worst |got - want| / scale over the kept rows; a component whose scale is 0 must be exactly 0 (inf otherwise)."""
    got, want = to_np(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d != 0, np.inf, 0.0))
    if keep is not None:
        e = e[keep]
    return float(e.max()) if e.size else 0.0
