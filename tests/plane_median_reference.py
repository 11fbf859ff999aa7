"""
The plane depth under the median rule (include/gsr_plane_median.h): a float32 restatement of the forward and of the backward's
addends, and a float64 yardstick of the moments.

Test helper, not a test file.  Nothing of the walk is written here: the applied entries, their alphas and T are
frame_walk_reference.walk_f32's (blend_forward_weight's lines), the entry's m and its clamp are plane_depth_reference._m32's, and the
frames, their float64 contributor images and their tie masks are median_depth_reference's, all nine of them.

  forward_f32   per pixel, over the applied entries in list order:  if T > 0.5: med = m, c = pos;  T <- T (1 - alpha).  numpy's exp
                and the hardware's differ in their last bit, so at a pixel inside median_depth_reference's tie mask this walk (like any
                other evaluation) may lawfully choose the neighbouring entry; chosen(), which evaluates m at a GIVEN contributor image,
                has no exp in it and replays the kernel bit for bit at every pixel.
  chosen        the backward's first half: the contributor clipped to the tile's clipped range, the id to [0, N), dx and dy as the
                forward forms them, m and the clamp decision.
  addends_f32   (g, g (-dx), g (-dy)) per pixel in float32, zeros where clamped or nothing was chosen.
  moments_f64   the float64 sums of the same addends per Gaussian -- the clamp decision taken from the float32 values, as
                gsr_plane_depth.h takes its branches -- with the sum of their magnitudes and their count n per row, the terms of the
                header's bound (n + 2) 2^-24 sum |addend|.

Frames may carry float64 xy (the chain test's exact projections): the float32 side casts them down, the float64 side reads them as
they are.
"""
import numpy as np

import frame_walk_reference as FWR
import median_depth_reference as M
import plane_depth_reference as PD

f32 = np.float32
U24 = 2.0 ** -24
MIN_CLAMPED, MIN_FREE = 2, 10        # per case, among the chosen entries: what case() asserts
_CASES = {}


def golden():
    """tests/golden/plane_median_margins.json: "closed_form_rel" (CPU: the restatement's worst relative error against the analytic
    plane on plane_depth_reference.sheet()), "chosen" per frame (CPU: clamped / free-with-slopes / all chosen entries), "backward_ratio"
    per frame (what an MI355X run measured: the worst error over the header's bound, a record only) and "mesh_gap_min" (null: no
    threshold on the torus rows, README "Plane depth under the median rule")."""
    return FWR.golden("plane_median_margins")


def draw_slopes(fr):
    """(N, 2) float32: slopes of the size of the inverse depths over a few pixels -- steep enough that some chosen entries meet the
    clamp inside a tile -- and a fifth of the Gaussians on the fallback branch, (0, 0) exactly."""
    rng = np.random.default_rng(3)
    slopes = (rng.normal(0, 0.15, (fr["N"], 2)) * fr["invd"][:, None]).astype(f32)
    slopes[rng.random(fr["N"]) < 0.2] = 0
    return slopes


def _f32_frame(fr):
    return fr if fr["xy"].dtype == f32 else dict(fr, xy=fr["xy"].astype(f32))


def forward_f32(fr, slopes):
    """(med (H, W) float32, contrib (H, W) int64, clamped (H, W) bool) by the header's forward."""
    fr = _f32_frame(fr)
    W, H = fr["W"], fr["H"]
    sl = FWR.to_np(slopes, f32).reshape(-1, 2)
    med, contrib, clamped = np.zeros((H, W), f32), np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        inside = (xs < W) & (ys < H)
        xs_, ys_ = xs[inside], ys[inside]
        T, m_p = np.ones(len(xs_), f32), np.zeros(len(xs_), f32)
        c_p, cl_p = np.zeros(len(xs_), np.int64), np.zeros(len(xs_), bool)
        for applied, alpha, G, dx, dy, i, _, _, k in FWR.walk_f32(fr, s, e, xs_, ys_, np.ones(len(xs_), bool)):
            m, cl = PD._m32(fr, sl, i, dx, dy)
            take = applied & (T > f32(0.5))
            m_p, c_p, cl_p = np.where(take, m, m_p), np.where(take, k + 1, c_p), np.where(take, cl, cl_p)
            T = np.where(applied, T * (f32(1) - alpha), T)
        med[ys_, xs_], contrib[ys_, xs_], clamped[ys_, xs_] = m_p, c_p, cl_p
    return med, contrib, clamped


def chosen(fr, slopes, contrib):
    """dict: ids (H, W) int64 (-1 where the pixel chose nothing: contrib clipped to the tile's clipped range is 0, or the id lies outside
    [0, N)), dx, dy, m (H, W) float32 and clamped (H, W) bool, all zero / False where ids is -1."""
    fr32 = _f32_frame(fr)
    W, H, N = fr["W"], fr["H"], fr["N"]
    sl = FWR.to_np(slopes, f32).reshape(-1, 2)
    gx = (W + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * gx + xs // 16
    lo = np.array([FWR.tile_range(fr, t) for t in range(len(fr["ranges"]))], np.int64).reshape(-1, 2)
    start, length = lo[tile, 0], np.maximum(lo[tile, 1] - lo[tile, 0], 0)
    c = np.clip(FWR.to_np(contrib).astype(np.int64).reshape(H, W), 0, length)
    at = np.where(c > 0, start + c - 1, 0)
    ids = np.where(c > 0, fr["point_list"].astype(np.int64)[at] if fr["D"] else -1, -1)
    ids = np.where((ids >= 0) & (ids < N), ids, -1)
    has = ids >= 0
    safe = np.where(has, ids, 0)
    dx = np.where(has, fr32["xy"][safe, 0] - xs.astype(f32), f32(0)).astype(f32)
    dy = np.where(has, fr32["xy"][safe, 1] - ys.astype(f32), f32(0)).astype(f32)
    invd = fr["invd"][safe]
    mr = PD.fma32(-sl[safe, 0], dx, PD.fma32(-sl[safe, 1], dy, invd))
    m = np.minimum(np.maximum(mr, invd * f32(0.25)), invd * PD.MAX_RATIO)
    return dict(ids=ids, dx=dx, dy=dy, m=np.where(has, m, f32(0)).astype(f32), clamped=has & (m != mr), c=c)


def addends_f32(fr, slopes, g, contrib, ch=None):
    """(ids (H, W), addends (H, W, 3) float32): what each pixel holds when the wave starts to sum."""
    ch = chosen(fr, slopes, contrib) if ch is None else ch
    g32 = FWR.to_np(g, f32).reshape(fr["H"], fr["W"])
    live = (ch["ids"] >= 0) & ~ch["clamped"]
    v = np.stack([g32, g32 * (-ch["dx"]), g32 * (-ch["dy"])], 2)
    return ch["ids"], np.where(live[:, :, None], v, f32(0)).astype(f32)


def moments_f64(fr, slopes, g, contrib, ch=None):
    """dict: signed (N, 3), abs (N, 3) float64 and count (N,) int64 -- per Gaussian the sum of (g, g (p.x - x_k), g (p.y - y_k)) over
    the pixels that chose it with an unclamped entry, the sum of the addends' magnitudes, and how many addends there are."""
    ch = chosen(fr, slopes, contrib) if ch is None else ch
    H, W, N = fr["H"], fr["W"], fr["N"]
    g64 = FWR.to_np(g, np.float64).reshape(H, W)
    live = (ch["ids"] >= 0) & ~ch["clamped"]
    ys, xs = np.nonzero(live)
    ids = ch["ids"][live]
    xy = fr["xy"].astype(np.float64)
    gg = g64[live]
    v = np.stack([gg, gg * (xs - xy[ids, 0]), gg * (ys - xy[ids, 1])], 1)
    signed, mag, count = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N, np.int64)
    np.add.at(signed, ids, v)
    np.add.at(mag, ids, np.abs(v))
    np.add.at(count, ids, 1)
    return dict(signed=signed, abs=mag, count=count)


def bound_ratio(got, r):
    """Worst |got - signed| / ((n + 2) 2^-24 sum |addend|) over the elements of the moments; a row without addends must be exactly 0
    (inf otherwise)."""
    got = FWR.to_np(got, np.float64).reshape(-1, 3)
    d = np.abs(got - r["signed"])
    bound = (r["count"][:, None] + 2) * U24 * r["abs"]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d != 0, np.inf, 0.0))
    return float(e.max()) if e.size else 0.0


def case(name):
    """dict of one of median_depth_reference.CASES with its case masks: fr, ref (median_f64), slopes, med / contrib / clamped (the
    restatement), ch (chosen() at the restatement's contributors), counts.  Built once; asserts that the frame still holds what the
    tests are there for."""
    if name not in _CASES:
        fr, ref = M.frame(name)
        slopes = draw_slopes(fr)
        med, contrib, clamped = forward_f32(fr, slopes)
        ch = chosen(fr, slopes, contrib)
        sel = contrib > 0
        free = sel & ~clamped & (slopes[np.where(sel, ch["ids"], 0)] != 0).any(2)
        counts = dict(clamped=int((sel & clamped).sum()), free_with_slopes=int(free.sum()), chosen=int(sel.sum()))
        assert counts["clamped"] >= MIN_CLAMPED and counts["free_with_slopes"] >= MIN_FREE, (name, counts)
        _CASES[name] = dict(fr=fr, ref=ref, slopes=slopes, med=med, contrib=contrib, clamped=clamped, ch=ch, counts=counts)
    return _CASES[name]


def with_masks(c, masks):
    """The case's frame with other mask bytes (None, "ff", "random": median_depth_reference.frame's)."""
    return M.frame([k for k, v in _CASES.items() if v is c][0], masks=masks)[0]
