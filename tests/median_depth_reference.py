"""
Float64 statement of the median inverse depth (include/gsr_median_depth.h) and of its gradient, and the frames it is held on.

Test helper, not a test file.  The weights are those of blend_grad_reference.blend_grads_f64 and features_reference.weights_f32 -- the
power expression with the pre-scaled conic, alpha = min(0.99, o exp(power)), the two skip tests, T <- T (1 - alpha) -- evaluated in
float64 on the frame's float32 arrays, dense per tile (pixels x entries), and bounded like the kernels' walk: by the frame's own
n_contrib, with ids outside [0, N) skipped.  (blend_grads_f64 itself decides its own n_contrib and indexes with every id, so it cannot
take these frames; the expressions are its.)  Per pixel, with T_k the transmittance BEFORE applied entry k:

    c   = the 1-based list position of the last applied entry with T_k > 0.5      (0 without an applied entry)
    med = inv_depth[id of that entry]                                            (the float32 value; 0 where c = 0)

which is the header's loop, T being non-increasing.  The gradient of sum_p g[p] med[p] with respect to inv_depth is the scatter-add of
g[p] to the chosen ids; its unit per Gaussian is the sum of |g[p]| (blend_grad_reference.errors' `scale`).

Tie mask: true where any prefix transmittance (T behind an applied entry) lies within a relative TIE = 2e-4 of 0.5.  The float32 walk
with the hardware exp may lawfully choose the neighbouring entry there: T is a product of up to 640 rounded factors, each off by
about eps32 plus the exp's 5e-7, so k eps32 = 4e-5 at k = 640 and the band is about five times that.  A pixel in the band is excused
from the contributor and value comparison, and from nothing else.

Frames: frame_walk_frames.build_frame (each Gaussian once per tile, so that a list position is one Gaussian in every tile) with the
opacities -- and for a few "wall" Gaussians the position and conic -- rewritten by list position, n_contrib topped up to the whole
list at some pixels, and out-of-range ids put where the median would have been.

Masks.  block_masks are the forward blend's: a bit may be clear only where no pixel of that 8x4 block applies the entry.  Bytes drawn
at random do not keep that promise (a wave would pass over entries its pixels apply, and the result would rightly differ), so the
"random" masks here are random bytes OR the bits the promise needs: `need`, per list entry, the blocks in which some pixel's float64
alpha reaches HALF the 1/255 threshold within its n_contrib -- looser than `applied`, so that a float32 decision at the threshold
cannot fall outside it.
"""
import numpy as np

import frame_walk_frames as FW
import frame_walk_reference as FWR

TIE = 2e-4
MAX_TIES = 0.01              # the largest share of a frame's pixels the tie mask may cover
ALPHA_MIN = float(np.float32(1.0 / 255.0))
NEVER = 0.003                # an opacity no pixel applies: alpha <= 0.003 < 1 / 255
N_GAUSS = 700


def golden():
    """tests/golden/median_depth_margins.json: "tie_share" per frame (CPU, from the reference alone), "E_backward" per frame, what an
    MI355X run measured (tools/record_median_depth_margins.py), and "mesh_gap_min" (null until every README row shows a gap)."""
    return FWR.golden("median_depth_margins")


def median_f64(fr, n_contrib=None):
    """fr: a frame dict (numpy).  Returns dict: contrib (H, W) int64, ids (H, W) int64 (-1 where contrib is 0), med (H, W) float32,
    tie (H, W) bool, T_final (H, W) float64, applied (H, W) int64 (entries applied), power_skips (entries left out for power > 0), need (D,) uint8 (the mask bits, see above)."""
    W, H, N = fr["W"], fr["H"], fr["N"]
    xy, co, invd = fr["xy"].astype(np.float64), fr["co"].astype(np.float64), fr["invd"]
    pl = fr["point_list"].astype(np.int64)
    nc_all = fr["n_contrib"] if n_contrib is None else n_contrib
    contrib, ids = np.zeros((H, W), np.int64), np.full((H, W), -1, np.int64)
    med, tie = np.zeros((H, W), np.float32), np.zeros((H, W), bool)
    T_final, applied_n = np.ones((H, W)), np.zeros((H, W), np.int64)
    power_skips = 0
    need = np.zeros(fr["D"], np.uint8)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        on_image = (xs < W) & (ys < H)
        xs, ys = xs[on_image], ys[on_image]
        idx = pl[s:e]
        L = len(idx)
        valid = (idx >= 0) & (idx < N)
        safe = np.where(valid, idx, 0)
        nc = np.clip(nc_all[ys, xs].astype(np.int64), 0, L)
        dx = xy[safe, 0][None, :] - xs.astype(np.float64)[:, None]
        dy = xy[safe, 1][None, :] - ys.astype(np.float64)[:, None]
        a_, b_, c_ = -0.5 * co[safe, 0][None, :], -co[safe, 1][None, :], -0.5 * co[safe, 2][None, :]
        power = (a_ * dx * dx + c_ * dy * dy) + b_ * dx * dy
        with np.errstate(over="ignore", under="ignore"):
            alpha = np.minimum(0.99, co[safe, 3][None, :] * np.exp(power))
        pos = np.arange(L)[None, :]
        walked = valid[None, :] & (pos < nc[:, None])
        power_skips += int((walked & (power > 0)).sum())
        keep = walked & ~(power > 0) & ~(alpha < ALPHA_MIN)
        one_minus = np.where(keep, 1.0 - alpha, 1.0)
        T_out = np.cumprod(one_minus, 1)
        T_in = np.concatenate([np.ones((len(xs), 1)), T_out[:, :-1]], 1)
        chosen = keep & (T_in > 0.5)
        c = np.where(chosen, pos + 1, 0).max(1)
        contrib[ys, xs] = c
        cid = np.where(c > 0, idx[np.maximum(c, 1) - 1], -1)
        ids[ys, xs] = cid
        med[ys, xs] = np.where(c > 0, invd[np.maximum(cid, 0)], np.float32(0))
        tie[ys, xs] = (keep & (np.abs(T_out / 0.5 - 1.0) < TIE)).any(1)
        T_final[ys, xs] = T_out[:, -1]
        bit = ((ys % 16) // 4) * 2 + (xs % 16) // 8                   # the forward's 8x4 blocks (blend_fwd.hip)
        reach = walked & ~(alpha < 0.5 * ALPHA_MIN)
        for k in range(8):
            need[s:e] |= (reach[bit == k].any(0).astype(np.uint8) << k) if (bit == k).any() else 0
        applied_n[ys, xs] = keep.sum(1)
    return dict(contrib=contrib, ids=ids, med=med, tie=tie, T_final=T_final, applied=applied_n, power_skips=power_skips, need=need)


def gradient_f64(fr, ref, g):
    """(signed (N,), scale (N,)) float64: the scatter-add of g[p] (and of |g[p]|) to the Gaussian each pixel chose."""
    g = np.asarray(g, np.float64).reshape(fr["H"], fr["W"])
    sel = ref["contrib"] > 0
    signed, scale = np.zeros(fr["N"]), np.zeros(fr["N"])
    np.add.at(signed, ref["ids"][sel], g[sel])
    np.add.at(scale, ref["ids"][sel], np.abs(g[sel]))
    return signed, scale


def gradient_error(col11, signed, scale):
    """Worst per-Gaussian |col11 - signed| / scale; a Gaussian whose scale is 0 must be exactly 0 (inf otherwise)."""
    got = np.asarray(col11, np.float64).reshape(-1)
    d = np.abs(got - signed)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(got != 0, np.inf, 0.0))
    return float(e.max()) if e.size else 0.0


def draw_g(H, W, seed=5):
    """dL/d(med): signed and uneven, so that a swapped pixel and a lost sign both show."""
    return np.random.default_rng(seed).normal(0, 1, (H, W)).astype(np.float32)


# ---- the frames ----
def _positions(fr):
    """Gaussian id by 0-based list position: once_per_tile frames list prefixes of one permutation."""
    t = int(np.argmax(fr["tile_len"]))
    return fr["point_list"][fr["starts"][t]:fr["starts"][t] + fr["tile_len"][t]].astype(np.int64)


def _wall(fr, rng, gid, opacity, sigma):
    """Make Gaussian `gid` a broad blob somewhere on the image: its alpha varies smoothly over every tile."""
    fr["xy"][gid] = (rng.uniform(0, fr["W"]), rng.uniform(0, fr["H"]))
    fr["co"][gid] = (1.0 / sigma ** 2, 0.0, 1.0 / sigma ** 2, opacity)


def _full_lists(fr, rng, share):
    """n_contrib = the whole list at `share` of each tile's pixels (build_frame's once_per_tile keeps n_contrib short of the end)."""
    for tile, ln in enumerate(fr["tile_len"]):
        xs, ys = FWR.tile_grid(fr["W"], tile)
        on_image = (xs < fr["W"]) & (ys < fr["H"])
        xs, ys = xs[on_image], ys[on_image]
        sel = rng.random(len(xs)) < share
        fr["n_contrib"][ys[sel], xs[sel]] = ln


# what each case does to the opacities, by 0-based list position k (1-based position k + 1)
def _first(fr, rng, pos):                   # (a) every pixel with n_contrib >= 1 crosses at entry 1
    _wall(fr, rng, pos[0], 0.95, 200.0)


def _spread(fr, rng, pos):                  # (b) crossings spread over the first batch
    fr["co"][:, 3] *= 0.35


def _edge(fr, rng, pos):                    # (c) crossings at positions 255, 256, 257, 258: the staging batch's edge
    fr["co"][pos[:254], 3] = NEVER
    for k, o in zip(range(254, min(257, len(pos))), (0.7, 0.6, 0.6)):       # three blobs a third of the image wide, then one over all of it
        _wall(fr, rng, pos[k], o, 0.3 * max(fr["W"], fr["H"]))
    if len(pos) > 257:
        _wall(fr, rng, pos[257], 0.95, 200.0)


def _third(fr, rng, pos):                   # (d) crossings in the third batch
    fr["co"][pos[:520], 3] = NEVER
    fr["co"][pos[520:], 3] *= 0.5


def _never(fr, rng, pos):                   # (e) T never reaches one half: the last applied entry wins
    fr["co"][:, 3] = 0.0045                 # applied only where exp(power) >= 0.871: a few entries per pixel


CASES = {
    # name: (W, H, lens, seed, shaping, the masks of frame(name), record_view)
    "first_64x48": (64, 48, FW.LENS, 11, _first, "random", False),
    "spread_64x48": (64, 48, FW.LENS, 12, _spread, "random", True),
    "spread_50x37": (50, 37, FW.LENS, 13, _spread, None, False),
    "edge_64x48": (64, 48, FW.LENS, 14, _edge, "random", False),
    "edge_16x8": (16, 8, (640,), 15, _edge, "ff", True),
    "third_50x37": (50, 37, FW.LENS, 16, _third, "random", True),
    "third_8x8": (8, 8, (640,), 17, _third, None, False),
    "never_64x48": (64, 48, FW.LENS, 18, _never, "random", False),
    "never_8x8": (8, 8, (640,), 19, _never, "ff", True),
}
BATCH_EDGE_CASES = ("edge_64x48", "edge_16x8", "third_50x37", "third_8x8")     # (c) and (d): what the early exit must not cut
_BUILT = {}


def frame(name, masks="case"):
    """(fr, ref): the frame of CASES[name] and median_f64 of it, built once.  masks: "case", or None / "ff" / "random" for the same
    frame with other mask bytes (the reference does not read them)."""
    if name not in _BUILT:
        W, H, lens, seed, shape, case_masks, record_view = CASES[name]
        fr = FW.build_frame(seed, W, H, lens=lens, N=N_GAUSS, masks=None, bad_ids=False, once_per_tile=True, record_view=record_view)
        rng = np.random.default_rng(1000 + seed)
        shape(fr, rng, _positions(fr))
        _full_lists(fr, rng, 0.3)
        # (h) out-of-range ids where the median would have been: at a tenth of the pixels that have one, in their tile's list
        clean = median_f64(fr)
        ys, xs = np.nonzero(clean["contrib"] > 0)
        pick = rng.random(len(ys)) < 0.1
        gx = (W + 15) // 16
        tiles = (ys[pick] // 16) * gx + xs[pick] // 16
        at = fr["starts"][tiles] + clean["contrib"][ys[pick], xs[pick]] - 1
        at = np.unique(at)[::3]                                        # (a third of them: the rest keep their medians)
        fr["point_list"][at] = np.where(rng.random(len(at)) < 0.5, -1 - rng.integers(0, 1000, len(at)), fr["N"] + rng.integers(0, 1000, len(at)))
        fr["bad"][at] = True
        fr["would_be_median"] = at
        fr["case_masks"] = case_masks
        _BUILT[name] = (fr, median_f64(fr), clean)
    fr, ref, _ = _BUILT[name]
    masks = fr["case_masks"] if masks == "case" else masks
    fr = dict(fr)
    fr["masks"] = (None if masks is None else np.full(fr["D"], 0xFF, np.uint8) if masks == "ff"
                   else np.random.default_rng(77).integers(0, 256, fr["D"]).astype(np.uint8) | ref["need"])
    return fr, ref


def clean_reference(name):
    """median_f64 of the frame before the out-of-range ids went in."""
    frame(name)
    return _BUILT[name][2]
