"""
Float64 yardstick for N-channel feature rendering (include/gsr_features.h), and a float32 restatement of its two sums.

Test helper, not a test file: a thin layer over blend_grad_reference.of_buffers.  Its `on_tile` callback hands out the dense float64
terms of every tile; with dL_dpixels = 1 and background 0, terms["dL_dcolor"][:, :, 0] is the weight w_k(p) of every (pixel, entry)
pair -- zero where the entry does not contribute, and zero at the pixels the module masks (a decision within NEAR of its threshold,
or a float64 n_contrib other than the forward's).  From those weights

    out[p][c]   = sum_k w_k(p) F[i_k][c]          (float64)
    dL_dF[i][c] = sum_p w_i(p) G[p][c]            (float64; G is zeroed at the masked pixels, so both sides lose them)
    mag[i][c]   = sum_p w_i(p) |G[p][c]|          (the unit a row's error is measured in)

The float32 restatement (numpy) takes nothing from float64: it replays the header's definition on the same buffers (frame_walk_reference.weights_f32) -- the float32
power expression with the pre-scaled conic, alpha = min(0.99, o exp(power)), the two skip tests, w = alpha T, T <- T (1 - alpha),
up to the FORWARD's n_contrib -- and sums out in list order and dL_dF in pixel order, one float32 multiply and one float32 add per
term.  `drops` removes terms from its backward sum only (a list entry, or one 8x4 block of a list entry), for the tests that show
the criterion sees them.

Errors: forward, max |out - out64| over the unmasked pixels in units of max |F|; backward, per Gaussian row, |dF - dF64| / mag,
worst channel (a channel whose mag is 0 must be exactly 0: inf otherwise).
"""
import numpy as np

import blend_grad_reference as B
import frame_walk_reference as FWR

TILE = 16
MAX_MASKED = 0.01
f32 = np.float32
_np = FWR.to_np


def golden():
    """tests/golden/features_margins.json: "floor", the smallest float32-restatement error of the CPU matrix, and "E_kernel", what an
    MI355X run measured per frame (tools/record_features_margins.py)."""
    return FWR.golden("features_margins")


def weights_f32(buf, W, H, tile, xs, ys):
    """(P, L) float32 weights of one tile by the header's definition, bounded by the forward's n_contrib."""
    fr = FWR.frame_of_buffers(buf, W, H)
    return FWR.weights_f32(fr, FWR.tile_range(fr, tile), xs, ys)


def _row_f32(wb, g32, C):
    row = np.zeros((wb.shape[1], C), f32)
    for p in range(wb.shape[0]):                                     # pixel order
        if wb[p].any():
            row = row + wb[p][:, None] * g32[p][None, :]
    return row


def render(buf, W, H, F, G, drops=()):
    """buf: a forward's buffer dict (numpy or torch).  F (N, C), G (H, W, C).  drops: ("entry", list position) or ("block", list
    position, 8x4 block 0..7) items; for each, dF32_dropped holds the float32 backward sum with that term left out.  Returns a dict:
    out64 (H, W, C), dF64 (N, C), mag (N, C), out32, dF32 (float32), dF32_dropped (list), mask (H, W) bool, n_contrib64, longest
    (list), D, tiles (per non-empty tile: tile, xs, ys, idx, w (P, L) float64, masked (P,))."""
    F64, G64 = _np(F, np.float64), _np(G, np.float64)
    F32, G32 = _np(F, f32), _np(G, f32)
    N, C = F64.shape
    ranges = _np(buf["ranges"]).reshape(-1, 2)
    nb = {k: _np(v) for k, v in buf.items() if k in ("points_xy_image", "conic_opacity", "colors", "depths", "point_list", "ranges", "n_contrib")}
    fr = FWR.frame_of_buffers(nb, W, H)
    out64, out32 = np.zeros((H, W, C)), np.zeros((H, W, C), f32)
    dF64, mag = np.zeros((N, C)), np.zeros((N, C))
    sums32 = [np.zeros((N, C), f32) for _ in range(1 + len(drops))]      # the intact sum, then one per drop
    tiles = []

    def on_tile(tile, xs, ys, idx, active, terms, masked):
        w = terms["dL_dcolor"][:, :, 0]                              # (P, L) float64, zero at the masked pixels
        tiles.append((tile, xs, ys, idx, w, masked))
        g = np.where(masked[:, None], 0.0, G64[ys, xs])
        out64[ys, xs] = w @ F64[idx]
        np.add.at(dF64, idx, w.T @ g)
        np.add.at(mag, idx, w.T @ np.abs(g))
        w32 = FWR.weights_f32(fr, FWR.tile_range(fr, tile), xs, ys)
        acc = np.zeros((len(xs), C), f32)
        for k in range(w32.shape[1]):                                # list order
            if w32[:, k].any():
                acc = acc + w32[:, k, None] * F32[idx[k]][None, :]
        out32[ys, xs] = acc
        g32 = np.where(masked[:, None], f32(0), G32[ys, xs])
        row = _row_f32(w32, g32, C)
        for v, drop in enumerate((None,) + tuple(drops)):
            r = row
            k = -1 if drop is None else drop[1] - int(ranges[tile, 0])
            if 0 <= k < w32.shape[1]:
                wb = w32.copy()
                if drop[0] == "entry":
                    wb[:, k] = 0
                else:
                    wb[((ys % 16) // 4) * 2 + (xs % 16) // 8 == drop[2], k] = 0
                r = _row_f32(wb, g32, C)
            for j, i in enumerate(idx):                              # tiles in order; a Gaussian's entries of one tile in list order
                sums32[v][i] = sums32[v][i] + r[j]

    ref = B.of_buffers(nb, np.zeros(3, f32), W, H, np.ones((H, W, 3), f32), on_tile=on_tile)
    lens = ranges[:, 1] - ranges[:, 0]
    return dict(out64=out64, dF64=dF64, mag=mag, out32=out32, dF32=sums32[0], dF32_dropped=sums32[1:], mask=ref["mask"],
                n_contrib64=ref["n_contrib"], longest=int(lens.max()) if len(lens) else 0, D=int(nb["point_list"].shape[0]), tiles=tiles)


def forward_error(out, r, F):
    """max |out - out64| over the unmasked pixels, in units of max |F|."""
    keep = ~r["mask"]
    d = np.abs(_np(out, np.float64).reshape(r["out64"].shape) - r["out64"])[keep]
    return float(d.max() / np.abs(_np(F, np.float64)).max()) if d.size else 0.0


def backward_errors(dF, r):
    """(N,) float64: per Gaussian row |dF - dF64| / mag, the worst channel."""
    got = _np(dF, np.float64).reshape(r["dF64"].shape)
    d, sc = np.abs(got - r["dF64"]), r["mag"]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(sc > 0, d / np.where(sc > 0, sc, 1.0), np.where(got != 0, np.inf, 0.0))
    return e.max(1) if e.size else np.zeros(e.shape[0])


def backward_error(dF, r):
    e = backward_errors(dF, r)
    return float(e.max()) if e.size else 0.0


def spread(a, b, r):
    """The worst difference of two runs in the same units."""
    d = np.abs(_np(a, np.float64).reshape(r["mag"].shape) - _np(b, np.float64).reshape(r["mag"].shape))
    sel = r["mag"] > 0
    return float((d[sel] / r["mag"][sel]).max()) if sel.any() else 0.0


def forward_criterion(E_kernel, E_f32):
    return E_kernel <= 3.0 * E_f32 + 2.0 ** -23


def backward_criterion(E_kernel, E_f32, E_spread, floor):
    return E_kernel <= 3.0 * max(E_f32, E_spread) + floor


# The four small scenes (conftest.lego_camera frame 0): (synthetic_scene arguments, opacity override, W, H)
SCENES = {
    "n300_50x37": ((300, 0.05, 0.6, 1), None, 50, 37),            # partial tiles on both axes
    "n2000_64x48": ((2000, 0.05, 0.6, 2), None, 64, 48),
    "n900_faint_48x32": ((900, 0.2, 0.3, 3), 0.01, 48, 32),       # faint, long lists: past one and two 256-entry batches, no saturation
    "n1500_opaque_48x48": ((1500, 0.15, 0.3, 4), 0.9, 48, 48),    # early saturation
}


def scene(scenes_mod, cameras_mod, name):
    from conftest import lego_camera, render_kwargs
    args, opacity, W, H = SCENES[name]
    sc = scenes_mod.synthetic_scene(*args)
    if opacity is not None:
        sc["opacities"][:] = opacity
    cam = lego_camera(cameras_mod, 0, width=W, height=H)
    return sc, cam, render_kwargs(sc, cam, width=W, height=H)


def draw(N, C, H, W, seed=11):
    """F (N, C) and G (H, W, C) from U(-1, 1), float32."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (N, C)).astype(f32), rng.uniform(-1, 1, (H, W, C)).astype(f32)
