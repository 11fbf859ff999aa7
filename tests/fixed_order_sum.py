"""The fixed-order sum ("The fixed-order sum"; csrc/fixed_sum.h) as a numpy model that performs the kernels' additions
one by one, in their order and in their number format, so that a test can ask for the same BITS:

    lane values (each lane adds what it visits, in visit order, onto +0)
    -> the 64-lane butterfly (partners 32, 16, .. 1 away: six pairwise adds)
    -> the four wave sums, converted to the accumulator type, added pairwise (w0+w1)+(w2+w3) or serially ((w0+w1)+w2)+w3
    -> one record per workgroup
    -> the record walk of one finishing workgroup (thread t adds records t, t+256, ... in ascending order onto +0)
    -> the same tree again.

On top of it, the lane visit orders of the flat image kernels whose terms a host can form without transcribing a kernel: the
weight total, the weighted L1 sum, the last three entries of the exposure gradient and the L1 sum of the D-SSIM pass.
Padding a lane with +0 terms is exact: an accumulator that starts at +0 is never -0 (x + -x = +0), and s + 0 = s otherwise."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
WAVE, THREADS, WAVES = 64, 256, 4
GROUP = 4                       # pixels per lane and round of the flat kernels
# The next three are dssim.hip's and dssim_window.h's own, which no header exports: tests/test_fixed_order_sum.py holds them to the source.
BLOCK_PIXELS = THREADS * GROUP  # ... and per workgroup and round (GSR_EXPOSURE_BLOCK_PIXELS, and dssim.hip's SUM_BLOCK_PIXELS)
WEIGHTED_MAX_BLOCKS = 512       # dssim.hip MAX_SUM_BLOCKS: the grid of gsr_weight_total and gsr_weighted_l1_loss_grad
TILE_W, TILE_H = 32, 16         # the D-SSIM tile (dssim_window.h TX, TY): thread t owns pixels (t % 32, 2 (t / 32)) and the one below


def butterfly(lanes):
    """The sum every lane of a wave ends with: lanes (..., 64) -> (...), in the dtype of `lanes`."""
    v = np.asarray(lanes)
    assert v.shape[-1] == WAVE and v.dtype in (F32, F64)
    idx = np.arange(WAVE)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ d]
    return v[..., 0]


def four_waves(w, order):
    """w (..., 4) wave sums -> their total, "pairwise" or "serial"."""
    w0, w1, w2, w3 = (w[..., k] for k in range(WAVES))
    if order == "pairwise":
        return (w0 + w1) + (w2 + w3)
    assert order == "serial", order
    return ((w0 + w1) + w2) + w3


def block_sum(lanes, order, acc=None):
    """A workgroup's total: lanes (..., 256) in the lane type; the wave sums are converted to `acc` (default: the lane type)."""
    v = np.asarray(lanes)
    assert v.shape[-1] == THREADS
    waves = butterfly(v.reshape(v.shape[:-1] + (WAVES, WAVE)))
    return four_waves(waves.astype(acc or v.dtype), order)


def record_walk(records):
    """records (n, ...) -> the finishing workgroup's lane values (..., 256): lane t = ((0 + r[t]) + r[t + 256]) + ..."""
    r = np.asarray(records)
    lanes = np.zeros((THREADS,) + r.shape[1:], r.dtype)
    for j in range(0, r.shape[0], THREADS):
        chunk = r[j:j + THREADS]
        lanes[:chunk.shape[0]] += chunk
    return np.moveaxis(lanes, 0, -1)


def finish(records, order):
    """The second tree: the total of n records (n, ...) -> (...)."""
    return block_sum(record_walk(records), order)


def lane_sums(terms, blocks):
    """The lanes of a grid-stride kernel: item i = (round * blocks + block) * 256 + thread; `terms` (items, K) are what a lane adds
    for one item, K adds in that order.  Returns (blocks, 256) in the dtype of `terms`."""
    t = np.asarray(terms)
    per_round = blocks * THREADS
    rounds = -(-t.shape[0] // per_round) if t.shape[0] else 0
    padded = np.zeros((rounds * per_round, t.shape[1]), t.dtype)
    padded[:t.shape[0]] = t
    padded = padded.reshape(rounds, per_round, t.shape[1])
    acc = np.zeros(per_round, t.dtype)
    for r in range(rounds):
        for k in range(t.shape[1]):
            acc = acc + padded[r, :, k]
    return acc.reshape(blocks, THREADS)


def sequential_sum(x):
    """((x0 + x1) + x2) + ... in the dtype of x."""
    x = np.asarray(x).reshape(-1)
    return np.cumsum(x, dtype=x.dtype)[-1]


def bits(x):
    """The bit pattern(s) of float32 / float64 value(s), for equality that tells -0 from +0 and NaN payloads apart."""
    x = np.asarray(x)
    return x.view(np.uint32 if x.dtype == F32 else np.uint64)


def spread_values(shape, seed, decades=3.0):
    """float32 N(0, 1) times 10^U(-decades, decades): six decades of magnitudes by default, and both signs."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-decades, decades, shape)).astype(F32)


def order_shows(total, terms):
    """True where `total` differs in bits from the sequential sum and from np.sum of the same float32 terms."""
    v = np.asarray(terms, F32).reshape(-1)
    return bool(bits(F32(total)) != bits(sequential_sum(v))) and bool(bits(F32(total)) != bits(np.sum(v, dtype=F32)))


# ---- the inputs of the bit tests ----
# Two sums of n positive float32 terms by two accurate orders agree to within an ulp or two, so they often agree exactly.  Where the
# terms may have either sign, the second half of the pixels therefore repeats the first with the sign turned and the magnitude
# 2^-10 off: the total is a thousandth of the partial sums, whose rounding errors then are hundreds of its ulps, and every order
# of additions leaves its own low bits.  (The sums do not care that a weight is meant to be >= 0.)  Where the terms are positive
# whatever the inputs -- the plain D-SSIM L1 sum -- only the choice of the seed helps: each case takes the first seed on which the
# order shows in all of its sums.
def _second_half(a, seed, sign):
    """a (P, ...) with pixels h .. 2h - 1 (h = P // 2) made of pixels 0 .. h - 1: copies (sign = +1), or negated and 2^-10 off."""
    h = a.shape[0] // 2
    if sign > 0:
        a[h:2 * h] = a[:h]
    else:
        off = np.random.default_rng(seed + 1).uniform(0.5, 1.0, a[:h].shape) * 2.0 ** -10
        a[h:2 * h] = -(a[:h] * (1.0 + off).astype(F32))
    return a


def _inputs(P, W, H, seed, with_g):
    q = {"m": _second_half(spread_values((P,), seed), seed, -1).reshape(H, W),
         "r": _second_half(spread_values((P, 3), seed + 4, 1.0), seed, +1).reshape(H, W, 3), "t": _second_half(spread_values((P, 3), seed + 5, 1.0), seed, +1).reshape(H, W, 3)}
    if with_g:
        q["g"] = _second_half(spread_values((P, 3), seed + 2), seed + 2, -1).reshape(H, W, 3)
    return q


def flat_orders_show(q, exposure_block_pixels, exposure_max_blocks):
    """The condition of the flat kernels' bit tests: every modelled sum differs from the sequential sum and np.sum of its terms."""
    bias = exposure_bias_grad(q["g"], exposure_block_pixels, exposure_max_blocks)
    return (order_shows(weight_total(q["m"]), q["m"]) and order_shows(weighted_l1_sum(q["r"], q["t"], q["m"]), q["m"][:, :, None] * np.abs(q["r"] - q["t"]))
            and all(order_shows(bias[j], q["g"][:, :, j]) for j in range(3)))


@functools.lru_cache(maxsize=4)
def flat_inputs(W, H, exposure_block_pixels=BLOCK_PIXELS, exposure_max_blocks=1024):
    """{"m" (H, W), "r", "t", "g" (H, W, 3)}: m and g cancel by halves; r and t, over two decades (the products m |r - t| then over
    eight: with more, a handful of terms decide the sum in any order), repeat by halves, so that m |r - t| cancels too.  From five
    pixels up (a group and a tail: up to four, every order adds the same pairs), the first seed on which flat_orders_show holds."""
    P = W * H
    for seed in range(7919 * W + H, 7919 * W + H + 64 * 8, 8):
        q = _inputs(P, W, H, seed, True)
        if P <= GROUP or flat_orders_show(q, exposure_block_pixels, exposure_max_blocks):
            return q
    raise AssertionError(f"no seed shows the order at {W}x{H}")


@functools.lru_cache(maxsize=4)
def tile_inputs(W, H):
    """{"m", "r", "t"} likewise for the D-SSIM L1 sums, plain and weighted, from two pixels up."""
    P = W * H
    for seed in range(7919 * W + H, 7919 * W + H + 64 * 8, 8):
        q = _inputs(P, W, H, seed, False)
        ad = np.abs(q["r"] - q["t"])
        if P == 1 or (order_shows(dssim_l1_sum(q["r"], q["t"]), ad) and order_shows(dssim_l1_sum(q["r"], q["t"], q["m"]), q["m"][:, :, None] * ad)):
            return q
    raise AssertionError(f"no seed shows the order at {W}x{H}")


# ---- sizes (W, H), from the block and round counts ----
def flat_sizes(block_pixels=BLOCK_PIXELS, max_blocks=WEIGHTED_MAX_BLOCKS, finish_threads=THREADS):
    """Tail only (1, 3 pixels), one group, groups plus tail, one workgroup exactly, two workgroups with a tail of 1, one record more
    than the finishing workgroup has threads (513 x 513: its lanes add two; tail 1), and more pixels than max_blocks workgroups take
    in one round (1025 x 513: a second grid-stride round; tail 1)."""
    side = int(np.sqrt(finish_threads * block_pixels)) + 1
    return [(1, 1), (3, 1), (GROUP, 1), (5, 7), (block_pixels, 1), (block_pixels + 1, 1), (side, side), (block_pixels + 1, max_blocks + 1)]


def tile_sizes(finish_threads=THREADS):
    """One pixel, one pixel short of a tile, one past it both ways (4 tiles), and more tiles than the finishing workgroup has
    threads (513 x 513: 17 x 33 = 561 tiles)."""
    side = 2 * finish_threads + 1
    assert -(-side // TILE_W) * -(-side // TILE_H) > finish_threads
    return [(1, 1), (TILE_W - 1, TILE_H - 1), (TILE_W + 1, TILE_H + 1), (side, side)]


# ---- the flat kernels ----
def _groups_with_tail(x, P):
    """x (P, ...) -> (ceil(P / 4), 4, ...) padded with +0: the 4-pixel groups, the last one partial."""
    g = -(-P // GROUP)
    out = np.zeros((g * GROUP,) + x.shape[1:], x.dtype)
    out[:P] = x
    return out.reshape((g, GROUP) + x.shape[1:])


def _block0_tail(lanes, tail_terms):
    """Workgroup 0's threads 0 .. (n & 3) - 1 each add the terms of one tail pixel (tail_terms (n & 3, K)) behind their groups."""
    for k in range(tail_terms.shape[1]):
        lanes[0, :tail_terms.shape[0]] += tail_terms[:, k]
    return lanes


def weighted_blocks(n):
    return max(1, min(WEIGHTED_MAX_BLOCKS, -(-n // BLOCK_PIXELS)))


def weight_total(weight):
    """M of gsr_weight_total: a lane adds (m0 + m1) + (m2 + m3) per whole group; pairwise wave sums; one float per workgroup."""
    m = np.asarray(weight, F32).reshape(-1)
    n, n4 = m.size, m.size // GROUP
    q = m[:n4 * GROUP].reshape(n4, GROUP)
    blocks = weighted_blocks(n)
    lanes = lane_sums(((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3]))[:, None], blocks)
    lanes = _block0_tail(lanes, m[n4 * GROUP:, None])
    return finish(block_sum(lanes, "pairwise"), "pairwise")


def weighted_l1_sum(rendered, target, weight):
    """loss_sum of gsr_weighted_l1_loss_grad: a lane adds m_p |r - t| for the 12 floats of a group in memory order."""
    m = np.asarray(weight, F32).reshape(-1)
    d = np.abs(np.asarray(rendered, F32).reshape(-1, 3) - np.asarray(target, F32).reshape(-1, 3))
    terms = m[:, None] * d                      # (n, 3): pixel-major, channel-minor = memory order
    n, n4 = m.size, m.size // GROUP
    blocks = weighted_blocks(n)
    lanes = lane_sums(terms[:n4 * GROUP].reshape(n4, 3 * GROUP), blocks)
    lanes = _block0_tail(lanes, terms[n4 * GROUP:])
    return finish(block_sum(lanes, "pairwise"), "pairwise")


def exposure_bias_grad(dL_dout, block_pixels, max_blocks):
    """dL_dE[9..11] of gsr_exposure_backward, the plain sums of g per channel: a lane adds the pixels of its groups in order, the
    partial last group pixel by pixel through the lane that owns it; 12 sums per 16-float record, pairwise wave sums."""
    g = np.asarray(dL_dout, F32).reshape(-1, 3)
    P = g.shape[0]
    blocks = min(-(-P // block_pixels), max_blocks)
    groups = _groups_with_tail(g, P)            # (groups, 4, 3)
    out = np.empty(3, F32)
    for j in range(3):
        out[j] = finish(block_sum(lane_sums(groups[:, :, j], blocks), "pairwise"), "pairwise")
    return out


def dssim_l1_sum(rendered, target, weight=None):
    """l1_sum of gsr_l1_dssim_loss_grad (weight: of its weighted twin): per 32 x 16 tile, thread t adds |x - y| (times m) of its two
    pixels, channel by channel; pixels outside the image add nothing; one float2 record per tile, row-major; pairwise."""
    x, y = np.asarray(rendered, F32), np.asarray(target, F32)
    H, W = x.shape[:2]
    ad = np.abs(x - y)
    if weight is not None:
        ad = np.asarray(weight, F32)[:, :, None] * ad
    gx, gy = -(-W // TILE_W), -(-H // TILE_H)
    pad = np.zeros((gy * TILE_H, gx * TILE_W, 3), F32)
    pad[:H, :W] = ad
    # (tile row, v0 / 2, p, tile column, u, c) -> lanes (tiles, 256) with thread = (v0 / 2) * 32 + u
    t = pad.reshape(gy, TILE_H // 2, 2, gx, TILE_W, 3).transpose(0, 3, 1, 4, 5, 2).reshape(gy * gx, THREADS, 3, 2)
    lanes = np.zeros((gy * gx, THREADS), F32)
    for c in range(3):
        for p in range(2):
            lanes = lanes + t[:, :, c, p]
    return finish(block_sum(lanes, "pairwise"), "pairwise")
