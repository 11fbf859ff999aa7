"""
The shared float32 restatement of csrc/frame_walk.h (tests/frame_walk_reference.py) against statements written out the slow way.
No GPU.

  1. walk_f32 against a per-pixel, per-entry scalar loop written from the header (FrameWalk's bounds, blend_forward_weight's lines)
     that calls nothing of the helper: the applied flags, alpha and T agree bit for bit on frames with out-of-range ids, partial
     tiles and every list length, no id outside [0, N) is yielded, and a range reaching past D is clipped;
  2. ordered_block_sum against a sequential float32 loop over each half;
  3. backward_block's flush adds to columns 3, 4, 6, 7, 9 and 10 and to no other.
"""
import numpy as np
import pytest

import frame_walk_frames as FW
import frame_walk_reference as FWR

f32 = np.float32


def scalar_walk(fr):
    """{(x, y): [(k, id, alpha, T before the entry)] of the applied entries} and {(x, y): final T}, one pixel and one entry at a time."""
    W, H, N, D = fr["W"], fr["H"], fr["N"], fr["D"]
    gx = (W + 15) // 16
    applied, final = {}, {}
    for tile in range(len(fr["ranges"])):
        start = min(max(int(fr["ranges"][tile][0]), 0), D)
        end = min(max(int(fr["ranges"][tile][1]), start), D)
        for q in range(256):
            x, y = (tile % gx) * 16 + q % 16, (tile // gx) * 16 + q // 16
            if x >= W or y >= H:
                continue
            nc = min(max(int(fr["n_contrib"][y, x]), 0), end - start)
            T, hits = f32(1), []
            for k in range(nc):
                i = int(fr["point_list"][start + k])
                if i < 0 or i >= N:
                    continue
                a_, b_, c_ = f32(-0.5) * fr["co"][i, 0], -fr["co"][i, 1], f32(-0.5) * fr["co"][i, 2]
                dx, dy = fr["xy"][i, 0] - f32(x), fr["xy"][i, 1] - f32(y)
                power = (a_ * dx * dx + c_ * dy * dy) + b_ * dx * dy
                with np.errstate(under="ignore", over="ignore"):
                    alpha = min(f32(0.99), fr["co"][i, 3] * np.exp(power))
                if power > 0 or alpha < f32(1.0 / 255.0):
                    continue
                hits.append((k, i, alpha, T))
                T = T * (f32(1) - alpha)
            applied[(x, y)], final[(x, y)] = hits, T
    return applied, final


def helper_walk(fr):
    """The same two dicts from FWR.tiles and FWR.walk_f32 over whole tiles, off-image pixels passed in and flagged."""
    applied = {(x, y): [] for y in range(fr["H"]) for x in range(fr["W"])}
    final = {p: f32(1) for p in applied}
    for tile, s, e, xs, ys in FWR.tiles(fr):
        assert 0 <= s < e <= fr["D"]
        inside = (xs < fr["W"]) & (ys < fr["H"])
        T = np.ones(len(xs), f32)
        for hit, alpha, G, dx, dy, i, con, o, k in FWR.walk_f32(fr, s, e, xs, ys, inside):
            assert 0 <= i < fr["N"] and i == fr["point_list"][s + k] and hit.any() and not hit[~inside].any()
            for p in np.flatnonzero(hit):
                applied[(int(xs[p]), int(ys[p]))].append((k, i, alpha[p], T[p]))
            T = np.where(hit, T * (f32(1) - alpha), T)
        for p in np.flatnonzero(inside):
            final[(int(xs[p]), int(ys[p]))] = T[p]
    return applied, final


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


@pytest.mark.parametrize("W,H", [(8, 8), (20, 12), (33, 17)])
def test_walk_f32_is_the_scalar_loop(W, H):
    fr = FW.build_frame(3, W, H, bad_ids=True)
    if W == 33:                                          # the last tile's range reaches past D, and some pixels' n_contrib with it
        fr["ranges"] = fr["ranges"].copy()
        fr["ranges"][-1, 1] += 1000
        fr["n_contrib"][16:, 32:] = 2000
        assert fr["bad"].any() and [e for *_, e, _, _ in FWR.tiles(fr)][-1] == fr["D"]
    want, want_T = scalar_walk(fr)
    got, got_T = helper_walk(fr)
    assert set(got) == set(want) and (W < 33 or sum(len(v) for v in want.values()) > 1000)      # (8 x 8 is one tile with an empty list)
    for p in want:
        assert [(k, i) for k, i, _, _ in got[p]] == [(k, i) for k, i, _, _ in want[p]], p
        assert _same_bits([a for _, _, a, _ in got[p]], [a for _, _, a, _ in want[p]]), p
        assert _same_bits([t for *_, t in got[p]], [t for *_, t in want[p]]) and _same_bits(got_T[p], want_T[p]), p


def test_ordered_block_sum_is_two_sequential_halves():
    rng = np.random.default_rng(1)
    vals = (rng.normal(0, 1, (300, 64)) * 10.0 ** rng.uniform(-3, 3, (300, 64))).astype(f32)
    want = np.zeros(300, f32)
    for n, v in enumerate(vals):
        lo, hi = f32(0), f32(0)
        for j in range(32):
            lo, hi = lo + v[j], hi + v[32 + j]
        want[n] = lo + hi
    got = FWR.ordered_block_sum(vals)
    assert got.dtype == f32 and _same_bits(got, want)
    assert (got != vals.sum(1, dtype=f32)).any()         # the order matters on these vectors: numpy's own sum is pairwise
    assert _same_bits(FWR.ordered_block_sum(vals.reshape(3, 100, 64)), want.reshape(3, 100))


def test_backward_block_flushes_six_columns():
    fr = FW.build_frame(5, 33, 17, bad_ids=True)
    acc = np.zeros((fr["N"], 16), f32)
    entries = 0
    for tile, s, e, xs, ys in FWR.tiles(fr):
        for bx, by, inside in FWR.blocks(xs, ys, fr["W"], fr["H"]):
            assert len(bx) == 64 and np.array_equal(bx - bx[0], np.arange(64) & 7) and np.array_equal(by - by[0], np.arange(64) >> 3)
            tails = FWR.backward_block(fr, s, e, bx, by, inside, np.zeros(64, f32), lambda i, dx, dy, w: (np.ones(64, f32), ()), acc)
            assert all(t.shape == (0,) for _, t in tails)
            entries += len(tails)
    assert entries > 100
    touched = (3, 4, 6, 7, 9, 10)
    assert all(acc[:, c].any() for c in touched)
    assert not acc[:, [c for c in range(16) if c not in touched]].any()
    assert np.isfinite(acc).all()
