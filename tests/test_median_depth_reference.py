"""The float64 statement of the median inverse depth (tests/median_depth_reference.py) held to hand-built pixels, its gradient to a
finite difference, and the frame matrix to the cases it is there for -- from the reference alone, on the CPU."""
import numpy as np
import pytest

import frame_walk_frames as FW
import median_depth_reference as M


def pixel(alphas, invd=None, n_contrib=None, ids=None):
    """A 1x1 frame whose Gaussians sit on the pixel with a unit conic: exp(power) = 1, so entry k's alpha is alphas[k]."""
    n = len(alphas)
    N = max(n, 1)
    ids = np.arange(n) if ids is None else np.asarray(ids)
    co = np.zeros((N, 4), np.float32)
    co[:, 0] = co[:, 2] = 1.0
    co[:n, 3] = alphas
    return dict(W=1, H=1, N=N, D=n, xy=np.zeros((N, 2), np.float32), co=co,
                invd=np.asarray(invd if invd is not None else 0.25 + 0.5 * np.arange(N), np.float32),
                point_list=ids.astype(np.int32), ranges=np.array([[0, n]], np.int32),
                n_contrib=np.array([[n if n_contrib is None else n_contrib]], np.int32))


def chosen(fr):
    r = M.median_f64(fr)
    return int(r["contrib"][0, 0]), float(r["med"][0, 0]), r


def test_hand_built_pixels():
    # T = 1, 0.6, 0.3: the second entry takes T to at most one half, and a third behind it changes nothing
    assert chosen(pixel([0.4, 0.5]))[:2] == (2, 0.75)
    assert chosen(pixel([0.4, 0.5, 0.9]))[:2] == (2, 0.75)
    # T = exactly 0.5 behind the first entry (1 - 0.5 is exact in every format): `T > 0.5` is strict, the pixel is closed ...
    c, med, r = chosen(pixel([0.5, 0.5]))
    assert (c, med) == (1, 0.25) and r["T_final"][0, 0] == 0.25 and r["tie"][0, 0]       # (and such a pixel is in the tie band)
    # ... while one float32 ulp less alpha leaves T above one half: the next entry still counts
    assert chosen(pixel([np.nextafter(np.float32(0.5), np.float32(0)), 0.5]))[:2] == (2, 0.75)
    assert chosen(pixel([0.2]))[:2] == (1, 0.25)                            # one entry: T never gets there, the last applied entry wins
    assert chosen(pixel([]))[:2] == (0, 0.0)                                # no entry
    assert chosen(pixel([0.4, 0.5], n_contrib=0))[:2] == (0, 0.0)
    # entries the blend does not apply do not count: alpha < 1/255, an id out of range, an entry past n_contrib
    assert chosen(pixel([0.4, 0.003, 0.2]))[:2] == (3, 1.25)
    assert chosen(pixel([0.003, 0.003]))[:2] == (0, 0.0)
    assert chosen(pixel([0.4, 0.5, 0.2], ids=[0, 7, 2]))[:2] == (3, 1.25)
    assert chosen(pixel([0.4, 0.5, 0.2], ids=[0, -1, 2]))[:2] == (3, 1.25)
    assert chosen(pixel([0.4, 0.5], n_contrib=1))[:2] == (1, 0.25)
    # the 0.99 cap: T = 0.01 behind one opaque entry
    c, med, r = chosen(pixel([1.0, 0.5]))
    assert (c, med) == (1, 0.25) and abs(r["T_final"][0, 0] - 0.005) < 1e-12
    # the value is the float32 inverse depth itself
    fr = pixel([0.9], invd=[np.float32(1) / np.float32(3)])
    assert chosen(fr)[2]["med"].tobytes() == fr["invd"][:1].tobytes()


@pytest.mark.parametrize("name", ["spread_50x37", "edge_16x8"])
def test_gradient_is_the_finite_difference_in_m(name):
    fr, ref = M.frame(name)
    g = M.draw_g(fr["H"], fr["W"]).astype(np.float64)
    signed, scale = M.gradient_f64(fr, ref, g)
    assert (scale >= np.abs(signed)).all() and (scale > 0).sum() >= 3
    loss = lambda r: float((g * r["med"].astype(np.float64)).sum())
    base = loss(ref)
    h = 2.0 ** -6
    touched = np.flatnonzero(scale > 0)
    for i in list(touched[:6]) + [int(np.flatnonzero(scale == 0)[0])]:
        moved = dict(fr)
        moved["invd"] = fr["invd"].copy()
        moved["invd"][i] += np.float32(h)
        step = float(moved["invd"][i]) - float(fr["invd"][i])               # (what float32 made of h)
        r = M.median_f64(moved)
        assert np.array_equal(r["contrib"], ref["contrib"])                 # piecewise constant in everything else
        assert abs((loss(r) - base) / step - signed[i]) <= 1e-9 * max(scale[i], 1.0), i


@pytest.mark.parametrize("name", list(M.CASES))
def test_tie_mask_covers_at_most_one_percent(name):
    fr, ref = M.frame(name)
    share = float(ref["tie"].mean())
    print(f"\nMEDIAN_TIE_SHARE {name} {share:.6f}")
    assert share <= M.MAX_TIES, (name, share)          # a condition on the frame, not a measurement: change the frame, not the cap
    assert name in M.golden()["tie_share"]


def _count(ref, value):
    return int(((ref["contrib"] == value) & ~ref["tie"]).sum())


def test_the_matrix_holds_the_cases_it_is_there_for():
    refs = {name: M.frame(name) for name in M.CASES}
    # (i) image sizes, (j) record views, every kind of mask
    assert {(fr["W"], fr["H"]) for fr, _ in refs.values()} == {(8, 8), (16, 8), (50, 37), (64, 48)}
    assert {fr["record_view"] for fr, _ in refs.values()} == {True, False}
    assert {fr["case_masks"] for fr, _ in refs.values()} == {None, "ff", "random"}
    # (a) the crossing at entry 1
    fr, ref = refs["first_64x48"]
    assert _count(ref, 1) >= 1000
    # (b) crossings spread over the first batch
    for name in ("spread_64x48", "spread_50x37"):
        fr, ref = refs[name]
        crossed = ref["contrib"][(ref["T_final"] <= 0.5) & (ref["contrib"] > 0) & (ref["contrib"] <= 256)]
        assert len(np.unique(crossed)) >= 50 and crossed.min() < 64 and crossed.max() > 192, name   # all four quarters of the batch
    # (c) crossings at list positions 255, 256, 257 and 258: either side of the staging batch's edge, in one frame and in one tile
    fr, ref = refs["edge_64x48"]
    assert all(_count(ref, k) >= 50 for k in (255, 256, 257, 258))
    fr, ref = refs["edge_16x8"]
    assert _count(ref, 256) >= 10 and _count(ref, 257) >= 10
    # (d) crossings in the third batch
    for name in ("third_50x37", "third_8x8"):
        fr, ref = refs[name]
        assert int(((ref["contrib"] > 512) & (ref["T_final"] <= 0.5)).sum()) >= 30 and not ((ref["contrib"] > 0) & (ref["contrib"] <= 512)).any()
    # (e) pixels that never cross: the last applied entry wins, including pixels whose n_contrib is the whole list of 640
    for name in ("never_64x48", "never_8x8"):
        fr, ref = refs[name]
        sel = ref["contrib"] > 0
        assert sel.sum() >= 50 and (ref["T_final"][sel] > 0.5).all()
        assert int((sel & (fr["n_contrib"] == 640)).sum()) >= 10
        assert int((ref["contrib"] > 512).sum()) >= 10
    # (f) n_contrib cuts the walk before the crossing: with the whole list the pixel would have chosen a later entry
    fr, ref = refs["spread_64x48"]
    whole = M.median_f64(fr, np.full_like(fr["n_contrib"], 640))
    assert int(((ref["contrib"] > 0) & (ref["T_final"] > 0.5) & (whole["contrib"] > ref["contrib"])).sum()) >= 100
    # (g) indefinite conics: entries left out for power > 0 inside the walk
    assert all(ref["power_skips"] > 0 for _, ref in refs.values())
    # (h) out-of-range ids where the median would have been, and they moved it
    for name, (fr, ref) in refs.items():
        at = fr["would_be_median"]
        ids = fr["point_list"][at]
        assert len(at) >= 1 and ((ids < 0) | (ids >= fr["N"])).all(), name
        assert (M.clean_reference(name)["contrib"] != ref["contrib"]).any(), name
    # every mask byte of the "random" masks keeps the forward's promise, and some bits are clear
    fr, ref = M.frame("edge_64x48", masks="random")
    assert (fr["masks"] & ref["need"] == ref["need"]).all() and (fr["masks"] != 0xFF).any() and ref["need"].any()
    assert FW.LENS[-1] == 640
