"""
The blend backward held to float64 Gaussian by Gaussian (tests/blend_grad_reference.py): the CPU half.  No GPU.

parity.assert_grad judges a gradient array against its own largest element, and blend gradients are heavy-tailed: a Gaussian
behind opaque ones, a speck, a faint one or a splat that clips a tile corner has its whole gradient inside the absolute band, so a
dropped 8x4 block or a dropped list entry -- an error of order one in that Gaussian's gradient -- passes.  Here every Gaussian's
error is divided by its own `scale` (the magnitude its terms carry before they cancel), after the pixels at which a float32
forward may decide otherwise than float64 have been taken out of BOTH sides by zeroing their cotangents (the backward is linear in
them), so no threshold flip enters and no loose band is needed.

  1. blend_grad_reference against f64_reference.backward_f64's autograd, per Gaussian, on test_f64_reference.CASE_NAMES (the four
     outputs the plain backward has), against absgrad_reference (signed and abs of dL_dmean2D, to 1e-12 of abs), and with depth and
     alpha cotangents against test_gpu_aux_grads.aux_backward_f64 (autograd again; on the cases up to 64 x 48: three autograd passes
     per tile make the 200 x 136 ones take a minute).
  2. the oracle (the float32 reference-order restatement) per Gaussian against the module: E_oracle per case and array, their
     smallest per array the criterion's floor (tests/golden/blend_grad_margins.json), and the masking conditions: at most 1 % of a
     case's pixels masked; at the others the oracle's n_contrib is float64's and its final_T within 1e-3 relative of float64's,
     where one flipped alpha >= 1/255 moves it by 3.9e-3 or more: the oracle agrees on every decision the mask keeps.
  3. the criterion E <= 3 max(E_oracle, E_spread) + floor sees what parity.assert_grad misses: a dropped 8x4 block of a small
     Gaussian, a dropped list entry of a small Gaussian at positions 31, 32, 127 and 128 (small: |g| below 1e-4 of the array's
     largest, the whole gradient inside assert_grad's absolute band).

The designed cases (test_gpu_blend_grad.py runs the kernels on them) are built here: specks under one pixel on the 8x4, 8x8 and
tile boundaries, faint Gaussians at 1 to 3 times 1/255, a 480-entry stack over tile (2, 1) with capped alphas in it, thin 40:1
splats (long axis 0.3 scene units), ordinary ones; and a frame with nothing visible.
"""
import json
import os

import numpy as np
import pytest

from conftest import ROOT, backward_kwargs, render_kwargs
import absgrad_reference as AR
import blend_grad_reference as B
import f64_reference as F
import parity
import test_f64_reference as R

PLAIN = B.OUTPUTS[:4]                       # what a backward without depth / alpha cotangents returns
MAX_MASKED = 0.01
GOLDEN = os.path.join(ROOT, "tests", "golden", "blend_grad_margins.json")
DESIGNED = {"designed_100x70": (100, 70, 41), "designed_97x61": (97, 61, 42)}
STACK_TILE = (2, 1)
ORACLE_CASES = R.CASE_NAMES + list(DESIGNED)


def designed_case(cameras, W, H, seed):
    rng = np.random.default_rng(seed)
    Rm = R._rotation(rng)
    d = Rm[2]
    cam = R.camera(cameras, Rm, 3.0 * d, W, H)
    tx, ty = float(cam["tan_fovx"]), float(cam["tan_fovy"])
    fx = W / (2.0 * tx)
    parts = []          # (pixel x, pixel y, depth, sigma per axis in pixels at that depth, opacity)

    def add(px, py, z, sig, op):
        px, py, z, op = (np.asarray(a, np.float64).ravel() for a in (px, py, z, op))
        parts.append((px, py, z, np.asarray(sig, np.float64).reshape(len(px), -1) * np.ones((1, 3)), op))
    n = 640             # specks: the boundary between pixels 7 and 8 is x = 7.5
    add(rng.integers(0, W // 8 + 1, n) * 8 - 0.5 + rng.uniform(-0.35, 0.35, n), rng.integers(0, H // 4 + 1, n) * 4 - 0.5 + rng.uniform(-0.35, 0.35, n),
        rng.uniform(2.5, 6.0, n), rng.uniform(0.05, 0.3, (n, 1)), rng.uniform(0.2, 0.95, n))
    n = 800             # faint: the reach rectangle is a few pixels
    add(rng.uniform(-2, W + 2, n), rng.uniform(-2, H + 2, n), rng.uniform(2.5, 6.0, n), rng.uniform(1.0, 4.0, (n, 1)), rng.uniform(1.0, 3.0, n) / 255.0)
    n = 480             # the stack, in depth order: capped entries among faint ones, so pixels end at many list positions
    op = rng.uniform(0.008, 0.016, n)
    op[[150, 300, 440, 441, 442]] = 1.0
    add(16 * STACK_TILE[0] + 7.5 + rng.uniform(-1, 1, n), 16 * STACK_TILE[1] + 7.5 + rng.uniform(-1, 1, n), np.linspace(3.0, 5.0, n), np.full((n, 1), 7.0), op)
    n = 300             # thin
    long_ = rng.uniform(5.0, 12.0, n)
    add(rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(2.5, 6.0, n), np.stack([long_, long_ / 40.0, long_ / 40.0], 1), rng.uniform(0.1, 0.9, n))
    n = 500             # ordinary
    add(rng.uniform(-5, W + 5, n), rng.uniform(-5, H + 5, n), rng.uniform(2.5, 6.0, n), rng.uniform(0.5, 3.0, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3)),
        rng.uniform(0.05, 0.95, n))
    px, py, z, sig, op = (np.concatenate([p[i] for p in parts]) for i in range(5))
    N = len(px)
    pc = np.stack([((2 * px + 1) / W - 1) * z * tx, ((2 * py + 1) / H - 1) * z * ty, z], 1)
    q = rng.normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    shs = np.concatenate([rng.normal(0, 0.5, (N, 1, 3)), rng.normal(0, 0.15, (N, 15, 3))], 1)
    sc = {"means": (pc @ Rm + 3.0 * d).astype(np.float32), "scales": (sig * z[:, None] / fx).astype(np.float32), "rotations": q.astype(np.float32),
          "opacities": op.astype(np.float32).reshape(N, 1), "shs": shs.astype(np.float32)}
    assert sc["scales"].max() <= 1.5 and (sc["scales"].max(1) / sc["scales"].min(1)).max() <= 50.0      # the fuzz suite's conditioning
    return sc, cam, render_kwargs(sc, cam, width=W, height=H, degree=2, train_convention=True, bg=(0.3, 0.5, 0.2))


def nothing_visible_case(cameras):
    """Every Gaussian behind the camera: D = 0."""
    sc, cam, kw = R.make_case(cameras, W=64, H=48, n=300, degree=3, train=True, bg=(0.2, 0.1, 0.4), sm=1.0, seed=5)
    c = np.asarray(cam["camera_center"], np.float32)
    fwd_dir = np.asarray(cam["world_to_camera"], np.float64)[:3, 2]
    sc["means"] = (c - 3.0 * fwd_dir + 0.1 * (np.asarray(sc["means"]) - c)).astype(np.float32)
    kw = render_kwargs(sc, cam, width=64, height=48, bg=(0.2, 0.1, 0.4))
    return sc, cam, kw


_CACHE = {}


def get_case(oracle, cameras, name):
    """{sc, cam, kw, buf (the oracle's forward)} of a float64-matrix case, a designed one or "nothing_visible"."""
    if name in R.CASE_NAMES:
        return R.oracle_case(oracle, cameras, name)
    if name not in _CACHE:
        sc, cam, kw = nothing_visible_case(cameras) if name == "nothing_visible" else designed_case(cameras, *DESIGNED[name])
        _CACHE[name] = dict(sc=sc, cam=cam, kw=kw, buf=oracle.render_gaussians(**kw)[2])
    return _CACHE[name]


def cotangents(H, W, seed=7, aux=False):
    rng = np.random.default_rng(seed)
    dpix = rng.normal(0, 1, (H, W, 3)).astype(np.float32)
    if not aux:
        return dpix, None, None
    return dpix, rng.normal(0, 1, (H, W)).astype(np.float32), rng.normal(0, 1, (H, W)).astype(np.float32)


def block_collector(D_len, ranges):
    """An on_tile hook and its two arrays: per list entry and 8x4 block of its tile (bit k of the forward's mask byte: k & 1 the x
    half, k >> 1 the band of four rows), the sums of the signed terms (D, 8, 11: OUTPUTS in order) and whether any term is active
    at a pixel the mask keeps."""
    terms, act = np.zeros((D_len, 8, 11)), np.zeros((D_len, 8), bool)
    ranges = np.asarray(ranges).reshape(-1, 2)

    def on_tile(tid, xs, ys, idx, active, t, masked):
        s = int(ranges[tid, 0])
        blk = ((ys % 16) // 4) * 2 + (xs % 16) // 8
        allt = np.concatenate([t[k] for k in B.OUTPUTS], 2)              # (P, L, 11)
        for k in range(8):
            sel = blk == k
            if sel.any():
                terms[s:s + len(idx), k] = allt[sel].sum(0)
                act[s:s + len(idx), k] = active[sel & ~masked].any(0)
    return on_tile, terms, act


COLS = {"dL_dcolor": slice(0, 3), "dL_dmean2D": slice(3, 5), "dL_dconic": slice(5, 9), "dL_dopacity": slice(9, 10), "dL_dinv_depths": slice(10, 11)}
_ORACLE = {}


def oracle_side(oracle, cameras, name):
    """The oracle's backward of a case on masked cotangents and the float64 sums on its own buffers: {ref, g, E, mask, dpix (masked),
    blk_terms, blk_active}, once per session."""
    if name not in _ORACLE:
        c = get_case(oracle, cameras, name)
        kw, buf = c["kw"], c["buf"]
        H, W = kw["image_height"], kw["image_width"]
        dpix, _, _ = cotangents(H, W)
        on_tile, bt, ba = block_collector(int(np.asarray(buf["point_list"]).shape[0]), buf["ranges"])
        ref = B.of_buffers(buf, kw["background"], W, H, dpix, on_tile=on_tile)
        (dpm,) = B.masked(ref["mask"], dpix)
        g = oracle.backward(**backward_kwargs(c["sc"], c["cam"], kw, buf, dpm))
        E = {k: B.worst(B.kernel_layout(g, k), ref[k]) for k in PLAIN}
        _ORACLE[name] = dict(ref=ref, g=g, E=E, mask=ref["mask"], dpix=dpm, blk_terms=bt, blk_active=ba)
    return _ORACLE[name]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def criterion(E_kernel, E_oracle, E_spread, floor):
    return E_kernel <= 3.0 * max(E_oracle, E_spread) + floor


# ---- 1. the module against autograd ----
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_signed_sums_are_the_autograd_gradients(oracle, cameras, name):
    c = R.oracle_case(oracle, cameras, name)
    buf = c["buf"]
    r = B.of_case(c["pre"], buf["point_list"], buf["ranges"], c["dpix"])
    f = F.backward_f64(c["sc"], c["kw"], buf["point_list"], buf["ranges"], c["dpix"], pre=c["pre"])
    for k in PLAIN:
        e = B.worst(B.kernel_layout(f, k), r[k])
        assert e <= 1e-10, (k, e)                      # float64 sums in two orders, in units of the terms' magnitude (measured 2.5e-12)
        assert np.all(r[k]["abs"] <= r[k]["scale"] * (1 + 1e-12)) and np.all(np.abs(r[k]["signed"]) <= r[k]["abs"] * (1 + 1e-12) + 1e-300)
    a = AR.of_case(c["pre"], buf["point_list"], buf["ranges"], c["dpix"])
    for s in ("signed", "abs"):
        assert np.all(np.abs(a[s] - r["dL_dmean2D"][s]) <= 1e-12 * a["abs"]), s


@pytest.mark.parametrize("name", [n for n in R.CASE_NAMES if not n.startswith("200x")])
def test_depth_and_alpha_cotangents_against_autograd(oracle, cameras, name):
    from test_gpu_aux_grads import aux_backward_f64
    c = R.oracle_case(oracle, cameras, name)
    kw, buf = c["kw"], c["buf"]
    H, W = kw["image_height"], kw["image_width"]
    dpix, gD, gA = cotangents(H, W, 11, aux=True)
    f_pix, f_dep, f_alp, _ = aux_backward_f64(c, dpix, gD, gA)
    r = B.of_case(c["pre"], buf["point_list"], buf["ranges"], dpix, gD, gA)
    for k in B.OUTPUTS:                                # (the blend-stage outputs carry no Q3 constant: plainly additive)
        e = B.worst(B.kernel_layout(f_pix, k) + B.kernel_layout(f_dep, k) + B.kernel_layout(f_alp, k), r[k])
        assert e <= 1e-10, (k, e)
    if (np.asarray(buf["radii"]) > 0).any():
        assert np.abs(r["dL_dinv_depths"]["signed"]).max() > 0


# ---- 2. the oracle per Gaussian; the masking conditions; the floor ----
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_oracle_per_gaussian_and_the_mask(oracle, cameras, name):
    c = get_case(oracle, cameras, name)
    o = oracle_side(oracle, cameras, name)
    kw, buf = c["kw"], c["buf"]
    H, W = kw["image_height"], kw["image_width"]
    mask, ref = o["mask"], o["ref"]
    print(f"\n{name}: masked {mask.mean():.5f} of the pixels ({int((ref['margin'] < B.NEAR).sum())} near a threshold, "
          f"{int((ref['n_contrib'] != np.asarray(buf['n_contrib']).reshape(H, W)).sum())} with another n_contrib); E_oracle "
          + ", ".join(f"{k} {v:.3e}" for k, v in o["E"].items()))
    assert mask.mean() <= MAX_MASKED
    keep = ~mask
    assert np.array_equal(ref["n_contrib"][keep], np.asarray(buf["n_contrib"]).reshape(H, W)[keep])
    t = lambda a: np.asarray(a, np.float64)
    import torch
    T64 = F.blend_f64(*(torch.as_tensor(x) for x in (t(buf["points_xy_image"]), t(buf["conic_opacity"])[:, :3], t(buf["conic_opacity"])[:, 3],
                                                     t(buf["colors"]), t(buf["depths"]))), buf["point_list"], buf["ranges"],
                      torch.as_tensor(t(kw["background"])[:3]), W, H)[2].numpy()
    relT = np.abs(np.asarray(buf["final_Ts"], np.float64).reshape(H, W) / T64 - 1.0)[keep]
    assert relT.max() < 1e-3, relT.max()
    for k, v in o["E"].items():
        assert np.isfinite(v), f"{k}: a Gaussian whose terms are all zero has a non-zero gradient"
    rec = golden()["E_oracle"].get(name)
    assert rec is not None and all(0.5 * rec[k] <= o["E"][k] <= 2.0 * rec[k] for k in PLAIN), (rec, o["E"])    # what is on file is this


def test_designed_cases_reach_what_they_were_built_for(oracle, cameras):
    for name in DESIGNED:
        c = get_case(oracle, cameras, name)
        o = oracle_side(oracle, cameras, name)
        kw, buf = c["kw"], c["buf"]
        W = kw["image_width"]
        gx = (W + 15) // 16
        tile = STACK_TILE[1] * gx + STACK_TILE[0]
        s, e = (int(v) for v in np.asarray(buf["ranges"]).reshape(-1, 2)[tile])
        nc = o["ref"]["n_contrib"][16 * STACK_TILE[1]:16 * STACK_TILE[1] + 16, 16 * STACK_TILE[0]:16 * STACK_TILE[0] + 16]
        assert e - s >= 400 and nc.max() >= 400
        ended = nc[nc < e - s] % 32                                        # pixels that ended before the list did
        assert ((ended >= 4) & (ended <= 28)).sum() >= 16                  # ... in the middle of a 32-entry bucket
        co = np.asarray(buf["conic_opacity"], np.float64)
        assert (co[:, 3] > 0.99).sum() >= 5 and ((co[:, 3] >= 1 / 255) & (co[:, 3] <= 3.001 / 255)).sum() >= 700
        assert c["sc"]["means"].shape[0] < 4000
    c = get_case(oracle, cameras, "nothing_visible")
    assert int(np.asarray(c["buf"]["point_list"]).shape[0]) == 0


def test_floor_on_file_is_the_smallest_oracle_margin(oracle, cameras):
    E = {name: oracle_side(oracle, cameras, name)["E"] for name in ORACLE_CASES}
    floor = golden()["floor"]
    for k in PLAIN:
        smallest = min(E[n][k] for n in ORACLE_CASES if E[n][k] > 0)
        print(f"  {k}: floor on file {floor[k]:.3e}, smallest E_oracle now {smallest:.3e}")
        assert floor[k] <= 2.0 * smallest                                  # (the libm's expf may differ from the one it was recorded with)
    assert floor["dL_dinv_depths"] == floor["dL_dcolor"]                  # the oracle has no depth cotangent: the same w_k sums


# ---- 3. what the old criterion misses ----
def _small_rows(g, frac=1e-4):
    m = np.abs(g).max(1)
    return (m > 0) & (m < frac * m.max())


def test_a_dropped_block_passes_assert_grad_and_fails_the_criterion(oracle, cameras):
    name = "designed_100x70"
    c, o = get_case(oracle, cameras, name), oracle_side(oracle, cameras, name)
    pl = np.asarray(c["buf"]["point_list"]).astype(np.int64)
    floor = golden()["floor"]
    for k in PLAIN:
        g = B.kernel_layout(o["g"], k).copy()
        small = _small_rows(g)
        bt = o["blk_terms"][:, :, COLS[k]]                                   # (D, 8, width)
        mag = np.abs(bt).max(2)
        mag[mag > 0.5 * parity.GRAD_ABS * np.abs(o["ref"][k]["signed"]).max()] = 0      # (terms may exceed their cancelled sum)
        # one (entry, block) per small Gaussian: the block carrying most of what that Gaussian gets
        order = np.argsort(-mag.max(1))
        seen, n = set(), 0
        for e in order:
            i = int(pl[e])
            if not small[i] or i in seen or mag[e].max() == 0:
                continue
            seen.add(i)
            g[i] -= bt[e, int(mag[e].argmax())]
            n += 1
            if n == 8:
                break
        assert n == 8, (k, n)
        parity.assert_grad(k, g, o["ref"][k]["signed"])                      # the array-wide contract does not see it
        E = B.worst(g, o["ref"][k])
        print(f"  {k}: 8 small Gaussians lose one 8x4 block each: assert_grad passes, E = {E:.3e} against E_oracle {o['E'][k]:.3e}")
        assert not criterion(E, o["E"][k], 0.0, floor[k])
        assert E > 100 * (3.0 * o["E"][k] + floor[k])


ENTRY_CASES = list(DESIGNED) + ["200x136_n3000"]     # the cases with tile lists of more than 128 entries


@pytest.mark.parametrize("position", [31, 32, 127, 128])
def test_a_dropped_list_entry_passes_assert_grad_and_fails_the_criterion(oracle, cameras, position):
    """A small Gaussian (|g| below 1e-4 of the array's largest, as in the dropped-block test) seldom sits that early in a list, so
    every case with long lists is searched, per array; every array that has such a Gaussian at this position shows it."""
    floor = golden()["floor"]
    done = 0
    for k in PLAIN:
        best = None                                                          # the entry there that is most of its Gaussian's gradient
        for name in ENTRY_CASES:
            c, o = get_case(oracle, cameras, name), oracle_side(oracle, cameras, name)
            pl = np.asarray(c["buf"]["point_list"]).astype(np.int64)
            small = _small_rows(B.kernel_layout(o["g"], k))
            m = np.abs(o["ref"][k]["signed"]).max()
            for s, e in np.asarray(c["buf"]["ranges"]).reshape(-1, 2):
                if e - s <= position or not small[int(pl[s + position])]:
                    continue
                drop = o["blk_terms"][s + position][:, COLS[k]].sum(0)
                if not np.any(drop) or np.abs(drop).max() > 0.5 * parity.GRAD_ABS * m:      # (terms may exceed their cancelled sum)
                    continue
                share = float((np.abs(drop) / np.maximum(o["ref"][k]["scale"][int(pl[s + position])], 1e-300)).max())
                if best is None or share > best[0]:
                    best = (share, int(pl[s + position]), drop, name)
        if best is None:
            continue
        o = oracle_side(oracle, cameras, best[3])
        g = B.kernel_layout(o["g"], k).copy()
        g[best[1]] -= best[2]
        parity.assert_grad(k, g, o["ref"][k]["signed"])                      # the array-wide contract does not see it
        E = B.worst(g, o["ref"][k])
        print(f"  {k}, {best[3]}: entry {position} of a tile's list dropped from a small Gaussian: assert_grad passes, E = {E:.3e} "
              f"against E_oracle {o['E'][k]:.3e}")
        assert not criterion(E, o["E"][k], 0.0, floor[k]), (k, E)
        assert E > 100 * (3.0 * o["E"][k] + floor[k])
        done += 1
    assert done >= 1
