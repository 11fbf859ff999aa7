"""
The blend backward (blend_bwd_splat.hip) held to float64 Gaussian by Gaussian on the MI355X.  tests/test_blend_grad_reference.py
has the why, the reference's own checks, the designed cases and what the array-wide contract misses.

Per case the float64 sums (tests/blend_grad_reference.py) are taken on the KERNEL forward's own per-Gaussian buffers; the pixels
within NEAR of a decision threshold, or whose n_contrib is not float64's, have their cotangents zeroed before any backward call
(at most 1 % of the pixels: asserted), so both sides lose them.  Every Gaussian's error is measured in units of its own `scale`:

    E_kernel <= 3 max(E_oracle, E_spread) + floor

E_oracle the oracle's error on the same case (the float32 reference-order restatement on its own masked cotangents), E_spread the
worst difference between two kernel runs, floor the smallest E_oracle of the CPU matrix (tests/golden/blend_grad_margins.json).
The oracle has no depth or alpha cotangents and no absolute sums: those runs are held to the plain run's E_oracle of the same case
(dL_dinv_depths to dL_dcolor's, the same w_k sums; dL_dmean2D_abs, against `abs`, to dL_dmean2D's).  A Gaussian whose float64 terms
are all zero must come back exactly zero.  Each check prints its row (BLEND_GRAD_ROW, JSON); tools/record_blend_grad_margins.py files
a run's rows in profiles/blend_grad/.  None is on file yet: whether the kernel, and in particular the outputs held to another
array's E_oracle, fit the bound is not known before the first MI355X run.

Which test reaches which path of the kernel:
  own chain (forward's records, block masks, cost-ordered block list, workspace cleared by the forward, second step of a
      sequence)                                   test_own_chain_and_copies[*] ("own chain" rows)
  copies (re-packed records, the kernel's own compaction, its own clear)      test_own_chain_and_copies[*] ("copies" rows)
  AUX (dL_ddepth_image, dL_dalpha_image) and ABS (absgrad=True), with masks and without      test_aux_and_absgrad[*]
  sh_gradient="factored" (payload rows against dL_dcolor), blend half on its own             test_factored_payload
  capacity mode, K > D                                                                       test_capacity_mode_frame
  8x4 and 8x8 blocks (GSR_BWD_BLOCK=32 / 64, a fresh child process each)                     test_each_block_shape[*]
  a frame with nothing visible                                                               test_nothing_visible
  the forward's block masks against the float64 terms                                        test_forward_block_masks_cover_every_active_term[*]

The mask check's positional bound: blend_fwd.hip writes a mask byte for every entry of every batch it stages, stages batches in list
order without gaps while any wave of the tile is alive, and n_contrib is the 1-based LIST position of a pixel's last contributing
entry (not a count of entries walked), which lies in a staged batch.  So every position below the tile's largest n_contrib is
inside the written prefix, and those are the positions judged.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, sub
import blend_grad_reference as B
import parity
import test_blend_grad_reference as T

pytestmark = pytest.mark.gpu
CASES = ["200x136_n700", "200x136_n3000"] + list(T.DESIGNED)
E_ORACLE_OF = {"dL_dinv_depths": "dL_dcolor", "dL_dmean2D_abs": "dL_dmean2D", "payload": "dL_dcolor"}
_SIDE = {}


def _np_buf(buf):
    return {k: parity.to_np(v) for k, v in buf.items()}


def kernel_side(oracle, cameras, name):
    """The kernel's forward of a case as the second step of a sequence, the float64 sums on its buffers for the plain and the
    depth + alpha cotangents, the masked cotangents, once per session."""
    if name not in _SIDE:
        gsr = pkg()
        c = T.get_case(oracle, cameras, name)
        kw = c["kw"]
        H, W = kw["image_height"], kw["image_width"]
        fmod = sub("forward")
        seen, fmod._backward_seen = fmod._backward_seen, True     # the trainer's state from its second step on: the forward clears the backward's workspace
        try:
            fwd = gsr.render_gaussians(**kw)[2]
        finally:
            fmod._backward_seen = seen                             # (the process's own state: later tests find it as it was)
        for k in ("radii", "point_list", "ranges"):
            parity.assert_exact(k, fwd[k], c["buf"][k])
        nb = _np_buf(fwd)
        dpix, gD, gA = T.cotangents(H, W, aux=True)
        on_tile, bt, ba = T.block_collector(int(nb["point_list"].shape[0]), nb["ranges"])
        ref = B.of_buffers(nb, kw["background"], W, H, dpix, on_tile=on_tile)
        mask = ref["mask"]
        print(f"\n{name}: {mask.mean():.5f} of the pixels masked ({int((ref['margin'] < B.NEAR).sum())} near a threshold, "
              f"{int((ref['n_contrib'] != nb['n_contrib'].reshape(H, W)).sum())} with another n_contrib than float64's)")
        assert mask.mean() <= T.MAX_MASKED
        cot = B.masked(mask, dpix, gD, gA)
        _SIDE[name] = dict(c=c, fwd=fwd, nb=nb, ref=ref, cot=cot, mask=mask, blk_active=ba, ref_aux=None)
    return _SIDE[name]


def aux_ref(s):
    if s["ref_aux"] is None:
        kw = s["c"]["kw"]
        s["ref_aux"] = B.of_buffers(s["nb"], kw["background"], kw["image_width"], kw["image_height"], *T.cotangents(kw["image_height"], kw["image_width"], aux=True))
        assert np.array_equal(s["ref_aux"]["mask"], s["mask"])
    return s["ref_aux"]


def _bkw(c, buf, dpix, packed=False):
    b = backward_kwargs(c["sc"], c["cam"], c["kw"], buf, dpix)
    if packed:       # copies of the three arrays: the records are re-packed, with 1/depth from the forward's depths
        for k in ("means2D", "conic_opacity", "rgb"):
            b[k] = b[k].clone()
        b["geom_buffer"] = dict(b["geom_buffer"], means2D=b["means2D"], conic_opacity=b["conic_opacity"], rgb=b["rgb"], depths=buf["depths"])
    else:
        b["geom_buffer"] = dict(b["geom_buffer"], depths=buf["depths"])
    return b


def _got(g, key):
    if key == "dL_dmean2D_abs":
        return parity.to_np(g[key]).astype(np.float64).reshape(-1, 2)
    if key == "payload":
        return parity.to_np(g[key]).astype(np.float64).reshape(-1, 3)
    return B.kernel_layout(g, key)


def _ref_of(ref, key):
    if key == "dL_dmean2D_abs":
        r = ref["dL_dmean2D"]
        return {"signed": r["abs"], "abs": r["abs"], "scale": r["scale"]}
    return ref[key]


def judge(name, path, g, g_again, ref, E_oracle, keys):
    """Print and assert the criterion for one backward result (and its repeat, for the spread)."""
    floor = T.golden()["floor"]
    bad = []
    for k in keys:
        r = _ref_of(ref, k)
        ok = E_ORACLE_OF.get(k, k)
        E_k = max(B.worst(_got(g, k), r), B.worst(_got(g_again, k), r))
        d = np.abs(_got(g, k) - _got(g_again, k))
        E_s = float((d[r["scale"] > 0] / r["scale"][r["scale"] > 0]).max()) if (r["scale"] > 0).any() else 0.0
        row = dict(case=name, path=path, block=os.environ.get("GSR_BWD_BLOCK", "auto"), array=k, E_oracle=E_oracle[ok], E_spread=E_s, E_kernel=E_k,
                   floor=floor[ok], bound=3.0 * max(E_oracle[ok], E_s) + floor[ok])
        print("BLEND_GRAD_ROW " + json.dumps(row))
        if not T.criterion(E_k, E_oracle[ok], E_s, floor[ok]):
            e = B.errors(_got(g, k), r)
            bad.append((k, E_k, row["bound"], int(np.argmax(e))))
    assert not bad, f"{name} / {path}: (array, E_kernel, bound, worst Gaussian) {bad}"


@pytest.mark.parametrize("name", CASES)
def test_own_chain_and_copies(oracle, cameras, name):
    gsr, bwd = pkg(), sub("backward").backward
    s = kernel_side(oracle, cameras, name)
    c, E_o = s["c"], T.oracle_side(oracle, cameras, name)["E"]
    dpm = s["cot"][0]
    g = gsr.backward(**_bkw(c, s["fwd"], dpm))
    assert bwd.last_call_used_forward_records and bwd.last_call_used_forward_masks and bwd.last_call_skipped_the_clear
    snap = {k: parity.to_np(g[k]).copy() for k in T.PLAIN}
    g2 = gsr.backward(**_bkw(c, s["fwd"], dpm))
    assert bwd.last_call_used_forward_records and bwd.last_call_used_forward_masks and not bwd.last_call_skipped_the_clear
    judge(name, "own chain", snap, g2, s["ref"], E_o, T.PLAIN)
    p1 = gsr.backward(**_bkw(c, s["fwd"], dpm, packed=True))
    assert not bwd.last_call_used_forward_records and not bwd.last_call_used_forward_masks
    snap = {k: parity.to_np(p1[k]).copy() for k in T.PLAIN}
    p2 = gsr.backward(**_bkw(c, s["fwd"], dpm, packed=True))
    judge(name, "copies", snap, p2, s["ref"], E_o, T.PLAIN)


@pytest.mark.parametrize("name", list(T.DESIGNED))
def test_aux_and_absgrad(oracle, cameras, name):
    gsr, bwd = pkg(), sub("backward").backward
    s = kernel_side(oracle, cameras, name)
    c, E_o = s["c"], T.oracle_side(oracle, cameras, name)["E"]
    dpm, gDm, gAm = s["cot"]
    ref = aux_ref(s)
    keys = B.OUTPUTS + ("dL_dmean2D_abs",)
    for packed in (False, True):
        run = lambda: gsr.backward(**_bkw(c, s["fwd"], dpm, packed), dL_ddepth_image=gDm, dL_dalpha_image=gAm, absgrad=True)
        g = run()
        assert bwd.last_call_used_forward_masks is (not packed)
        snap = {k: parity.to_np(g[k]).copy() for k in keys}
        judge(name, "aux + abs, " + ("copies" if packed else "own chain"), snap, run(), ref, E_o, keys)


def test_factored_payload(oracle, cameras):
    name = "designed_97x61"
    gsr = pkg()
    s = kernel_side(oracle, cameras, name)
    c, E_o = s["c"], T.oracle_side(oracle, cameras, name)["E"]
    N = c["sc"]["means"].shape[0]
    # a payload row is the Gaussian's dL_dcolor with the clamped channels zeroed (what the SH stage multiplies the basis with)
    keep = 1.0 - s["nb"]["clamped_state"].reshape(N, 3).astype(np.float64)
    ref = dict(s["ref"], payload={k: v * keep for k, v in s["ref"]["dL_dcolor"].items()})
    assert (keep == 0).any() and np.abs(ref["payload"]["signed"]).max() > 0

    def run():
        got = []
        g = gsr.backward(**_bkw(c, s["fwd"], s["cot"][0]), sh_gradient="factored", on_payload=lambda p: got.append(p[:3 * N].view(N, 3).clone()))
        assert len(got) == 1 and g["dL_dshs"] is None
        assert torch.equal(got[0], g["_view_payload"][:3 * N].view(N, 3))
        return {"payload": parity.to_np(got[0]).astype(np.float64), "dL_dcolor": parity.to_np(g["dL_dcolor"]).copy(),
                "dL_dopacity": parity.to_np(g["dL_dopacity"]).copy()}
    judge(name, "factored payload", run(), run(), ref, dict(E_o, payload=E_o["dL_dcolor"]), ("payload", "dL_dcolor", "dL_dopacity"))


def test_capacity_mode_frame(oracle, cameras):
    name = "designed_100x70"
    gsr = pkg()
    s = kernel_side(oracle, cameras, name)
    c, E_o = s["c"], T.oracle_side(oracle, cameras, name)["E"]
    D = int(s["nb"]["point_list"].shape[0])
    K = D + D // 3 + 5
    cbuf = sub("forward").render_gaussians(**c["kw"], capacity=K, capacity_hint=D)[2]
    assert cbuf["point_list"].shape[0] == K and sub("forward").rendered_count(cbuf) == (D, False)
    assert torch.equal(cbuf["point_list"][:D], s["fwd"]["point_list"]) and torch.equal(cbuf["n_contrib"], s["fwd"]["n_contrib"])
    for k in ("points_xy_image", "conic_opacity", "colors", "depths"):        # the same buffers: the same float64 sums and mask
        assert torch.equal(cbuf[k], s["fwd"][k]), k
    run = lambda: gsr.backward(**_bkw(c, cbuf, s["cot"][0]))
    g = run()
    snap = {k: parity.to_np(g[k]).copy() for k in T.PLAIN}
    judge(name, f"capacity K = {K} > D = {D}", snap, run(), s["ref"], E_o, T.PLAIN)


def test_nothing_visible(oracle, cameras):
    gsr = pkg()
    c = T.get_case(oracle, cameras, "nothing_visible")
    kw = c["kw"]
    H, W = kw["image_height"], kw["image_width"]
    buf = gsr.render_gaussians(**kw)[2]
    assert int(buf["point_list"].shape[0]) == 0
    dpix, gD, gA = T.cotangents(H, W, aux=True)
    ref = B.of_buffers(_np_buf(buf), kw["background"], W, H, dpix, gD, gA)
    assert not ref["mask"].any()
    for extra in ({}, dict(dL_ddepth_image=gD, dL_dalpha_image=gA, absgrad=True)):
        g = gsr.backward(**_bkw(c, buf, dpix), **extra)
        for k in (B.OUTPUTS + ("dL_dmean2D_abs",)) if extra else T.PLAIN:
            assert B.worst(_got(g, k), _ref_of(ref, k)) == 0.0, k              # every scale is zero: exactly zero gradients


@pytest.mark.parametrize("name", CASES)
def test_forward_block_masks_cover_every_active_term(oracle, cameras, name):
    s = kernel_side(oracle, cameras, name)
    kw = s["c"]["kw"]
    H, W = kw["image_height"], kw["image_width"]
    masks = parity.to_np(s["fwd"]["point_list"]._gsr_block_masks[0])
    ranges = s["nb"]["ranges"].reshape(-1, 2)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nc = np.zeros((gy * 16, gx * 16), np.int64)
    nc[:H, :W] = s["nb"]["n_contrib"].reshape(H, W)
    tmax = nc.reshape(gy, 16, gx, 16).max((1, 3)).reshape(-1)
    judged = missing = 0
    for t, (a, b) in enumerate(ranges):
        n = min(int(tmax[t]), int(b - a))                  # the written prefix (see the module docstring)
        need = s["blk_active"][a:a + n]
        bits = (masks[a:a + n, None] >> np.arange(8)[None, :]) & 1
        judged += int(need.sum())
        missing += int((need & (bits == 0)).sum())
    print(f"\n{name}: {judged} (entry, 8x4 block) pairs with an active float64 term at an unmasked pixel, {missing} without their mask bit")
    assert judged > 0 and missing == 0


@pytest.mark.parametrize("px", [32, 64])
def test_each_block_shape(px):
    env = dict(os.environ, GSR_BWD_BLOCK=str(px))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "own_chain or aux_and or factored or capacity_mode or nothing"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("BLEND_GRAD_ROW")]
    print("\n".join(lines))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    # the child ran every criterion test on every case with the variable in place (whatever CASES and DESIGNED hold), none skipped
    rows = [json.loads(l[len("BLEND_GRAD_ROW "):]) for l in lines]
    assert rows and all(row["block"] == str(px) for row in rows)
    for path, cases in (("own chain", CASES), ("copies", CASES), ("aux + abs, own chain", T.DESIGNED), ("aux + abs, copies", T.DESIGNED)):
        assert {row["case"] for row in rows if row["path"] == path} == set(cases), path
    assert any(row["path"] == "factored payload" for row in rows) and any(row["path"].startswith("capacity") for row in rows)
    assert not re.search(r"\d+ skipped", r.stdout), r.stdout[-2000:]
