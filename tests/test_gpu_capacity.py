"""Capacity-mode forward (include/gsr_capacity.h) against the sized path on the same inputs: the same integer outputs and
bit-identical images for every capacity K >= D, zeros for a frame without pairs, every write inside the K-sized buffers when
D > K (guard tails), no host wait, and a trainer run that overflows on purpose and recovers.  These are the cases at the
workload's own sizes and tiers; K and D at block edges, K alone crossing a tier, dirty buffers, frame sequences and the forced
GSR_DEBUG paths on small frames are in tests/test_gpu_capacity_edges.py."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, lego_camera, render_kwargs, sub
import parity

pytestmark = pytest.mark.gpu

BO_FLAG = 8 * 32 * 16      # gsr_internal.h GSR_BO_FLAG: the block order's "filed" word (the forward chose 8x4 blocks)


def _scene(kind, dev):
    gsr = sub("scenes")
    cams = sub("cameras")
    if kind == "c0":        # the reference trainer's start: small-depth path, D >= 20 N (8x8 backward blocks)
        P = sub("densify").init_gaussian_params(5000, 0.1, dev)
        sc = {"means": P["positions"], "scales": P["scales"], "rotations": P["rotations"], "opacities": P["opacities"], "shs": P["shs"]}
        return sc, lego_camera(cams, 0, 800, 800)
    if kind == "c2":        # 32-bit tile items, 8x4 backward blocks
        cfg = gsr.CONFIGS["C2"]
        return gsr.synthetic_scene(cfg["n"], cfg["scale_median"], cfg["scale_sigma"], cfg["seed"]), lego_camera(cams, 0, 800, 800)
    # 1920 x 1080 with more than 2^19 Gaussians: 13 tile bits + 20 id bits -> 64-bit items, narrowed by the first partition pass
    return gsr.synthetic_scene(600_000, 0.006, 0.6, 11), lego_camera(cams, 0, 1920, 1080)


def _to_dev(sc, dev):
    return {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(v, np.float32)).to(dev)) for k, v in sc.items()}


def _render(kw, **cap):
    gsr = sub("forward")
    return gsr.render_gaussians(**kw, **cap)


def _grads(sc, cam, kw, buf, dpix):
    return sub("backward").backward(**backward_kwargs(sc, cam, kw, buf, dpix))


def _same_ints(got, ref, D):
    for k in ("ranges", "n_contrib", "radii", "point_offsets"):
        assert torch.equal(got[k], ref[k]), k
    assert torch.equal(got["point_list"][:D], ref["point_list"]), "point_list"


def _staged_entries(buf, H, W):
    """List positions whose block mask the forward blend wrote: per tile, the entries up to its largest n_contrib."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nc = torch.zeros((gy * 16, gx * 16), dtype=torch.int64, device=buf["n_contrib"].device)
    nc[:H, :W] = buf["n_contrib"]
    tmax = nc.view(gy, 16, gx, 16).amax(dim=(1, 3)).reshape(-1)
    rg = buf["ranges"].to(torch.int64)
    lengths = torch.minimum(tmax, rg[:, 1] - rg[:, 0])
    first = torch.repeat_interleave(rg[:, 0], lengths)
    offs = torch.arange(first.numel(), device=first.device) - torch.repeat_interleave(torch.cumsum(lengths, 0) - lengths, lengths)
    return first + offs


def _same_floats(g, r):
    (gi, gd, gb), (ri, rd, rb) = g, r
    assert torch.equal(gi, ri) and torch.equal(gd, rd) and torch.equal(gb["final_Ts"], rb["final_Ts"])


@pytest.mark.parametrize("kind", ["c0", "c2", "hd"])
def test_capacity_mode_matches_the_sized_path(kind):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sc, cam = _scene(kind, dev)
    sc = _to_dev(sc, dev)
    kw = render_kwargs(sc, cam)
    sub("forward")._backward_seen = True            # the trainer's state: the forward pre-clears the backward workspace
    ref = _render(kw)
    D = int(ref[2]["point_list"].shape[0])
    N = int(sc["means"].shape[0])
    assert D > 0
    if kind == "c0":
        assert D >= 20 * N                          # the 8x8-block backward
    if kind == "c2":
        assert D < 20 * N
    H, W = kw["image_height"], kw["image_width"]
    dpix = torch.as_tensor((np.random.default_rng(1).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)).to(dev)
    g_ref = _grads(sc, cam, kw, ref[2], dpix)
    filed_ref = int(ref[2]["point_list"]._gsr_block_masks[2][BO_FLAG])
    assert filed_ref == (0 if kind in ("c0", "hd") else 1)
    for K in (D, D + 1, 2 * D + 17):
        got = _render(kw, capacity=K, capacity_hint=D)
        assert got[2]["point_list"].shape[0] == K and sorted(got[2]) == sorted(ref[2])
        assert sub("forward").rendered_count(got[2]) == (D, False)
        _same_ints(got[2], ref[2], D)
        _same_floats(got, ref)
        m_got, m_ref = got[2]["point_list"]._gsr_block_masks[0], ref[2]["point_list"]._gsr_block_masks[0]
        pos = _staged_entries(ref[2], H, W)           # (entries behind a tile's saturation batch are never written: undefined)
        assert torch.equal(m_got[pos], m_ref[pos]), "block_masks"
        # forward and backward agree on the block shape: the forward filed the 8x4 blocks exactly when the sized path did
        assert int(got[2]["point_list"]._gsr_block_masks[2][BO_FLAG]) == filed_ref
        parity.compare_backward(_grads(sc, cam, kw, got[2], dpix), g_ref)
    # a hint far from D costs time, never correctness: both shapes either way
    for hint in (1, 40 * N):
        got = _render(kw, capacity=D + 5, capacity_hint=hint)
        _same_ints(got[2], ref[2], D)
        _same_floats(got, ref)
        parity.compare_backward(_grads(sc, cam, kw, got[2], dpix), g_ref)
    torch.cuda.synchronize()


def test_a_frame_without_pairs_gives_zeros():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cams = sub("cameras")
    cam = lego_camera(cams, 0, 160, 120)
    sc = sub("scenes").synthetic_scene(3000, 0.05, 0.5, 3)
    # every Gaussian behind the camera (the camera looks at the origin): nothing is rendered
    c = np.asarray(cam["camera_center"], np.float64)
    sc["means"] = (c[None, :] * 1.5 + 0.1 * np.asarray(sc["means"], np.float64)).astype(np.float32)
    sc = _to_dev(sc, dev)
    kw = render_kwargs(sc, cam, bg=(0.3, 0.5, 0.7))
    sub("forward")._backward_seen = True
    ref = _render(kw)
    assert ref[2]["point_list"].shape[0] == 0
    dpix = torch.full((120, 160, 3), 1e-3, device=dev)
    g_ref = _grads(sc, cam, kw, ref[2], dpix)
    for K in (0, 5, 1000):
        got = _render(kw, capacity=K)
        assert sub("forward").rendered_count(got[2]) == (0, False)
        for t in (got[0], got[1], got[2]["final_Ts"], got[2]["n_contrib"], got[2]["ranges"]):
            assert not t.any()                       # zeros, not the background (quirk Q10)
        _same_floats(got, ref)
        assert torch.equal(got[2]["ranges"], ref[2]["ranges"]) and torch.equal(got[2]["n_contrib"], ref[2]["n_contrib"])
        g = _grads(sc, cam, kw, got[2], dpix)
        for k in parity.GRAD_KEYS:
            assert torch.equal(torch.as_tensor(g[k]), torch.as_tensor(g_ref[k])), k


@pytest.mark.parametrize("kind", ["c2", "hd"])
def test_an_overflowed_frame_stays_inside_its_buffers(kind):
    """D > K: the call succeeds, the count says so, and the guard tails behind point_list, block_masks and the binning workspace
    are untouched by the forward and by a backward on that frame.  (Bounded by construction: if this ever faults, the
    out-of-range write is to be found from the guards and the code, not by running it again.)"""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = sub("_lib").lib()
    sc, cam = _scene(kind, dev)
    sc = _to_dev(sc, dev)
    kw = render_kwargs(sc, cam)
    ref = _render(kw)
    D, N = int(ref[2]["point_list"].shape[0]), int(sc["means"].shape[0])
    H, W = kw["image_height"], kw["image_width"]
    G = 1 << 16
    dpix = torch.full((H, W, 3), 1e-6, device=dev)
    for K in (0, 1, D - 1, D // 3):
        need = int(L.gsr_binning_workspace_bytes(N, K, W, H))
        pl_all = torch.full((K + G,), -7, dtype=torch.int32, device=dev)
        bm_all = torch.full((K + 16 + G,), 0xA5, dtype=torch.uint8, device=dev)
        bw_all = torch.full((need + G,), 0x5A, dtype=torch.uint8, device=dev)
        guards = lambda: (pl_all[K:].clone(), bm_all[K:].clone(), bw_all[need:].clone())
        before = guards()
        got = _render(kw, capacity=K, capacity_hint=D, capacity_buffers={"point_list": pl_all[:K], "block_masks": bm_all[:K], "binning_ws": bw_all[:need]})
        assert sub("forward").rendered_count(got[2]) == (D, True)
        torch.cuda.synchronize()
        for a, b, name in zip(guards(), before, ("point_list", "block_masks", "binning_ws")):
            assert torch.equal(a, b), f"K={K}: the forward wrote past {name}"
        if K > 0:
            assert int(got[2]["point_list"].min()) >= 0 and int(got[2]["point_list"].max()) < N
        rg = got[2]["ranges"]
        assert int(rg.min()) >= 0 and int(rg.max()) <= min(D, K) and bool((rg[:, 0] <= rg[:, 1]).all())
        _grads(sc, cam, kw, got[2], dpix)
        torch.cuda.synchronize()
        for a, b, name in zip(guards(), before, ("point_list", "block_masks", "binning_ws")):
            assert torch.equal(a, b), f"K={K}: the backward wrote past {name}"
        again = _render(kw)                          # the sized path afterwards: the default path's integers exactly
        assert again[2]["point_list"].shape[0] == D
        _same_ints(again[2], ref[2], D)


def test_capacity_mode_does_not_wait_for_the_device():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sc, cam = _scene("c2", dev)
    sc = _to_dev(sc, dev)
    kw = render_kwargs(sc, cam)
    D = int(_render(kw)[2]["point_list"].shape[0])
    _render(kw, capacity=2 * D, capacity_hint=D)   # warm: the pinned count word and the K-sized workspace exist before the timed call
    torch.cuda.synchronize()
    # calibrate the spin kernel to >= 200 ms
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(10_000_000)
    b.record()
    b.synchronize()
    cycles = int(10_000_000 * max(1.0, 200.0 / max(a.elapsed_time(b), 1e-3)))

    def pending_after(**cap):
        torch.cuda.synchronize()
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record()
        out = _render(kw, **cap)
        still = not ev.query()
        torch.cuda.synchronize()
        return still, out

    still, out = pending_after(capacity=2 * D, capacity_hint=D)
    assert still, "the capacity-mode call waited for the device"
    assert sub("forward").rendered_count(out[2]) == (D, False)
    still, _ = pending_after()
    assert not still, "the sized path is expected to wait for D (behind the spin kernel)"


def test_trainer_with_capacity_retries_and_matches_the_sized_run(tmp_path):
    """300 iterations on the committed Lego views, density control from iteration 100 every 50 (N changes), --capacity from a K of
    1 000 that the first frame overflows.  Bounds: two sized runs of this command drift apart by float-atomic order alone -- measured
    up to 4e-4 (relative) in the loss lines before the first density-control call, 3.9e-3 after it, and 1.6 % in the final point
    count (profiles/capacity_train_lego/README.md) -- so the capacity run is held to 2e-3 before that call, 1e-2
    after it, and 5 % in the point count."""
    def run(extra, log):
        cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--dataset", os.path.join(ROOT, "data", "lego"), "--views", "8",
               "--iterations", "300", "--gaussians", "5000", "--densify-from", "100", "--densify-interval", "50", "--print-interval", "10",
               "--log", str(log)] + extra
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
        lines = [(int(m.group(1)), float(m.group(2))) for m in re.finditer(r"iter\s+(\d+)\s+loss\s+([0-9.eE+-]+)", p.stdout)]
        recs = [json.loads(l) for l in open(log)]
        return lines, recs
    sized, rs = run([], tmp_path / "sized.jsonl")
    capd, rc = run(["--capacity", "--capacity-initial", "1000"], tmp_path / "cap.jsonl")
    retries = [r for r in rc if r["record"] == "capacity_retry"]
    calls = [r for r in rs if r["record"] == "density_control" and r["iteration"] > 0]
    print(f"\n{len(retries)} capacity retries: {retries[:4]}; points after each call: {[r['points'] for r in calls]}")
    print("relative loss differences:", [round(abs(a - b) / max(a, b), 5) for (_, a), (_, b) in zip(sized, capd)])
    assert len(retries) >= 1 and retries[0]["iteration"] == 0 and retries[0]["capacity"] == 1000 and retries[0]["D"] > 1000
    assert len({r["points"] for r in calls}) >= 2                   # N changed, more than once
    assert [i for i, _ in sized] == [i for i, _ in capd] and len(sized) >= 30
    for (i, a), (_, b) in zip(sized, capd):
        assert abs(a - b) <= (2e-3 if i < 100 else 1e-2) * max(a, b), (i, a, b)
    n_s = [r for r in rs if r["record"] == "summary"][0]["points_final"]
    n_c = [r for r in rc if r["record"] == "summary"][0]["points_final"]
    assert abs(n_s - n_c) <= 0.05 * n_s, (n_s, n_c)
