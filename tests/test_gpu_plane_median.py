"""
The plane depth under the median rule (csrc/median_depth.hip, include/gsr_plane_median.h) on the MI355X, against the float32
restatement and the float64 yardstick of tests/plane_median_reference.py.

  1. forward, on median_depth_reference.CASES, all nine (crossings at entry 1, over the first batch, at list positions 255-258, in the
     third batch, never; 8x8 to 64x48), slopes from plane_median_reference.draw_slopes (every case keeps clamped and unclamped chosen
     entries): the contributor image is bit for bit gsr_median_depth_forward's on the same frame; the value is bit for bit the
     restatement's m of the entry the contributor names at EVERY pixel (two fused multiply-adds and a clamp: nothing in it that a
     restatement cannot replay), and outside the tie mask contributor and value are bit for bit the restatement's own walk (inside it
     numpy's exp and the hardware's may lawfully choose neighbouring entries: median_depth_reference says why); outputs pre-filled
     with NaN / -1 are written everywhere; zero slopes give gsr_median_depth_forward's value bit for bit; the bits are the same with
     the case's masks, without masks, all 0xFF and random, on a second call and on a side stream; a frame without lists gives zeros.
  2. backward, all nine cases, g = median_depth_reference.draw_g, fed the REFERENCE's contributor image (an input): per element of the
     moments the error against the float64 yardstick is at most (n + 2) 2^-24 sum |addend|, n the row's addend count -- one rounding in
     dx, one in the product, n - 1 in a sum of any order.  The worst ratio to that bound an MI355X run measured is on file
     (tests/golden/plane_median_margins.json, "backward_ratio": a record only).  The entry point ADDS: rows of Gaussians chosen nowhere,
     or clamped everywhere, keep a seeded buffer's bits, g = 0 and a zero contributor image leave it as it is, stale contributors are
     clipped.  On frame_walk_frames.BACKWARD_SHAPES, where no row takes more than two addends, the bits repeat.
  3. on a rendered frame (the trainer's hidden scene, flattened, at 64x64): render_plane_median_depth agrees with the restatement;
     plane_median_gradients(grads=backward_view(...)) adds exactly what the two per-Gaussian kernels make of its moments, agrees with
     the fresh-tensor result plus the plain gradients, and leaves every other key of grads bit for bit; fuse_views(plane_depth="median")
     on the torus demo's smallest row gives a finite mesh with info["plane_depth"] == "median".
  4. the trainer with --lambda-depth 1 --depth-render plane-median ends finite, with its summary field.  No quality claim and no
     threshold on the torus numbers ("mesh_gap_min": null).

Every measured figure is printed as a PLANE_MEDIAN_ROW JSON line.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg, sub
import frame_walk_frames as FW
import median_depth_reference as M
import plane_depth_reference as PD
import plane_median_reference as PM
import parity

pytestmark = pytest.mark.gpu
f32 = np.float32


def _row(**kw):
    print("\nPLANE_MEDIAN_ROW " + json.dumps(kw))


def _dev(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev)


def _forward(d, slopes, stream=None):
    """(med, contrib) numpy of the kernel on a FW.DeviceFrame, into outputs pre-filled with NaN and -1."""
    med = torch.full((d.H, d.W), float("nan"), dtype=torch.float32, device=d.dev)
    contrib = torch.full((d.H, d.W), -1, dtype=torch.int32, device=d.dev)
    FW._lib.check(d.L.gsr_pmed_forward(C.byref(d.dframe), FW._host.ptr(slopes), FW._host.ptr(med), FW._host.ptr(contrib),
                                       d.stream if stream is None else stream))
    torch.cuda.synchronize()
    return med.cpu().numpy(), contrib.cpu().numpy()


def _centre_forward(d):
    med = torch.full((d.H, d.W), float("nan"), dtype=torch.float32, device=d.dev)
    contrib = torch.full((d.H, d.W), -1, dtype=torch.int32, device=d.dev)
    FW._lib.check(d.L.gsr_median_depth_forward(C.byref(d.dframe), FW._host.ptr(med), FW._host.ptr(contrib), d.stream))
    torch.cuda.synchronize()
    return med.cpu().numpy(), contrib.cpu().numpy()


def _backward(d, slopes, g, contrib, mom):
    g, contrib = _dev(np.asarray(g, f32), d.dev), _dev(np.asarray(contrib, np.int32), d.dev)
    FW._lib.check(d.L.gsr_pmed_backward(C.byref(d.dframe), FW._host.ptr(slopes), FW._host.ptr(g), FW._host.ptr(contrib), FW._host.ptr(mom), d.stream))
    torch.cuda.synchronize()
    return mom.cpu().numpy()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _check_forward(c, got, centre):
    fr, ref, slopes = c["fr"], c["ref"], c["slopes"]
    med, contrib = got
    assert np.isfinite(med).all() and (contrib >= 0).all(), "every pixel is written"
    assert contrib.tobytes() == centre[1].tobytes()                  # c does not depend on the slopes
    ch = PM.chosen(fr, slopes, contrib)
    assert np.array_equal(ch["c"], contrib) and ((ch["ids"] >= 0) == (contrib > 0)).all()      # inside the list, a Gaussian in [0, N)
    assert med.tobytes() == ch["m"].tobytes()                        # every pixel: the header's m of the entry the contributor names
    assert not med[contrib == 0].view(np.uint32).any()
    keep = ~ref["tie"]
    assert ref["tie"].mean() <= M.MAX_TIES
    assert np.array_equal(contrib[keep], c["contrib"][keep]) and med[keep].tobytes() == c["med"][keep].tobytes()
    return ch


@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_against_the_restatement_and_the_centre_median(name):
    c = PM.case(name)
    d = FW.DeviceFrame(c["fr"])
    sd = _dev(c["slopes"], d.dev)
    centre = _centre_forward(d)
    got = _forward(d, sd)
    ch = _check_forward(c, got, centre)
    sel = got[1] > 0
    clamped, moved = int((sel & ch["clamped"]).sum()), int((got[0] != centre[0]).sum())
    _row(test="forward", case=name, pixels=int(sel.size), chosen=int(sel.sum()), clamped=clamped, differs_from_centre_median=moved,
         excused=int(c["ref"]["tie"].sum()), excused_and_different=int((c["ref"]["tie"] & (got[1] != c["contrib"])).sum()))
    assert clamped >= PM.MIN_CLAMPED and moved >= PM.MIN_FREE
    # zero slopes: gsr_median_depth_forward's value, bit for bit
    zero = _forward(d, torch.zeros((d.N, 2), device=d.dev))
    assert _same(zero, centre)


@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_bits_do_not_depend_on_masks_calls_or_streams(name):
    c = PM.case(name)
    base = _forward(FW.DeviceFrame(c["fr"]), _dev(c["slopes"], torch.device("cuda", 0)))          # the case's own masks
    for masks in (None, "ff", "random"):
        fr, _ = M.frame(name, masks=masks)
        d = FW.DeviceFrame(fr)
        sd = _dev(c["slopes"], d.dev)
        assert _same(_forward(d, sd), base), masks
        assert _same(_forward(d, sd), base), (masks, "a second call")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert _same(_forward(d, sd, FW._host.raw_stream(d.dev)), base)


def test_forward_of_a_frame_without_lists_is_zero():
    fr = FW.build_frame(3, 50, 37, lens=(0,), bad_ids=False)
    assert fr["D"] == 0
    d = FW.DeviceFrame(fr)
    sd = _dev(PM.draw_slopes(fr), d.dev)
    med, contrib = _forward(d, sd)
    assert not med.view(np.uint32).any() and not contrib.any()
    seed = torch.rand((d.N, 3), device=d.dev)
    assert np.array_equal(_backward(d, sd, M.draw_g(37, 50), np.ones((37, 50)), seed.clone()), seed.cpu().numpy())      # D = 0: nothing is enqueued


@pytest.mark.parametrize("name", list(M.CASES))
def test_backward_against_float64(name):
    c = PM.case(name)
    fr, ref, slopes = c["fr"], c["ref"], c["slopes"]
    d = FW.DeviceFrame(fr)
    sd = _dev(slopes, d.dev)
    g = M.draw_g(fr["H"], fr["W"])
    ch = PM.chosen(fr, slopes, ref["contrib"])
    r = PM.moments_f64(fr, slopes, g, ref["contrib"], ch)
    zeros = lambda: torch.zeros((d.N, 3), device=d.dev)
    mom = _backward(d, sd, g, ref["contrib"], zeros())
    ratio = PM.bound_ratio(mom, r)
    rec = PM.golden()["backward_ratio"].get(name)
    chosen_rows = np.zeros(fr["N"], bool)
    chosen_rows[ch["ids"][ch["ids"] >= 0]] = True
    clamped_everywhere = int((chosen_rows & (r["count"] == 0)).sum())
    _row(test="backward", case=name, ratio_to_bound=ratio, recorded=rec, rows=int((r["count"] > 0).sum()), max_addends=int(r["count"].max()),
         rows_clamped_everywhere=clamped_everywhere)
    assert (r["count"] > 0).sum() >= 3 and np.abs(mom).max() > 0 and np.isfinite(mom).all()
    assert ratio <= 1.0, ratio
    # the entry point ADDS: untouched rows keep a seeded buffer's bits, the others move by the same sums
    seed = (np.random.default_rng(2).normal(0, 1, (fr["N"], 3)) * 1e-3).astype(f32)
    seeded = _backward(d, sd, g, ref["contrib"], _dev(seed, d.dev))
    idle = r["count"] == 0
    assert idle.sum() >= 100 and seeded[idle].tobytes() == seed[idle].tobytes()
    plus_seed = dict(signed=r["signed"] + seed, abs=r["abs"] + np.abs(seed), count=r["count"] + 1)
    assert PM.bound_ratio(seeded, plus_seed) <= 1.0
    # g = 0 leaves the buffer as it is, and so does a contributor image of zeros
    assert _backward(d, sd, np.zeros_like(g), ref["contrib"], _dev(seed, d.dev)).tobytes() == seed.tobytes()
    assert _backward(d, sd, g, np.zeros_like(ref["contrib"]), _dev(seed, d.dev)).tobytes() == seed.tobytes()
    # zero slopes: nothing is clamped, and column 0 is the centre median's scatter of g
    flat = _backward(d, torch.zeros((d.N, 2), device=d.dev), g, ref["contrib"], zeros())
    r0 = PM.moments_f64(fr, np.zeros_like(slopes), g, ref["contrib"])
    signed, scale = M.gradient_f64(fr, ref, g)
    assert np.abs(r0["signed"][:, 0] - signed).max() <= 1e-12 * scale.max() and r0["count"].sum() == (ref["contrib"] > 0).sum()
    assert PM.bound_ratio(flat, r0) <= 1.0
    # stale contributors: past the list, negative -- clipped to the tile's range, never out of bounds, finite
    wild = np.where(np.random.default_rng(1).random(g.shape) < 0.5, 1 << 30, -5).astype(np.int32)
    assert np.isfinite(_backward(d, sd, g, wild, zeros())).all()


@pytest.mark.parametrize("tag", list(FW.BACKWARD_SHAPES))
def test_backward_bits_repeat_where_no_row_takes_more_than_two_addends(tag):
    seeded = tag == "8x8"                               # one wave adds: a seeded buffer takes one addend per destination
    fr = FW.build_frame(11, lens=(640,), once_per_tile=True, **FW.BACKWARD_SHAPES[tag])
    fr["co"][:, 3] *= 0.35
    d = FW.DeviceFrame(fr)
    slopes = PM.draw_slopes(fr)
    sd = _dev(slopes, d.dev)
    med, contrib = _forward(d, sd)
    assert (contrib > 0).sum() >= 20
    g = M.draw_g(fr["H"], fr["W"])
    seed = (np.random.default_rng(2).normal(0, 1, (fr["N"], 3)) * 1e-3).astype(f32) if seeded else np.zeros((fr["N"], 3), f32)
    first = _backward(d, sd, g, contrib, _dev(seed, d.dev))
    assert np.isfinite(first).all() and (first != seed).any(1).sum() >= 5
    for _ in range(2):
        assert _backward(d, sd, g, contrib, _dev(seed, d.dev)).tobytes() == first.tobytes()
    assert _backward(FW.DeviceFrame(FW.other_bad_ids(fr, 5)), sd, g, contrib, _dev(seed, d.dev)).tobytes() == first.tobytes()
    if not seeded:
        assert PM.bound_ratio(first, PM.moments_f64(fr, slopes, g, contrib)) <= 1.0


# ---- on a rendered frame ----
_RENDERED = {}


def rendered():
    """examples/train.py's hidden scene with its Gaussians flattened (plane_depth_reference.plane_scales: most take the plane branch),
    2 000 of them at 64x64, drawn by render_view; the frame dict the references read, once per session."""
    if not _RENDERED:
        gsr = pkg()
        dev = torch.device("cuda", 0)
        size, N = 64, 2000
        sc = gsr.scenes.synthetic_scene(N, 0.05, 0.5, seed=7)
        P = {"positions": _dev(sc["means"], dev), "scales": _dev(PD.plane_scales(sc["scales"]), dev), "rotations": _dev(sc["rotations"], dev),
             "opacities": _dev(sc["opacities"], dev), "shs": _dev(sc["shs"], dev)}
        cam = gsr.cameras.nerf_camera(gsr.scenes.orbit_pose(0, 8), size, size, gsr.scenes.LEGO_CAMERA_ANGLE_X)
        bg = np.zeros(3, f32)
        image, depth, buf = gsr.render_view(P, cam, bg)
        nb = {k: parity.to_np(buf[k]) for k in ("points_xy_image", "conic_opacity", "point_list", "ranges", "n_contrib")}
        invd = parity.to_np(sub("_frame").inv_depth_of(buf, N, dev)).astype(f32)
        fr = PD.frame_of_buffers(nb, size, size, invd)
        _RENDERED.update(P=P, cam=cam, bg=bg, buf=buf, fr=fr, ref=M.median_f64(fr), H=size, W=size, N=N, dev=dev,
                         g=(M.draw_g(size, size) / (size * size)).astype(f32))
    return _RENDERED


def test_render_plane_median_depth_on_a_rendered_frame():
    pd, med_mod = sub("plane_depth"), sub("median_depth")
    f = rendered()
    H, W, N, buf, fr, ref = f["H"], f["W"], f["N"], f["buf"], f["fr"], f["ref"]
    med, contrib, s, n = pd.render_view_plane_median_depth(f["P"], f["cam"], buf)
    assert med.dtype == torch.float32 and contrib.dtype == torch.int32 and tuple(med.shape) == tuple(contrib.shape) == (H, W) and tuple(s.shape) == (N, 2)
    centre = med_mod.render_median_depth(buf, H, W)
    assert torch.equal(contrib, centre[1])
    assert torch.equal(pd.render_plane_median_depth(torch.zeros_like(s), buf, H, W)[0], centre[0])
    sl, mk, ck = parity.to_np(s), parity.to_np(med), parity.to_np(contrib).astype(np.int64)
    share = float((sl != 0).any(1).mean())
    ch = PM.chosen(fr, sl, ck)
    assert mk.tobytes() == ch["m"].tobytes()
    m32, c32, _ = PM.forward_f32(fr, sl)
    keep = ~ref["tie"]
    assert ref["tie"].mean() <= M.MAX_TIES and (ck > 0).mean() > 0.5 and share > 0.5
    assert np.array_equal(ck[keep], c32[keep]) and mk[keep].tobytes() == m32[keep].tobytes()
    _row(test="rendered", plane_branch=share, chosen=int((ck > 0).sum()), clamped=int(ch["clamped"].sum()),
         differs_from_centre_median=int((mk != parity.to_np(centre[0])).sum()))
    assert (mk != parity.to_np(centre[0])).sum() > 500
    out = (torch.full((H, W), float("nan"), device=f["dev"]), torch.full((H, W), -1, dtype=torch.int32, device=f["dev"]))
    got = pd.render_plane_median_depth(s, buf, H, W, out=out, use_block_masks=False)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], med) and torch.equal(out[1], contrib)
    z = med_mod.view_depth(med, buf["final_Ts"].reshape(H, W))
    assert bool(torch.isfinite(z).all()) and bool((z >= 0).all()) and bool((z > 0).any())


def test_plane_median_gradients_add_into_a_backward_view_result():
    gsr = pkg()
    pd, nr, dist = sub("plane_depth"), sub("normal_render"), sub("dist")
    f = rendered()
    H, W, N, buf, fr, P, cam, dev = f["H"], f["W"], f["N"], f["buf"], f["fr"], f["P"], f["cam"], f["dev"]
    med, contrib, s, n = pd.render_view_plane_median_depth(P, cam, buf)
    gd = _dev(f["g"], dev)
    dpix = (np.random.default_rng(3).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(f32)
    # the moments against the yardstick, cleared by default and added to on request
    r = PM.moments_f64(fr, parity.to_np(s), f["g"], parity.to_np(contrib))
    mom = pd.plane_median_depth_backward(gd, contrib, s, buf, H, W)
    ratio = PM.bound_ratio(parity.to_np(mom), r)
    _row(test="rendered_backward", ratio_to_bound=ratio, rows=int((r["count"] > 0).sum()), max_addends=int(r["count"].max()))
    assert ratio <= 1.0 and (r["count"] > 0).sum() > 100
    poisoned = torch.full((N, 3), 7.0, device=dev)
    assert pd.plane_median_depth_backward(gd, contrib, s, buf, H, W, out=poisoned) is poisoned
    assert PM.bound_ratio(parity.to_np(poisoned), r) <= 1.0                                   # cleared first
    twice = pd.plane_median_depth_backward(gd, contrib, s, buf, H, W, out=mom.clone(), accumulate=True)
    assert PM.bound_ratio(0.5 * parity.to_np(twice).astype(np.float64), r) <= 1.5            # added to: twice the sums
    # fresh tensors
    dmean_f, drot_f, mom_f = pd.plane_median_gradients(P, cam, buf, gd, contrib, s, n)
    assert tuple(dmean_f.shape) == (N, 3) and tuple(drot_f.shape) == (N, 4) and bool(dmean_f.any()) and bool(drot_f.any())
    assert bool(torch.isfinite(dmean_f).all()) and bool(torch.isfinite(drot_f).all())
    # into a backward_view result: exactly what the two per-Gaussian kernels make of the call's own moments, added in float32
    plain = gsr.backward_view(P, cam, f["bg"], buf, dpix)
    grads = gsr.backward_view(P, cam, f["bg"], buf, dpix)
    before = {k: v.clone() for k, v in grads.items() if isinstance(v, torch.Tensor)}
    dmean, drot, mom_g = pd.plane_median_gradients(P, cam, buf, gd, contrib, s, n, grads=grads)
    assert dmean is grads["dL_dmean3D"] and drot is grads["dL_drot"]
    want_mean, dn = pd.plane_slopes_backward(mom_g, n, P["scales"], P["positions"], cam)
    want_rot = nr.gaussian_normals_backward(dn, P["scales"], P["rotations"], P["positions"], cam)
    assert torch.equal(grads["dL_dmean3D"], before["dL_dmean3D"] + want_mean) and torch.equal(grads["dL_drot"], before["dL_drot"] + want_rot)
    assert float((grads["dL_dmean3D"] - before["dL_dmean3D"]).abs().max()) > 0 and float((grads["dL_drot"] - before["dL_drot"]).abs().max()) > 0
    # ... which is the fresh-tensor result plus the plain gradients (another run of the same atomics: to the gradients' tolerance)
    parity.assert_grad("dL_dmean3D", grads["dL_dmean3D"], plain["dL_dmean3D"] + dmean_f)
    parity.assert_grad("dL_drot", grads["dL_drot"], plain["dL_drot"] + drot_f)
    # every other key keeps its bits; the arena a trainer hands on carries the two sums (they are views of it)
    o = [int(x) for x in dist.arena_offsets(N)]
    for k, v in before.items():
        if k not in ("dL_dmean3D", "dL_drot", "_arena"):
            assert torch.equal(grads[k], v), k
    assert set(grads) == set(plain)
    arena = grads["_arena"]
    assert torch.equal(arena[o[0]:o[0] + 3 * N].view(N, 3), grads["dL_dmean3D"]) and torch.equal(arena[o[2]:o[2] + 4 * N].view(N, 4), grads["dL_drot"])
    assert torch.equal(arena[o[1]:o[2]], before["_arena"][o[1]:o[2]]) and torch.equal(arena[o[3]:], before["_arena"][o[3]:])


# ---- the workflow ----
def test_flat_torus_gives_a_mesh_with_the_plane_depth_under_the_median_rule():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from eval_mesh import demo_torus
    gsr = pkg()
    m = demo_torus(gsr, 64, 8, 100_000, 256, seed=0, log=lambda s: None, depth_mode="plane-median", flat=0.1)      # the README's first row
    assert m["triangles"] > 0 and m["vertices"] > 0 and m["depth_mode"] == "plane-median" and m["flat"] == 0.1 and m["plane_depth"] == "median"
    for k in ("accuracy", "completeness", "chamfer", "accuracy_voxels", "completeness_voxels"):
        assert np.isfinite(m[k]) and m[k] >= 0, (k, m[k])
    _row(test="torus", accuracy_voxels=m["accuracy_voxels"], completeness_voxels=m["completeness_voxels"], triangles=m["triangles"])
    assert PM.golden()["mesh_gap_min"] is None                      # no threshold on the torus rows (README "Plane depth under the median rule")
    P = {"positions": torch.zeros((4, 3), device="cuda"), "scales": torch.ones((4, 3), device="cuda"), "rotations": torch.zeros((4, 4), device="cuda")}
    with pytest.raises(ValueError, match="plane_depth='median'"):
        gsr.tsdf.fuse_views(lambda c: None, [{}], depth_mode="median", plane_depth="median", params=P)


def test_trainer_runs_with_the_plane_median_depth_term(tmp_path):
    log = tmp_path / "plane_median.jsonl"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--log", str(log), "--print-interval", "1000", "--size", "100",
                        "--views", "8", "--iterations", "300", "--lambda-depth", "1", "--depth-render", "plane-median"],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    s = [json.loads(line) for line in open(log)]
    s = [r for r in s if r["record"] == "summary"][0]
    assert all(s["parameters_finite"].values()) and s["depth_render"] == "plane-median"
    for k in ("train_psnr_mean", "train_depth_l1_mean", "train_plane_median_depth_l1_mean"):
        assert np.isfinite(s[k]), k
    _row(test="trainer", psnr=s["train_psnr_mean"], depth_l1=s["train_depth_l1_mean"], plane_median_depth_l1=s["train_plane_median_depth_l1_mean"])
