"""
The median inverse depth (csrc/median_depth.hip, include/gsr_median_depth.h) on the MI355X, against the float64 statement of
tests/median_depth_reference.py.

  1. forward, over the frame matrix (crossings at entry 1, over the first batch, at list positions 255-258, in the third batch,
     never; n_contrib cuts, indefinite conics, out-of-range ids where the median would have been; 8x8 to 64x48; record views): at the
     pixels outside the tie mask median_contrib is the reference's and median_inv_depth is inv_depth[id] bit for bit; the tie mask
     covers at most 1 % of a frame; outputs pre-filled with NaN / -1 are written everywhere; at EVERY pixel, excused or not, the value
     is exactly the inverse depth of the entry the contributor names; the bits are the same with masks NULL, all 0xFF and random
     (random bytes that keep the forward's promise, see the reference), twice in a row, and on another stream.
  2. backward, fed the REFERENCE's contributor image (an input: the forward's ties stay out of it): column 11 against the float64
     scatter-add per Gaussian in units of its sum of |g|.  The a priori bound is ADDENDS eps32: a Gaussian's column is a chain of at
     most `addends` float32 additions (its pixels inside the blocks, then one atomic per block), each off by at most eps32 / 2 of a
     partial sum that is at most sum |g|; the tripwire is 10 x what an MI355X run measured (tests/golden/median_depth_margins.json,
     tools/record_median_depth_margins.py).  Columns 0-10 and 12-15 of a seeded array keep their bits; g = 0 leaves the array as it
     is; the bits repeat on frame_walk_frames.BACKWARD_SHAPES.
  3. through backward_view on a rendered frame (2 000 Gaussians, 64x48): dL_dinv_depths of the median term alone is the scatter;
     together with dL_dpixels the colour columns are the plain call's; camera_grad and sh_gradient="factored" agree with the dense call.
  4. the torus demo, small, in both depth modes: a non-empty, finite mesh with finite accuracy and completeness.  (No threshold on
     the gap between the modes: "mesh_gap_min" in the golden file is null, see README "Median depth".)
  5. the trainer with --lambda-depth 1 --depth-render median ends finite, with its summary fields.  No quality claim.

Every measured figure is printed as a MEDIAN_DEPTH_ROW JSON line.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, backward_kwargs, pkg, sub
import frame_walk_frames as FW
import median_depth_reference as M
import parity

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)


def _row(**kw):
    print("\nMEDIAN_DEPTH_ROW " + json.dumps(kw))


def _forward(d, stream=None):
    """(med, contrib) numpy of the kernel on a FW.DeviceFrame, into outputs pre-filled with NaN and -1."""
    med = torch.full((d.H, d.W), float("nan"), dtype=torch.float32, device=d.dev)
    contrib = torch.full((d.H, d.W), -1, dtype=torch.int32, device=d.dev)
    FW._lib.check(d.L.gsr_median_depth_forward(C.byref(d.dframe), FW._host.ptr(med), FW._host.ptr(contrib), d.stream if stream is None else stream))
    torch.cuda.synchronize()
    return med.cpu().numpy(), contrib.cpu().numpy()


def _backward(d, g, contrib, acc):
    g = torch.as_tensor(np.ascontiguousarray(g, np.float32)).to(d.dev)
    contrib = torch.as_tensor(np.ascontiguousarray(contrib, np.int32)).to(d.dev)
    FW._lib.check(d.L.gsr_median_depth_backward(C.byref(d.dframe), FW._host.ptr(g), FW._host.ptr(contrib), FW._host.ptr(acc), d.stream))
    torch.cuda.synchronize()
    return acc.cpu().numpy()


def _check_forward(fr, ref, med, contrib):
    H, W = fr["H"], fr["W"]
    assert np.isfinite(med).all() and (contrib >= 0).all(), "every pixel is written"
    # every pixel, excused or not: the value is the inverse depth of the entry the contributor names, bit for bit; 0 / 0 otherwise
    gx = (W + 15) // 16
    ys, xs = np.nonzero(contrib > 0)
    tiles = (ys // 16) * gx + xs // 16
    assert (contrib[ys, xs] <= np.asarray(fr["tile_len"])[tiles]).all()
    ids = fr["point_list"][fr["starts"][tiles] + contrib[ys, xs] - 1]
    assert ((ids >= 0) & (ids < fr["N"])).all()
    assert med[ys, xs].tobytes() == fr["invd"][ids].tobytes()
    assert not med[contrib == 0].view(np.uint32).any()
    keep = ~ref["tie"]
    assert ref["tie"].mean() <= M.MAX_TIES
    wrong = keep & (contrib != ref["contrib"])
    assert not wrong.any(), (int(wrong.sum()), contrib[wrong][:5], ref["contrib"][wrong][:5])
    assert med[keep].tobytes() == ref["med"][keep].tobytes()


@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_against_float64(name):
    fr, ref = M.frame(name)
    med, contrib = _forward(FW.DeviceFrame(fr))
    _check_forward(fr, ref, med, contrib)
    _row(test="forward", case=name, pixels=int(ref["tie"].size), excused=int(ref["tie"].sum()),
         excused_and_different=int((ref["tie"] & (contrib != ref["contrib"])).sum()), chosen=int((contrib > 0).sum()))


@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_bits_do_not_depend_on_masks_calls_or_streams(name):
    base = None
    for masks in (None, "ff", "random"):
        fr, ref = M.frame(name, masks=masks)
        d = FW.DeviceFrame(fr)
        got = _forward(d)
        base = base or got
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), masks
        again = _forward(d)
        assert again[0].tobytes() == base[0].tobytes() and again[1].tobytes() == base[1].tobytes(), (masks, "a second call")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = _forward(d, FW._host.raw_stream(d.dev))
    assert other[0].tobytes() == base[0].tobytes() and other[1].tobytes() == base[1].tobytes()
    if name in M.BATCH_EDGE_CASES:                      # (the early exit's batch edges: checked against float64 too, not only against itself)
        _check_forward(fr, ref, *base)


def test_forward_of_a_frame_without_lists_is_zero():
    fr = FW.build_frame(3, 50, 37, lens=(0,), bad_ids=False)
    assert fr["D"] == 0
    med, contrib = _forward(FW.DeviceFrame(fr))
    assert not med.view(np.uint32).any() and not contrib.any()


def _addends(fr, ref):
    """Per Gaussian: the float32 additions its column goes through -- its pixels, block by block, and one atomic per block."""
    n = np.zeros(fr["N"], np.int64)
    sel = ref["contrib"] > 0
    np.add.at(n, ref["ids"][sel], 1)
    return int(n.max()) + 1                             # (+ 1: the atomic onto the seeded value)


@pytest.mark.parametrize("name", list(M.CASES))
def test_backward_against_float64(name):
    fr, ref = M.frame(name)
    d = FW.DeviceFrame(fr)
    g = M.draw_g(fr["H"], fr["W"])
    signed, scale = M.gradient_f64(fr, ref, g)
    acc = _backward(d, g, ref["contrib"], d.accumulators(False))
    E = M.gradient_error(acc[:, 11], signed, scale)
    bound = _addends(fr, ref) * EPS32
    rec = M.golden().get("E_backward", {}).get(name)
    _row(test="backward", case=name, E_kernel=E, bound=bound, recorded=rec, touched=int((scale > 0).sum()))
    assert (scale > 0).sum() >= 3 and np.abs(acc[:, 11]).max() > 0
    assert not acc[:, [c for c in range(16) if c != 11]].any()
    assert E <= bound, (E, bound)
    assert rec is None or E <= max(10.0 * rec, EPS32), (E, rec)
    # a seeded array: the other fifteen columns keep their bits, column 11 moves by the same sums
    seeded = _backward(d, g, ref["contrib"], d.accumulators(True))
    others = [c for c in range(16) if c != 11]
    assert seeded[:, others].tobytes() == fr["acc_seed"][:, others].tobytes()
    assert M.gradient_error(seeded[:, 11].astype(np.float64) - fr["acc_seed"][:, 11].astype(np.float64), signed, scale + np.abs(fr["acc_seed"][:, 11])) <= bound
    # g = 0 leaves the array as it is, and so does a contributor image of zeros
    assert _backward(d, np.zeros_like(g), ref["contrib"], d.accumulators(True)).tobytes() == fr["acc_seed"].tobytes()
    assert _backward(d, g, np.zeros_like(ref["contrib"]), d.accumulators(True)).tobytes() == fr["acc_seed"].tobytes()
    # stale contributors: past the list, negative -- clipped to the tile's range, never out of bounds, finite
    wild = np.where(np.random.default_rng(1).random(g.shape) < 0.5, 1 << 30, -5).astype(np.int32)
    assert np.isfinite(_backward(d, g, wild, d.accumulators(False))).all()


@pytest.mark.parametrize("tag", list(FW.BACKWARD_SHAPES))
def test_backward_bits_repeat_where_no_row_takes_more_than_two_addends(tag):
    seeded = tag == "8x8"                               # one wave adds: a seeded accumulator takes one addend per destination
    fr = FW.build_frame(11, lens=(640,), once_per_tile=True, **FW.BACKWARD_SHAPES[tag])
    fr["co"][:, 3] *= 0.35
    d = FW.DeviceFrame(fr)
    med, contrib = _forward(d)
    assert (contrib > 0).sum() >= 20
    g = M.draw_g(fr["H"], fr["W"])
    first = _backward(d, g, contrib, d.accumulators(seeded))
    assert np.isfinite(first).all() and (first[:, 11] != (fr["acc_seed"][:, 11] if seeded else 0)).any()
    for _ in range(2):
        assert _backward(d, g, contrib, d.accumulators(seeded)).tobytes() == first.tobytes()
    assert _backward(FW.DeviceFrame(FW.other_bad_ids(fr, 5)), g, contrib, d.accumulators(seeded)).tobytes() == first.tobytes()


# ---- through backward_view on a rendered frame ----
_RENDERED = {}


def rendered():
    """The kernel forward of n2000_64x48, the frame dict the reference reads (what the kernel reads: the records' 1 / depth) and the
    float64 statement on it, once per session."""
    if not _RENDERED:
        from test_gpu_features import _case
        gsr = pkg()
        sc, cam, kw, extra = _case("n2000_64x48")
        H, W = kw["image_height"], kw["image_width"]
        image, inv_depth, buf = gsr.render_gaussians(**kw, **extra)
        N = sc["means"].shape[0]
        nb = {k: parity.to_np(buf[k]) for k in ("points_xy_image", "conic_opacity", "point_list", "ranges", "n_contrib")}
        fr = dict(W=W, H=H, N=N, D=int(nb["point_list"].shape[0]), xy=nb["points_xy_image"].reshape(-1, 2).astype(np.float32),
                  co=nb["conic_opacity"].reshape(-1, 4).astype(np.float32), invd=parity.to_np(sub("_frame").inv_depth_of(buf, N, image.device)).astype(np.float32),
                  point_list=nb["point_list"].reshape(-1), ranges=nb["ranges"].reshape(-1, 2), n_contrib=nb["n_contrib"].reshape(H, W))
        ref = M.median_f64(fr)
        g = M.draw_g(H, W) / (H * W)
        _RENDERED.update(sc=sc, cam=cam, kw=kw, H=H, W=W, N=N, buf=buf, fr=fr, ref=ref, g=g, dev=image.device,
                         gd=torch.as_tensor(g, device=image.device), contrib=torch.as_tensor(ref["contrib"].astype(np.int32), device=image.device))
    return _RENDERED


def _bw(f, dpix=None, median=True, **more):
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], dpix)
    if median:
        kw.update(dL_dmedian_depth=f["gd"], median_contributor=f["contrib"])
    return pkg().backward(**kw, **more)


def test_render_median_depth_on_a_rendered_frame():
    med_mod = sub("median_depth")
    f = rendered()
    H, W, ref, fr = f["H"], f["W"], f["ref"], f["fr"]
    med, contrib = med_mod.render_median_depth(f["buf"], H, W)
    assert med.dtype == torch.float32 and contrib.dtype == torch.int32 and tuple(med.shape) == tuple(contrib.shape) == (H, W)
    keep = ~ref["tie"]
    assert ref["tie"].mean() <= M.MAX_TIES and (ref["contrib"] > 0).mean() > 0.5
    assert np.array_equal(parity.to_np(contrib)[keep], ref["contrib"][keep]) and parity.to_np(med)[keep].tobytes() == ref["med"][keep].tobytes()
    out = (torch.full((H, W), float("nan"), device=f["dev"]), torch.full((H, W), -1, dtype=torch.int32, device=f["dev"]))
    got = med_mod.render_median_depth(f["buf"], H, W, out=out, use_block_masks=False)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(out[0], med) and torch.equal(out[1], contrib)
    # the median lies among the depths the expected inverse depth averages: where both exist they are close on a surface-like frame
    z = med_mod.view_depth(med, f["buf"]["final_Ts"].reshape(H, W))
    assert bool(torch.isfinite(z).all()) and bool((z >= 0).all()) and bool((z > 0).any())
    assert bool(((z > 0) == ((med > 0) & (1.0 - f["buf"]["final_Ts"].reshape(H, W) >= 0.5))).all())


def test_backward_view_carries_the_median_term():
    f = rendered()
    N, fr, ref = f["N"], f["fr"], f["ref"]
    signed, scale = M.gradient_f64(fr, ref, f["g"])
    alone = _bw(f)
    assert tuple(alone["dL_dinv_depths"].shape) == (N,) and bool(torch.isfinite(alone["_arena"]).all())
    E = M.gradient_error(parity.to_np(alone["dL_dinv_depths"]), signed, scale)
    bound = _addends(fr, ref) * EPS32
    _row(test="backward_view", E_kernel=E, bound=bound)
    assert E <= bound and (scale > 0).sum() > 100
    assert not bool(alone["dL_dcolor"].any()) and not bool(alone["dL_dconic"].any())        # the term alone: column 11 and nothing else
    assert bool(alone["dL_dmean3D"].any())                                                  # ... which the per-Gaussian half carries on to the means
    dpix = (np.random.default_rng(3).normal(0, 1, (f["H"], f["W"], 3)) / (f["H"] * f["W"] * 3)).astype(np.float32)
    plain, both = _bw(f, dpix, median=False, absgrad=True), _bw(f, dpix, absgrad=True)
    assert "dL_dinv_depths" in both and "dL_dinv_depths" not in plain
    for k in ("dL_dcolor", "dL_dconic", "dL_dopacity", "dL_dshs", "dL_dmean2D_abs"):                         # what the term does not touch
        parity.assert_grad(k, both[k], plain[k])
    assert M.gradient_error(parity.to_np(both["dL_dinv_depths"]), signed, scale) <= bound
    assert float((both["dL_dmean3D"] - plain["dL_dmean3D"]).abs().max()) > 0


def test_camera_grad_and_factored_calls_agree_with_the_dense_call():
    f = rendered()
    dpix = (np.random.default_rng(3).normal(0, 1, (f["H"], f["W"], 3)) / (f["H"] * f["W"] * 3)).astype(np.float32)
    keys = ("dL_dmean3D", "dL_dscale", "dL_drot", "dL_dopacity", "dL_dinv_depths")
    dense = _bw(f, dpix)
    cam = _bw(f, dpix, camera_grad=True)
    for k in keys + ("dL_dshs", "dL_dmean2D", "dL_dconic"):
        parity.assert_grad(k, cam[k], dense[k])
    plain_cam = _bw(f, dpix, median=False, camera_grad=True)
    for k in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"):
        assert bool(torch.isfinite(cam[k]).all()) and bool(cam[k].any())
    assert float((cam["dL_dviewmatrix"] - plain_cam["dL_dviewmatrix"]).abs().max()) > 0       # the camera kernels read column 11
    seen = []
    fact = _bw(f, dpix, sh_gradient="factored", on_payload=seen.append, camera_grad=True)
    assert fact["dL_dshs"] is None and len(seen) == 1 and seen[0] is fact["_view_payload"]
    for k in keys:
        parity.assert_grad(k, fact[k], dense[k])
    parity.assert_grad("dL_dviewmatrix", fact["dL_dviewmatrix"], cam["dL_dviewmatrix"])
    parity.assert_grad("payload", fact["_view_payload"], _bw(f, dpix, median=False, sh_gradient="factored")["_view_payload"])
    # without the forward's records the frame is re-packed from the forward's depths
    kw = backward_kwargs(f["sc"], f["cam"], f["kw"], f["buf"], dpix)
    kw.update({"means2D": f["buf"]["points_xy_image"].clone(), "conic_opacity": f["buf"]["conic_opacity"].clone(), "rgb": f["buf"]["colors"].clone()},
              dL_dmedian_depth=f["gd"], median_contributor=f["contrib"])
    with pytest.raises(ValueError, match="depths"):
        pkg().backward(**kw)
    kw["geom_buffer"] = dict(kw["geom_buffer"], depths=f["buf"]["depths"])
    repacked = pkg().backward(**kw)
    assert not pkg().backward.last_call_used_forward_records
    for k in keys:
        parity.assert_grad(k, repacked[k], dense[k])


# ---- the workflow ----
def test_torus_demo_gives_a_mesh_in_both_depth_modes():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from eval_mesh import demo_torus
    rows = {}
    for mode in ("expected", "median"):
        m = demo_torus(pkg(), 48, 8, 20_000, 128, seed=0, log=lambda s: None, depth_mode=mode)
        assert m["triangles"] > 0 and m["vertices"] > 0 and m["depth_mode"] == mode
        for k in ("accuracy", "completeness", "chamfer", "accuracy_voxels", "completeness_voxels"):
            assert np.isfinite(m[k]) and m[k] >= 0, (mode, k, m[k])
        rows[mode] = {k: m[k] for k in ("accuracy_voxels", "completeness_voxels", "triangles")}
    _row(test="torus", **rows)
    assert M.golden()["mesh_gap_min"] is None           # no threshold on the gap: README "Median depth" says why


def test_trainer_runs_with_the_median_depth_term(tmp_path):
    log = tmp_path / "median.jsonl"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), "--log", str(log), "--print-interval", "1000", "--size", "100",
                        "--views", "8", "--iterations", "300", "--lambda-depth", "1", "--depth-render", "median"],
                       cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    s = [json.loads(line) for line in open(log)]
    s = [r for r in s if r["record"] == "summary"][0]
    assert all(s["parameters_finite"].values()) and s["depth_render"] == "median"
    for k in ("train_psnr_mean", "train_depth_l1_mean", "train_median_depth_l1_mean"):
        assert np.isfinite(s[k]), k
    _row(test="trainer", psnr=s["train_psnr_mean"], depth_l1=s["train_depth_l1_mean"], median_depth_l1=s["train_median_depth_l1_mean"])
