"""gsr_knn on the MI355X against the float32 yardstick (tests/knn_reference.py), BIT FOR BIT: include/gsr_knn.h defines the result
exactly (float32 d2 in a stated order, candidates by (d2, index), k = min(3, N - 1)), so no tolerance is needed or allowed.  The
clouds are the ones on which a pruning structure can go wrong: fewer than three neighbours, wave and block edges, one Morton cell
for everything, two cells for everything, axes of zero extent, an outlier that stretches the grid, massive ties, several blocks.
Then the properties the definition implies (permutation, determinism, independence from the workspace's contents and the stream),
init_scales, gaussians_from_points through the renderer, and the trainer's two new starts."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, lego_camera, pkg, render_kwargs, sub
from knn_reference import knn_reference
from test_knn_reference import lattice

pytestmark = pytest.mark.gpu
B = sub("_lib").KNN_BLOCK_POINTS


def uniform(n, seed=0):
    return np.random.default_rng(seed).uniform(-1.3, 1.3, (n, 3)).astype(np.float32)


def mixture(n, seed=1):
    """Three Gaussian components of very different density: the blocks' boxes differ in size by orders of magnitude."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, 3, n)
    centre = np.array([[0.0, 0.0, 0.0], [2.0, -1.0, 0.5], [-3.0, 4.0, 1.0]])[which]
    sigma = np.array([0.02, 0.3, 1.5])[which][:, None]
    return (centre + rng.normal(0, 1, (n, 3)) * sigma).astype(np.float32)


def clusters():
    rng = np.random.default_rng(2)
    a = rng.uniform(0, 1e-3, (200, 3))
    b = rng.uniform(0, 1e-3, (200, 3)) + 1e3
    return np.concatenate([a, b]).astype(np.float32)[rng.permutation(400)]


def collinear(axis):
    p = np.tile(np.array([0.5, -2.0, 0.25], np.float32), (700, 1))
    p[:, axis] = np.random.default_rng(3 + axis).uniform(-5, 5, 700).astype(np.float32)
    return p


def outlier():
    return np.concatenate([np.random.default_rng(4).uniform(0, 1, (2000, 3)), [[1e4, 1e4, 1e4]]]).astype(np.float32)


# 8 B + 1 = 2 049 points span nine blocks: the index yardstick takes well under a second there
CLOUDS = {
    **{f"uniform_{n}": functools.partial(uniform, n) for n in (1, 2, 3, 4, 5, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1)},
    "identical_300": lambda: np.full((300, 3), 0.37, np.float32),
    "two_tight_clusters": clusters,
    "collinear_x": functools.partial(collinear, 0),
    "collinear_z": functools.partial(collinear, 2),
    "one_far_outlier": outlier,
    "lattice_8x8x8": lattice,
    f"mixture_{8 * B + 1}": functools.partial(mixture, 8 * B + 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(points, yardstick mean, yardstick indices): computed once, shared, never written."""
    p = CLOUDS[name]()
    mean, idx = knn_reference(p, want_indices=True)
    for a in (p, mean, idx):
        a.setflags(write=False)
    return p, mean, idx


def run(p, want_indices=True):
    knn = sub("knn")
    out = knn.knn(torch.tensor(p).cuda(), want_indices=want_indices)
    torch.cuda.synchronize()
    if want_indices:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy(), None


def differing(got, ref):
    bad = np.nonzero(got.reshape(len(got), -1).view(np.uint32) != ref.reshape(len(ref), -1).view(np.uint32))[0]
    return f"{len(bad)} of {len(got)} rows differ, first {bad[:5].tolist()}: got {got[bad[:3]].tolist()} want {ref[bad[:3]].tolist()}"


@pytest.mark.parametrize("name", list(CLOUDS))
def test_knn_matches_the_yardstick_bit_for_bit(name):
    p, mean, idx = case(name)
    got_mean, got_idx = run(p)
    assert got_mean.dtype == np.float32 and got_idx.dtype == np.int32 and got_idx.shape == (len(p), 3)
    assert got_mean.tobytes() == mean.tobytes(), differing(got_mean, mean)
    assert got_idx.tobytes() == idx.tobytes(), differing(got_idx, idx)
    only_mean, _ = run(p, want_indices=False)                   # nn_index = NULL: the same distances
    assert only_mean.tobytes() == mean.tobytes(), differing(only_mean, mean)


def test_closed_forms_on_the_device():
    p, _, _ = case("lattice_8x8x8")
    mean, idx = run(p)
    assert (mean == np.float32(0.0625)).all() and idx[0].tolist() == [1, 8, 64]
    mean, idx = run(case("identical_300")[0])
    assert (mean == 0).all() and idx[0].tolist() == [1, 2, 3] and (idx[4:] == np.array([0, 1, 2])).all()
    mean, idx = run(case("uniform_1")[0])
    assert mean.tolist() == [0.0] and idx.tolist() == [[-1, -1, -1]]
    mean, idx = run(np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], np.float32))
    assert mean.tolist() == [9.0, 9.0] and idx.tolist() == [[1, -1, -1], [0, -1, -1]]


def test_many_blocks_values_only():
    """16 385 points of the mixture, 65 blocks, through the NULL path; the value yardstick takes about three seconds."""
    p = mixture(16385, seed=6)
    mean, _ = knn_reference(p)
    got, _ = run(p, want_indices=False)
    assert got.tobytes() == mean.tobytes(), differing(got, mean)


def test_an_index_permutation_gives_the_same_distances():
    p, mean, _ = case(f"mixture_{8 * B + 1}")
    perm = np.random.default_rng(9).permutation(len(p))
    got, _ = run(p[perm], want_indices=False)
    assert got.tobytes() == mean[perm].tobytes()               # (d2 does not depend on the indices; only the tie-break does)
    assert np.sort(got).tobytes() == np.sort(mean).tobytes()


def test_same_bits_every_call_whatever_the_workspace_held_and_on_a_side_stream():
    _host, _lib, knn = sub("_host"), sub("_lib"), sub("knn")
    p, mean, idx = case(f"mixture_{8 * B + 1}")
    pts = torch.tensor(p).cuda()
    dev = pts.device
    first = knn.knn(pts, want_indices=True)
    again = knn.knn(pts, want_indices=True)
    ws = _host.workspace("knn", _lib.lib().gsr_knn_workspace_bytes(len(p)), dev)
    ws.fill_(0xFF)
    dirty = knn.knn(pts, want_indices=True)
    assert _host.workspace("knn", 1, dev) is ws                 # (the call above ran in the workspace that was filled)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = knn.knn(pts, want_indices=True)
    torch.cuda.synchronize()
    for name, (m, i) in (("first", first), ("again", again), ("0xFF workspace", dirty), ("side stream", aside)):
        assert m.cpu().numpy().tobytes() == mean.tobytes(), name
        assert i.cpu().numpy().tobytes() == idx.tobytes(), name
    out = (torch.empty(len(p), device=dev), torch.empty((len(p), 3), dtype=torch.int32, device=dev))
    assert knn.knn(pts, want_indices=True, out=out)[0] is out[0]
    torch.cuda.synchronize()
    assert out[0].cpu().numpy().tobytes() == mean.tobytes() and out[1].cpu().numpy().tobytes() == idx.tobytes()


def test_init_scales_floors_and_takes_the_root():
    knn = sub("knn")
    same = knn.init_scales(torch.from_numpy(case("identical_300")[0].copy()).cuda())
    assert same.shape == (300, 3) and same.dtype == torch.float32
    assert (same == torch.sqrt(torch.tensor(1e-7, dtype=torch.float32, device="cuda"))).all()
    quarter = knn.init_scales(torch.from_numpy(case("identical_300")[0].copy()).cuda(), floor=0.25)
    assert (quarter == torch.sqrt(torch.tensor(0.25, dtype=torch.float32, device="cuda"))).all() and abs(float(quarter[0, 0]) - 0.5) < 1e-6
    p, mean, _ = case("one_far_outlier")
    s = knn.init_scales(torch.from_numpy(p.copy()).cuda())
    assert s.shape == (len(p), 3) and s.is_contiguous()
    want = torch.sqrt(torch.from_numpy(mean.copy()).cuda())     # (every mean is far above the floor here)
    assert mean.min() > 1e-7 and all(torch.equal(s[:, c], want) for c in range(3))


def test_gaussians_from_points_render(cameras):
    gsr, pc = pkg(), sub("point_cloud")
    rng = np.random.default_rng(11)
    xyz = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    rgb = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    P = pc.gaussians_from_points(xyz, rgb, device="cuda")
    n = len(xyz)
    assert {k: tuple(v.shape) for k, v in P.items()} == {"positions": (n, 3), "scales": (n, 3), "rotations": (n, 4), "opacities": (n,),
                                                         "shs": (n * 16, 3)}
    assert all(v.dtype == torch.float32 and v.is_cuda for v in P.values())
    mean, _ = knn_reference(xyz)
    assert mean.min() > 1e-7 and np.allclose(P["scales"][:, 0].cpu().numpy(), np.sqrt(mean), rtol=1e-6, atol=0)   # (the root is torch's, on the device)
    assert torch.equal(P["scales"][:, 0], P["scales"][:, 1]) and torch.equal(P["scales"][:, 0], P["scales"][:, 2])
    assert (P["rotations"].cpu() == torch.tensor([1.0, 0.0, 0.0, 0.0])).all() and (P["opacities"] == 0.1).all()
    shs = P["shs"].view(n, 16, 3).cpu().numpy()
    assert (shs[:, 1:] == 0).all() and (shs[:, 0] == (rgb - np.float32(0.5)) / np.float32(0.28209479177387814)).all()
    Q = pc.gaussians_from_points(xyz, device="cuda")
    assert (Q["shs"] == 0).all() and torch.equal(Q["scales"], P["scales"])
    cam = lego_camera(cameras, 0, 64, 64)
    scene = {"means": P["positions"], "opacities": P["opacities"], "scales": P["scales"], "rotations": P["rotations"], "shs": P["shs"].view(n, 16, 3)}
    img, _, buf = gsr.render_gaussians(**render_kwargs(scene, cam, width=64, height=64))
    torch.cuda.synchronize()
    img = img if isinstance(img, torch.Tensor) else torch.as_tensor(img)
    assert img.numel() == 64 * 64 * 3 and bool(torch.isfinite(img).all()) and float(img.abs().sum()) > 0.0


def _train(tmp, *extra):
    log = os.path.join(tmp, "run.jsonl")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "train.py"), "--size", "100", "--views", "8", "--iterations", "30", "--gaussians", "3000",
           "--print-interval", "1000", "--log", log, *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    records = [json.loads(ln) for ln in open(log)]
    header, summary = records[0], [r for r in records if r["record"] == "summary"][0]
    assert header["record"] == "arguments"
    assert all(summary["parameters_finite"].values()) and np.isfinite(summary["train_psnr_mean"])
    return header, summary, p.stdout


def test_trainer_starts_from_knn_scales_and_from_a_point_file(tmp_path):
    header, summary, _ = _train(str(tmp_path), "--init", "knn")
    assert header["init"] == "knn" and summary["points_start"] == 3000
    lo, mid, hi = (header[k] for k in ("init_scale_min", "init_scale_median", "init_scale_max"))
    assert 0.0 < lo <= mid <= hi < 2.6 and np.isfinite([lo, mid, hi]).all()
    # the same numbers from the yardstick: the reference start's positions are the library's, read back
    P = sub("densify").init_gaussian_params(3000, 0.1, "cuda")
    mean, _ = knn_reference(P["positions"].cpu().numpy())
    root = np.sqrt(np.maximum(mean, np.float32(1e-7)))
    assert np.allclose([lo, hi], [root.min(), root.max()], rtol=1e-6)
    # from a file the test writes: 1 500 coloured points; --gaussians is overridden
    from test_knn_abi import RGB, XYZ, _write_ply
    rng = np.random.default_rng(12)
    xyz = rng.uniform(-0.8, 0.8, (1500, 3)).astype(np.float32)
    ply = str(tmp_path / "cloud.ply")
    _write_ply(ply, XYZ + RGB, list(xyz.T) + list(rng.integers(0, 256, (3, 1500)).astype(np.uint8)))
    header, summary, out = _train(str(tmp_path), "--init-points", ply)
    assert header["init"] == "points" and header["gaussians"] == 1500 and summary["points_start"] == 1500
    assert "is overridden" in out
    mean, _ = knn_reference(xyz)
    root = np.sqrt(np.maximum(mean, np.float32(1e-7)))
    assert np.allclose([header["init_scale_min"], header["init_scale_max"]], [root.min(), root.max()], rtol=1e-6)
