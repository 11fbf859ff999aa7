"""GPU tests of the library's host-side state (include/gsr.h, 'Conventions'): the count check behind GSR_E_CAPACITY, concurrent
host threads over distinct buffers and streams (readback slots are leased per call, not per thread), and the timing-ablation
switches of GSR_DEBUG being inert in the product build.  And of the binding's: the image losses' scratch comes from the one grow-only
cache, _host.workspace -- a call handed a larger buffer than it asked for, or a buffer full of another call's leavings, gives the bits
of a call with a fresh one; the cache holds one buffer per (kind, stream), whatever the image sizes were; a side stream has its own."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import parity
from conftest import ROOT, lego_camera, pkg, render_kwargs, sub

pytestmark = pytest.mark.gpu


def test_forward_render_refuses_a_wrong_count(cameras, scenes):
    """gsr_forward_render used to trust GsrBinning.D -- too large wrote out of bounds on the device, too small
    truncated the list.  Now it must equal the count gsr_forward_count returned for the same geom workspace."""
    import torch
    _lib, _host = sub("_lib"), sub("_host")
    L = _lib.lib()
    W, H, n = 128, 96, 1500
    sc = scenes.synthetic_scene(n, 0.05, 0.5, seed=3)
    cam = lego_camera(cameras, frame=1, width=W, height=H)
    kw = render_kwargs(sc, cam, width=W, height=H)
    dev = torch.device("cuda", 0)
    t = lambda a, shape: torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).to(dev)
    means, scales, rots, op, shs = t(sc["means"], (n, 3)), t(sc["scales"], (n, 3)), t(sc["rotations"], (n, 4)), t(sc["opacities"], (n,)), t(sc["shs"], (n * 16, 3))
    scene = _lib.GsrScene(n, _host.ptr(means), _host.ptr(scales), _host.ptr(rots), _host.ptr(op), _host.ptr(shs), 3, 1.0, 1)
    cs = _host.make_camera(kw["viewmatrix"], kw["projmatrix"], kw["campos"], kw["background"], kw["tan_fovx"], kw["tan_fovy"], W, H)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    i32, f32 = torch.int32, torch.float32
    bufs = [e((n,), i32), e((n,), i32), e((n,), i32), e((n, 2), f32), e((n,), f32), e((n, 6), f32), e((n, 3), f32), e((n, 4), f32), e((n, 3), f32)]
    geom = _lib.GsrGeom(*[_host.ptr(b) for b in bufs], None)
    gws = torch.empty(L.gsr_geom_workspace_bytes(n), dtype=torch.uint8, device=dev)
    gws2 = torch.empty_like(gws)                                            # never counted
    D = C.c_int64(0)
    stream = _host.stream_ptr(dev)
    assert L.gsr_forward_count(C.byref(scene), C.byref(cs), C.byref(geom), _host.ptr(gws), gws.numel(), C.byref(D), stream) == 0
    D = D.value
    assert D > 0
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    img = [e((H, W, 3), f32), e((H, W), f32), e((H, W), f32), e((H, W), i32)]
    image = _lib.GsrImage(*[_host.ptr(b) for b in img])
    ranges = e((tiles, 2), i32)
    point_list = e((D + 64,), i32)
    bws = torch.empty(L.gsr_binning_workspace_bytes(n, D + 64, W, H), dtype=torch.uint8, device=dev)

    def render(d, ws):
        b = _lib.GsrBinning(d, _host.ptr(point_list), _host.ptr(ranges), None)
        return L.gsr_forward_render(C.byref(scene), C.byref(cs), C.byref(geom), C.byref(b), C.byref(image), _host.ptr(ws), ws.numel(),
                                    _host.ptr(bws), bws.numel(), stream)

    assert render(D + 1, gws) == _lib.GSR_E_CAPACITY
    assert render(D - 1, gws) == _lib.GSR_E_CAPACITY
    assert render(D, gws2) == _lib.GSR_E_CAPACITY
    assert render(D, gws) == 0                                              # the right count still renders, and twice
    first = img[0].clone()
    assert render(D, gws) == 0
    torch.cuda.synchronize()
    assert torch.equal(first, img[0]) and bool(torch.isfinite(first).all())
    with pytest.raises(RuntimeError, match="count"):
        _lib.check(_lib.GSR_E_CAPACITY)


def test_two_host_threads_over_distinct_buffers(oracle, cameras, scenes):
    """Two host threads, each with its own HIP stream, scene and (per-stream) workspaces, call render_gaussians + backward
    concurrently (ctypes drops the GIL inside the library): results equal what the same calls give one after the other."""
    import torch
    gsr = pkg()
    cases = []
    for k, (n, seed, frame) in enumerate([(20000, 71, 0), (26000, 72, 4)]):
        sc = scenes.synthetic_scene(n, 0.03, 0.6, seed=seed)
        cam = lego_camera(cameras, frame=frame, width=256, height=192)
        kw = render_kwargs(sc, cam, width=256, height=192)
        for key in ("means3D", "opacity", "scales", "rotations", "sh"):
            kw[key] = torch.as_tensor(np.ascontiguousarray(kw[key], np.float32)).cuda()
        cases.append(kw)

    def run(kw, reps, out):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for _ in range(reps):
                img, depth, buf = gsr.render_gaussians(**kw)
            st.synchronize()
        out.append((img.cpu().numpy(), buf["point_list"].cpu().numpy(), buf["ranges"].cpu().numpy(), buf["n_contrib"].cpu().numpy()))

    seq = [[], []]
    for k in range(2):
        run(cases[k], 1, seq[k])
    par = [[], []]
    errs = []

    def guarded(k):
        try:
            run(cases[k], 25, par[k])
        except Exception as ex:      # noqa: BLE001 -- surfaced below
            errs.append(ex)

    threads = [threading.Thread(target=guarded, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errs, errs
    for k in range(2):
        for a, b in zip(seq[k][0], par[k][0]):
            np.testing.assert_array_equal(a, b)
    ref = oracle.render_gaussians(**{**cases[0], **{key: cases[0][key].cpu().numpy() for key in ("means3D", "opacity", "scales", "rotations", "sh")}})
    parity.assert_exact("point_list", par[0][0][1], ref[2]["point_list"])


def test_debug_ablation_bits_are_inert_in_the_product_build():
    """GSR_DEBUG=15 (every timing ablation: no atomics, one pixel per bucket, no SH fetch, no stores) must change nothing in
    libgsr_hip.so: smoke() still matches the oracle.  The library reads the variable once, hence a subprocess."""
    env = dict(os.environ, GSR_DEBUG="15")
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "smoke ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- one workspace cache (_host.workspace) behind the image losses ----
SIZES = ((5, 9), (33, 15), (97, 61))        # (W, H): under one SSIM window and one normals tile; across a tile edge; a larger buffer
KINDS = ("sum", "dssim", "weighted_dssim", "depth_corr", "normals")


def _dev():
    return torch.device("cuda", 0)


def _inputs(W, H):
    rng = np.random.default_rng(1000 * W + H)
    y, x = np.mgrid[0:H, 0:W]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(_dev())      # noqa: E731
    n = rng.normal(size=(H, W, 3)) + np.array([0.0, 0.0, -2.0])
    return {"rendered": up(rng.uniform(0, 1, (H, W, 3))), "target": up(rng.uniform(0, 1, (H, W, 3))),
            "weights": up(rng.uniform(0, 1, (H, W)) * (rng.uniform(size=(H, W)) > 0.2)),          # a fifth of the pixels do not count
            "depth": up(0.5 + 0.02 * x + 0.03 * y + 0.01 * rng.normal(size=(H, W))), "prior": up(rng.uniform(0.1, 2.0, (H, W))),
            "final_Ts": up(rng.uniform(0.0, 0.3, (H, W))), "normal": up(n / np.linalg.norm(n, axis=2, keepdims=True)),
            "camera": {"tan_fovx": 0.5, "tan_fovy": 0.5 * H / W, "width": W, "height": H}}


@pytest.fixture(scope="module")
def inputs():
    return {size: _inputs(*size) for size in SIZES}


def _call(kind, a):
    """The public call behind a workspace kind; every output tensor of it."""
    loss = sub("loss")
    if kind == "sum":
        out = loss.l1_loss_and_gradients(a["rendered"], a["target"], 0.2, weights=a["weights"])
    elif kind == "dssim":
        out = loss.l1_dssim_loss_and_gradients(a["rendered"], a["target"])
    elif kind == "weighted_dssim":
        out = loss.l1_dssim_loss_and_gradients(a["rendered"], a["target"], weights=a["weights"])
    elif kind == "depth_corr":
        out = loss.depth_corr_loss_and_gradients(a["depth"], a["prior"], a["weights"])
    else:
        out = loss.normal_loss_and_gradients(a["depth"], a["final_Ts"], a["normal"], a["camera"], mask=a["weights"])
    assert all(t is not None for t in out)
    return out


def _needed(kind, W, H):
    L = sub("_lib").lib()
    entry = {"sum": L.gsr_weight_total_workspace_bytes, "dssim": L.gsr_dssim_workspace_bytes, "weighted_dssim": L.gsr_weighted_dssim_workspace_bytes,
             "depth_corr": L.gsr_depth_corr_workspace_bytes, "normals": L.gsr_normals_workspace_bytes}[kind]
    return int(entry(W, H))


def _same_bits(got, want):
    return all(torch.equal(g.contiguous().view(torch.int32), w.contiguous().view(torch.int32)) for g, w in zip(got, want))


def _ours(cache):
    return {k for k in cache if k[0] in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_one_workspace_per_kind_and_stream_whatever_the_sizes(kind, inputs):
    host = sub("_host")
    dev = _dev()
    before = _ours(host._ws)
    main = host.raw_stream(dev)
    # a bare weight image has its total formed in the call, in the "sum" workspace
    touched = {kind, "sum"} if kind == "weighted_dssim" else {kind}
    first = {size: _call(kind, inputs[size]) for size in SIZES}                          # ascending: the buffer is made, and grows
    ws = host._ws[(kind, dev.index, main)]
    assert ws.numel() >= max(_needed(kind, W, H) for W, H in SIZES)
    for size in SIZES:
        for t in first[size]:
            assert bool(torch.isfinite(t).all()), size
    for k in touched:
        host._ws[(k, dev.index, main)].fill_(0xFF)
    for size in reversed(SIZES):                                                         # descending: a larger buffer than the call asks for, full of NaN
        assert ws.numel() > _needed(kind, *size), size
        assert _same_bits(_call(kind, inputs[size]), first[size]), size
        assert host._ws[(kind, dev.index, main)] is ws, size
    assert _ours(host._ws) - before <= {(k, dev.index, main) for k in touched}           # one per (kind, stream): none per size
    # a side stream: a buffer of its own, the same bits
    mid = _ours(host._ws)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        key = (kind, dev.index, host.raw_stream(dev))
        assert key[2] != main
        again = {size: _call(kind, inputs[size]) for size in SIZES}
        assert _ours(host._ws) - mid <= {(k,) + key[1:] for k in touched}
        side_ws = host._ws[key]
    side.synchronize()
    assert side_ws is not ws and side_ws.data_ptr() != ws.data_ptr() and host._ws[(kind, dev.index, main)] is ws
    for size in SIZES:
        assert _same_bits(again[size], first[size]), size
