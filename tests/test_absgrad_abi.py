"""CPU-side checks of the screen-space densification statistics and the absolute-gradient backward (include/gsr_densify_stats.h):
the float64 yardstick of the GPU tests (tests/absgrad_reference.py) is itself right -- its signed sum is f64_reference's blend-stage
dL_dmean2D and its per-pixel terms are torch autograd of the float64 blend, one pixel at a time --, the header is plain C99, the
library exports its entry points, every argument is checked before anything is enqueued, the trainer parses and refuses the new
flags, and dist.reduce_densify_stats sums / maximises over two gloo ranks."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from abi_helpers import compile_c99_probe, declared_names, fake_call_setup, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, PKG_NAME, sub
import absgrad_reference as AR
import f64_reference as F
import test_f64_reference as R

HDR = os.path.join(ROOT, "include", "gsr_densify_stats.h")
NAMES = {"gsr_backward_flags", "gsr_backward_blend_flags", "gsr_densify_stats_update", "gsr_densify_mark_stats", "gsr_prune_mark_stats"}


# ---- the yardstick ----
SMALL = dict(W=40, H=32, n=14, degree=3, train=True, bg=(0.2, 0.5, 0.3), sm=1.0, seed=41, outside=0.0, behind=0.0, scale=0.12, aniso=4.0,
             opaque=0.15)


def _small_case(oracle, cameras):
    sc, cam, kw = R.make_case(cameras, **SMALL)
    _, _, buf = oracle.render_gaussians(**kw)
    pre = F.preprocess_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    assert int((np.asarray(buf["radii"]) > 0).sum()) >= 8
    rng = np.random.default_rng(3)
    H, W = kw["image_height"], kw["image_width"]
    dpix = rng.normal(0, 1, (H, W, 3)).astype(np.float32)
    gD = rng.normal(0, 1, (H, W)).astype(np.float32)
    gA = rng.normal(0, 1, (H, W)).astype(np.float32)
    return sc, kw, buf, pre, dpix, gD, gA


def test_yardstick_signed_sum_is_the_f64_blend_gradient(oracle, cameras):
    sc, kw, buf, pre, dpix, _, _ = _small_case(oracle, cameras)
    ref = F.backward_f64(sc, kw, buf["point_list"], buf["ranges"], dpix, pre=pre)["dL_dmean2D"]
    got = AR.of_case(pre, buf["point_list"], buf["ranges"], dL_dpixels=dpix)
    scale = np.abs(ref).max()
    assert scale > 0 and int((np.abs(ref[:, :2]).max(1) > 0).sum()) >= 8
    assert np.abs(got["signed"] - ref[:, :2]).max() <= 1e-6 * scale
    assert np.all(ref[:, 2] == 0)
    # the magnitudes dominate the signed sums, and differ from them (opposite-signed pixels exist)
    assert np.all(got["abs"] >= np.abs(got["signed"]) - 1e-12 * scale)
    assert np.any(got["abs"] > 1.5 * np.abs(got["signed"]))


def test_yardstick_per_pixel_terms_are_autograd_of_the_f64_blend(oracle, cameras):
    """The jacobian over pixels: for every pixel, autograd of (colour . dpix + Dinv gD + (1 - T_final) gA) at that pixel alone with
    respect to the screen positions, against the closed-form terms."""
    sc, kw, buf, pre, dpix, gD, gA = _small_case(oracle, cameras)
    cam = pre["cam"]
    W, H = cam.W, cam.H
    got = AR.of_case(pre, buf["point_list"], buf["ranges"], dpix, gD, gA, per_pixel=True)
    xy = pre["xy"].detach().clone().requires_grad_(True)
    img, dep, fT, _ = F.blend_f64(xy, pre["conic"].detach(), pre["opacity"].detach(), pre["colour"].detach(), pre["depth"].detach(),
                                  buf["point_list"], buf["ranges"], cam.bg, W, H)
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    per_pixel = (img * t64(dpix)).sum(2) + dep * t64(gD) + (1.0 - fT) * t64(gA)
    half = np.array([0.5 * W, 0.5 * H])
    scale = np.abs(got["terms"]).max()
    assert scale > 0
    worst = 0.0
    for p in range(H * W):
        g = torch.autograd.grad(per_pixel[p // W, p % W], xy, retain_graph=True)[0].numpy() * half[None, :]
        worst = max(worst, float(np.abs(g - got["terms"][p]).max()))
    assert worst <= 1e-6 * scale, (worst, scale)
    assert np.abs(got["terms"].sum(0) - got["signed"]).max() <= 1e-9 * np.abs(got["signed"]).max()
    assert np.abs(np.abs(got["terms"]).sum(0) - got["abs"]).max() <= 1e-9 * got["abs"].max()


# ---- header, exports ----
def test_densify_stats_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_densify_stats.h"\n'
                                'int main(void) {\n'
                                '  GsrDensifyStats st = {0, 0, 0, 0};\n'
                                '  uint32_t f = GSR_BWD_ABSGRAD;\n'
                                '  int (*a)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrBinning *, const GsrImage *,\n'
                                '           const GsrPixelGrads *, const GsrGrads *, float *, void *, size_t, uint32_t, void *) = gsr_backward_flags;\n'
                                '  int (*b)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrBinning *, const GsrImage *,\n'
                                '           const GsrPixelGrads *, float *, void *, size_t, uint32_t, void *) = gsr_backward_blend_flags;\n'
                                '  int (*u)(const GsrDensifyStats *, const int32_t *, const void *, size_t, int32_t, void *) = gsr_densify_stats_update;\n'
                                '  int (*m)(const GsrParams *, const GsrDensifyStats *, float, float, float, int, int32_t *, void *) = gsr_densify_mark_stats;\n'
                                '  int (*p)(const GsrParams *, const GsrDensifyStats *, float, float, float, int32_t *, void *) = gsr_prune_mark_stats;\n'
                                '  (void)st; (void)f; (void)a; (void)b; (void)u; (void)m; (void)p; return 0; }\n')


def test_densify_stats_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.DENSIFY_STATS_EXPORTS) == declared
    for other in (_lib.EXPORTS, _lib.CAPACITY_EXPORTS, _lib.LOSS_EXPORTS, _lib.AUX_EXPORTS, _lib.CAMERA_EXPORTS):
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_densify_stats.h" in doc and "GSR_BWD_ABSGRAD" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "GsrDensifyStats" not in gsr_h and "GSR_BWD_ABSGRAD" not in gsr_h
    assert _lib.lib().gsr_abi_version() == 7


# ---- argument checks ----
def test_flagged_backward_arguments_are_checked_before_any_hip_call(libpath):
    """Fake 16-byte-aligned pointers: every case below returns before anything is dereferenced or enqueued."""
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    ws_bytes = int(L.gsr_backward_workspace_bytes(N, 100, W, H))
    img = _lib.GsrImage(None, None, A, A)
    geom = _lib.GsrGeom(A, None, None, A, None, A, A, A, A, A, None)
    PG = _lib.GsrPixelGrads

    def call(pg, flags=_lib.BWD_ABSGRAD, half=None, D=100, ws=A, wsb=ws_bytes, gr=None, inv=None, g=geom, **bover):
        b = _lib.GsrBinning(D, A, A, None, None, None, 0)
        for k, v in bover.items():
            setattr(b, k, v)
        pgr = C.byref(pg) if pg is not None else None
        if half == "blend":
            return L.gsr_backward_blend_flags(C.byref(scene), C.byref(cam), C.byref(g), C.byref(b), C.byref(img), pgr, None, ws, wsb, flags, None)
        gr = gr or _lib.GsrGrads(A, A, A, A, A, None, None, None, None)
        return L.gsr_backward_flags(C.byref(scene), C.byref(cam), C.byref(g), C.byref(b), C.byref(img), pgr, C.byref(gr), inv, ws, wsb, flags, None)

    for half in (None, "blend"):
        for flags in (0, _lib.BWD_ABSGRAD):
            assert call(None, flags, half) == _lib.GSR_E_NULL
            assert call(PG(None, None, None), flags, half) == _lib.GSR_E_NULL
            assert call(PG(A + 4, None, None), flags, half) == _lib.GSR_E_ALIGN
            assert call(PG(A, None, A + 8), flags, half) == _lib.GSR_E_ALIGN
            assert call(PG(A, None, None), flags, half, D=-1) == _lib.GSR_E_OVERFLOW
            assert call(PG(A, None, None), flags, half, wsb=ws_bytes - 1) == _lib.GSR_E_WORKSPACE
            assert call(PG(A, None, None), flags, half, ws=None) == _lib.GSR_E_WORKSPACE
            assert call(PG(A, None, None), flags, half, point_list=A + 4) == _lib.GSR_E_ALIGN
            # an inverse-depth gradient needs records that carry 1/depth
            assert call(PG(A, A, None), flags, half, g=_lib.GsrGeom(A, None, None, A, None, A, A, A, A, None, None)) == _lib.GSR_E_NULL
        for flags in (2, 3, 0x80000000):                                  # unknown bits, before anything else
            assert call(PG(A, None, None), flags, half) == _lib.GSR_E_DIMS
            assert call(None, flags, half) == _lib.GSR_E_DIMS
    assert call(PG(A, None, None), gr=_lib.GsrGrads(None, A, A, A, A, None, None, None, None)) == _lib.GSR_E_NULL
    assert call(PG(A, None, None), gr=_lib.GsrGrads(A, A, A + 4, A, A, None, None, None, None)) == _lib.GSR_E_ALIGN
    assert call(PG(A, None, None), inv=A + 4) == _lib.GSR_E_ALIGN


def test_statistics_arguments_are_checked_before_any_hip_call(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    A = 0x10000
    N = 8
    wsb = int(L.gsr_backward_workspace_bytes(N, 0, 1, 1))
    ST = _lib.GsrDensifyStats
    ok = ST(N, A, A, A)
    upd = lambda st, radii=A, ws=A, b=wsb, use_abs=0: L.gsr_densify_stats_update(C.byref(st) if st is not None else None, radii, ws, b, use_abs, None)
    assert upd(None) == _lib.GSR_E_NULL
    assert upd(ST(N, None, A, A)) == _lib.GSR_E_NULL
    assert upd(ST(N, A, None, A)) == _lib.GSR_E_NULL
    assert upd(ST(N, A, A, None)) == _lib.GSR_E_NULL
    assert upd(ok, radii=None) == _lib.GSR_E_NULL
    assert upd(ST(-1, A, A, A)) == _lib.GSR_E_DIMS
    assert upd(ST((1 << 27) + 1, A, A, A)) == _lib.GSR_E_DIMS
    assert upd(ST(N, A + 4, A, A)) == _lib.GSR_E_ALIGN
    assert upd(ST(N, A, A + 8, A)) == _lib.GSR_E_ALIGN
    assert upd(ST(N, A, A, A + 4)) == _lib.GSR_E_ALIGN
    assert upd(ok, radii=A + 4) == _lib.GSR_E_ALIGN
    assert upd(ok, ws=A + 4) == _lib.GSR_E_ALIGN
    assert upd(ok, ws=None) == _lib.GSR_E_WORKSPACE
    assert upd(ok, b=wsb - 1, use_abs=1) == _lib.GSR_E_WORKSPACE
    assert upd(ST(0, None, None, None), radii=None, ws=None, b=0) == _lib.GSR_OK       # N = 0: nothing to do

    P = _lib.GsrParams
    params = P(N, A, A, A, A, A)
    mask = lambda p, st, mode=_lib.MARK_CLONE, out=A: L.gsr_densify_mark_stats(C.byref(p) if p is not None else None,
                                                                              C.byref(st) if st is not None else None, 1e-4, 1.0, 0.01, mode, out, None)
    prune = lambda p, st, out=A: L.gsr_prune_mark_stats(C.byref(p) if p is not None else None, C.byref(st) if st is not None else None,
                                                        0.005, 20.0, 0.1, out, None)
    for fn in (mask, prune):
        assert fn(None, ok) == _lib.GSR_E_NULL
        assert fn(params, None) == _lib.GSR_E_NULL
        assert fn(params, ST(N, None, A, A)) == _lib.GSR_E_NULL
        assert fn(params, ST(N + 1, A, A, A)) == _lib.GSR_E_DIMS                       # more statistics rows than Gaussians
        assert fn(P(-1, A, A, A, A, A), ST(0, None, None, None)) == _lib.GSR_E_DIMS
        assert fn(params, ST(N, A, A + 4, A)) == _lib.GSR_E_ALIGN
        assert fn(params, ok, out=None) == _lib.GSR_E_NULL
        assert fn(P(N, A, None, A, A, A), ok) == _lib.GSR_E_NULL                       # scales
        assert fn(P(0, None, None, None, None, None), ST(0, None, None, None), out=None) == _lib.GSR_OK
    assert mask(params, ok, mode=2) == _lib.GSR_E_DIMS
    assert prune(P(N, A, A, A, None, A), ok) == _lib.GSR_E_NULL                        # opacities


def test_update_refuses_a_result_without_absolute_columns():
    """Python knows what C cannot: use_abs on a backward that ran without absgrad, a foreign dict, a workspace written since."""
    densify = sub("densify")
    st = densify.DensifyStats(4, "cpu")
    assert st.grad_accum.dtype == torch.float32 and st.vis_count.dtype == torch.int32 and st.max_radii.dtype == torch.int32
    with pytest.raises(ValueError, match="dict backward"):
        st.update(torch.zeros(4, dtype=torch.int32), {"dL_dmean2D": torch.zeros(4, 3)})
    ws = torch.zeros(1024, dtype=torch.uint8)
    g = torch.zeros(4, 3)
    g._gsr_backward_ws = (ws, ws._version, False, 4)
    with pytest.raises(ValueError, match="absgrad=True"):
        st.update(torch.zeros(4, dtype=torch.int32), {"dL_dmean2D": g}, use_abs=True)
    ws.add_(1)
    with pytest.raises(ValueError, match="written after"):
        st.update(torch.zeros(4, dtype=torch.int32), {"dL_dmean2D": g})
    g._gsr_backward_ws = (ws, ws._version, True, 5)
    with pytest.raises(ValueError, match="holds 4"):
        st.update(torch.zeros(4, dtype=torch.int32), {"dL_dmean2D": g}, use_abs=True)
    st.grad_accum += 1
    st.reset()
    assert not st.grad_accum.any() and not st.vis_count.any() and not st.max_radii.any()


# ---- trainer flags ----
def _train(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_and_refuses_the_densification_flags():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--densify-stat", "--absgrad", "--densify-grad-threshold", "--prune-screen-size", "--prune-world-size"):
        assert flag in p.stdout, flag
    for extra in (["--absgrad"], ["--prune-screen-size", "20"], ["--prune-world-size", "0.1"],
                  ["--densify-stat", "reference", "--absgrad"]):
        p = _train(*extra)
        assert p.returncode != 0 and "need --densify-stat screen" in p.stderr, (extra, p.stderr[-2000:])
    for extra in (["--densify-stat", "screen", "--prune-screen-size", "-1"], ["--densify-stat", "screen", "--prune-world-size", "-0.1"],
                  ["--densify-grad-threshold", "-0.0001"], ["--densify-grad-threshold", "nan"]):
        p = _train(*extra)
        assert p.returncode != 0 and "must be >= 0" in p.stderr, (extra, p.stderr[-2000:])
    p = _train("--densify-stat", "blurry")
    assert p.returncode != 0 and "invalid choice" in p.stderr


# ---- dist.reduce_densify_stats over two gloo ranks ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import importlib
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    d = importlib.import_module(f"{PKG_NAME}.dist")
    densify = importlib.import_module(f"{PKG_NAME}.densify")
    d.init_from_env(backend="gloo")
    st = densify.DensifyStats(5, "cpu")
    st.grad_accum += torch.tensor([1.0, 0.0, 2.5, 0.25, 0.0]) * (rank + 1)
    st.vis_count += torch.tensor([1, 0, 3, 2, 0], dtype=torch.int32) * (rank + 1)
    st.max_radii += torch.tensor([7, 0, 3, 9, 0], dtype=torch.int32) if rank == 0 else torch.tensor([2, 0, 11, 9, 1], dtype=torch.int32)
    out = d.reduce_densify_stats(st, world)
    assert out is st
    q.put((rank, st.grad_accum.tolist(), st.vis_count.tolist(), st.max_radii.tolist()))
    torch.distributed.destroy_process_group()


def test_reduce_densify_stats_two_gloo_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, g, v, m in res:                                               # SUM, SUM, MAX -- identical on both ranks
        assert g == [3.0, 0.0, 7.5, 0.75, 0.0]
        assert v == [3, 0, 9, 6, 0]
        assert m == [7, 0, 11, 9, 1]
    # a single process: nothing to reduce, the object comes back as it is
    st = sub("densify").DensifyStats(3, "cpu")
    assert sub("dist").reduce_densify_stats(st) is st
