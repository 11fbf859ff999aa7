"""The two dispatch schedules, read back and held to their contracts (tests/schedule_reference.py): the forward blend's tile order
(csrc/fwd_order.h) and the backward blend's block order (blend_fwd.hip file_blocks, walked by blend_backward_splat_kernel<8,4,true>).

Grids: the smallest at which each mechanism can break, a few thousand small Gaussians each.
    tiles  W x H          forward order  block filing   what it covers
        1  16 x 16        on             on             the smallest grid
        7  112 x 16       on             on             fewer tiles than bands
        9  48 x 48        on             on             two tiles per band, bands 5-7 empty
      255  4080 x 16      on             on             one below a thread row of fwd_order_block
      256  256 x 256      on             on             a full thread row
      257  4112 x 16      on             on             the first tile of the second register slot
     3841  368 x 2672     on             on             the first tile of register slot 15
     4095  1040 x 1008    on             on             one below the limit
     4096  1024 x 1024    on             on             the limit
     4096  1023 x 1021    on             on             the limit, partial last column and row
     4096  1024 x 1024 L  on             off (8x8)      large splats: D >= 20 N, the backward takes 8x8 blocks, `filed` = 0
     4097  272 x 3856     off            off            past both limits: row-major forward, band-order backward
The forward tests drive gsr_forward_count / gsr_forward_render through ctypes with buffers they own and poison before every frame
(render_gaussians allocates with torch.empty: a tile that never ran could keep a previous, correct frame).  The tile-order tables
are found through gsr_fwd_order_tables_offset (include/gsr_debug_layout.h), never by restating the workspace layout.

Tolerances are parity.py's contract; integer outputs (point_list, ranges, n_contrib) must equal the oracle's exactly.  (Exact
n_contrib needs a scene without a pixel whose alpha sits within one rounding of 1/255: there v_exp_f32 and libm's expf decide the
alpha < 1/255 test differently, the one difference parity.py's contract tolerates.  The 4097-tile scene first drawn, N = 5000, has
such a pixel -- [3784, 226]: n_contrib 5 against 0, final_T 1 - 1/255 against 1 -- so that grid uses N = 4800.)  The ordered
and the unordered backward must agree within twice the kernel's own run-to-run spread, measured here by repeated calls (the
practice of test_gpu_f64_reference.py): float-atomic order differs between the two dispatches as between any two calls."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import backward_kwargs, lego_camera, render_kwargs, sub
import parity
import schedule_reference as S

pytestmark = pytest.mark.gpu

#          W     H     N     splat sigma in pixels
GRIDS = [(16, 16, 3000, 2.0), (112, 16, 3000, 2.0), (48, 48, 3000, 2.0), (4080, 16, 4000, 2.0), (256, 256, 4000, 2.0), (4112, 16, 4000, 2.0),
         (368, 2672, 5000, 2.5), (1040, 1008, 5000, 2.5), (1024, 1024, 6000, 3.0), (1023, 1021, 6000, 3.0), (272, 3856, 4800, 0.8)]
LARGE = (1024, 1024, 3000, 14.0)        # D >= 20 N: 8x8 backward blocks, nothing filed
LIMIT = GRIDS[8]
GRID_IDS = [f"{g[0]}x{g[1]}" for g in GRIDS]
BG = (0.1, 0.2, 0.3)


def _tiles(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


@functools.lru_cache(maxsize=None)
def _case(W, H, N, sigma_px, frame=0):
    """Scene, camera and the oracle's forward, made once and shared (read-only).  Splat size is set in pixels through the focal
    length (set by the width); on a strip image the scene is scaled by H / W along the camera's y axis, so that it fills the strip."""
    from oracle import oracle
    cams, scenes = sub("cameras"), sub("scenes")
    cam = lego_camera(cams, frame, W, H)
    sc = scenes.synthetic_scene(N, sigma_px * 4.0 / cam["fx"], 0.5, seed=7 * W + H)
    if max(W, H) > 4 * min(W, H):
        axis = np.asarray(cam["world_to_camera"], np.float64)[:3, 1].copy()     # the camera's y axis in world space: depths stay
        axis /= np.linalg.norm(axis)
        m = np.asarray(sc["means"], np.float64)
        sc["means"] = (m + (H / W - 1.0) * (m @ axis)[:, None] * axis[None, :]).astype(np.float32)
    kw = render_kwargs(sc, cam, width=W, height=H, bg=BG)
    ref = oracle.render_gaussians(**kw, threads=8)          # (threads: the same bits, pixels are independent)
    dpix = (np.random.default_rng(W + H).normal(0, 1, (H, W, 3)) / (H * W * 3)).astype(np.float32)
    return {"sc": sc, "cam": cam, "kw": kw, "ref": ref, "dpix": dpix, "W": W, "H": H, "N": N, "D": int(ref[2]["point_list"].shape[0])}


@functools.lru_cache(maxsize=None)
def _oracle_backward(W, H, N, sigma_px):
    from oracle import oracle
    c = _case(W, H, N, sigma_px)
    return oracle.backward(**backward_kwargs(c["sc"], c["cam"], c["kw"], c["ref"][2], c["dpix"]))


def _dev():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dev


def _to_dev(sc, dev):
    return {k: torch.as_tensor(np.ascontiguousarray(v, np.float32)).to(dev) for k, v in sc.items()}


# ---- cost tables ----
def _walked(cost):
    return (np.asarray(cost, np.int64) << 16).astype(np.int32)


def cost_tables(n_tiles):
    """(name, int32 [4 * 4096] or None = what the previous frame left) in the order they are rendered."""
    full = 4 * S.FO_MAX_TILES
    rng = np.random.default_rng(n_tiles)
    z = lambda: np.zeros(full, np.int32)
    t = np.arange(n_tiles)
    heavy_first, heavy_last, desc, asc, past = z(), z(), z(), z(), z()
    heavy_first[2], heavy_last[4 * (n_tiles - 1) + 1] = 0x7FFF << 16, 0x7FFF << 16
    desc[4 * t + t % 4] = _walked(n_tiles - t)              # strictly descending tile costs, carried by one wave each
    asc[4 * t + (t + 1) % 4] = _walked(t + 1)
    past[4 * n_tiles:] = rng.integers(1, 2 ** 31, full - 4 * n_tiles).astype(np.int32)
    return [("zero", z()), ("0x7FFFFFFF", np.full(full, 0x7FFFFFFF, np.int32)), ("0xFFFFFFFF", np.full(full, -1, np.int32)),
            ("garbage", rng.integers(-2 ** 31, 2 ** 31, full).astype(np.int32)), ("heavy first", heavy_first), ("heavy last", heavy_last),
            ("descending", desc), ("ascending", asc), ("past n_tiles", past), ("previous frame's", None)]


# ---- gsr_forward_count + gsr_forward_render over buffers the test owns ----
class Driver:
    """One scene and one geom workspace; every frame's outputs are poisoned before the calls."""

    def __init__(self, sc, dev):
        self._lib, self._host = sub("_lib"), sub("_host")
        self.L, self.dev = self._lib.lib(), dev
        n = self.N = int(np.asarray(sc["means"]).reshape(-1, 3).shape[0])
        t = lambda a, shape: torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(shape).to(dev)
        self.inputs = [t(sc["means"], (n, 3)), t(sc["scales"], (n, 3)), t(sc["rotations"], (n, 4)), t(sc["opacities"], (n,)), t(sc["shs"], (n * 16, 3))]
        self.scene = self._lib.GsrScene(n, *[self._host.ptr(x) for x in self.inputs], 3, 1.0, 1)
        i32, f32 = torch.int32, torch.float32
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        self.geom_names = ["radii", "tiles_touched", "point_offsets", "points_xy_image", "depths", "cov3Ds", "colors", "conic_opacity", "clamped_state"]
        self.geom_bufs = [e((n,), i32), e((n,), i32), e((n,), i32), e((n, 2), f32), e((n,), f32), e((n, 6), f32), e((n, 3), f32), e((n, 4), f32), e((n, 3), f32)]
        self.geom = self._lib.GsrGeom(*[self._host.ptr(b) for b in self.geom_bufs], None, None)
        self.gws = torch.full((int(self.L.gsr_geom_workspace_bytes(n)),), 0xA5, dtype=torch.uint8, device=dev)     # a fresh workspace's garbage
        c_off, o_off = C.c_size_t(0), C.c_size_t(0)
        assert self.L.gsr_fwd_order_tables_offset(n, C.byref(c_off), C.byref(o_off)) == 0
        self.cost = self.gws[c_off.value:c_off.value + 16 * S.FO_MAX_TILES].view(i32)
        self.order = self.gws[o_off.value:o_off.value + 4 * S.FO_MAX_TILES].view(i32)
        self.stream = self._host.stream_ptr(dev)

    def frame(self, kw, W, H, table=None):
        """Render one frame.  Returns (outputs as device tensors, the cost table the frame inherited, the order it made)."""
        L, lib, host, dev = self.L, self._lib, self._host, self.dev
        i32, f32 = torch.int32, torch.float32
        if table is not None:
            self.cost.copy_(torch.as_tensor(table))
        inherited = self.cost.cpu().numpy().copy()
        # poison: tile 0 is a valid tile, so a slot the order kernel misses shows as a duplicate, never as a wild index
        self.order.fill_(0 if _tiles(W, H) <= S.FO_MAX_TILES else -3)
        cam = host.make_camera(kw["viewmatrix"], kw["projmatrix"], kw["campos"], kw["background"], kw["tan_fovx"], kw["tan_fovy"], W, H)
        D = C.c_int64(0)
        assert L.gsr_forward_count(C.byref(self.scene), C.byref(cam), C.byref(self.geom), host.ptr(self.gws), self.gws.numel(), C.byref(D), self.stream) == 0
        D = D.value
        assert D > 0
        tiles = _tiles(W, H)
        img = [torch.full((H, W, 3), float("nan"), dtype=f32, device=dev), torch.full((H, W), float("nan"), dtype=f32, device=dev),
               torch.full((H, W), float("nan"), dtype=f32, device=dev), torch.full((H, W), -1, dtype=i32, device=dev)]
        ranges = torch.full((tiles, 2), -1, dtype=i32, device=dev)
        point_list = torch.full((D,), -1, dtype=i32, device=dev)
        masks = torch.empty((D + 16,), dtype=torch.uint8, device=dev)[:D]
        order = torch.full((int(L.gsr_block_order_ints(W, H)),), -9, dtype=i32, device=dev)
        bws = torch.empty(int(L.gsr_binning_workspace_bytes(self.N, D, W, H)), dtype=torch.uint8, device=dev)
        b = lib.GsrBinning(D, host.ptr(point_list), host.ptr(ranges), host.ptr(masks), host.ptr(order), None, 0)
        image = lib.GsrImage(*[host.ptr(x) for x in img])
        assert L.gsr_forward_render(C.byref(self.scene), C.byref(cam), C.byref(self.geom), C.byref(b), C.byref(image), host.ptr(self.gws), self.gws.numel(),
                                    host.ptr(bws), bws.numel(), self.stream) == 0
        torch.cuda.synchronize()
        out = dict(zip(self.geom_names, self.geom_bufs))
        out.update(image=img[0], depth=img[1], final_Ts=img[2], n_contrib=img[3], ranges=ranges, point_list=point_list, masks=masks, block_order=order)
        return out, inherited, self.order.cpu().numpy().copy()


FRAME_KEYS = ["image", "depth", "final_Ts", "n_contrib", "ranges", "point_list"]


def _check_frame(out, ref, name):
    """Nothing poisoned survives; integers equal the oracle's exactly; floats meet parity's forward contract."""
    for k in ("image", "depth", "final_Ts"):
        assert not bool(torch.isnan(out[k]).any()), f"{name}: a poisoned pixel of {k} survived: some tile never ran"
    for k in ("n_contrib", "ranges", "point_list"):
        assert int(out[k].min()) >= 0, f"{name}: a poisoned entry of {k} survived"
    parity.compare_forward((out["image"], out["depth"], out), ref)
    got, want = parity.to_np(out["n_contrib"]), ref[2]["n_contrib"]
    for y, x in np.argwhere(got != want)[:8]:                # (printed before the assertion: what kind of difference it is)
        print(f"{name}: n_contrib[{y}, {x}] = {got[y, x]}, oracle {want[y, x]}; final_T {float(out['final_Ts'][y, x]):.9g}, oracle {ref[2]['final_Ts'][y, x]:.9g}")
    parity.assert_exact("n_contrib", got, want)


def _check_filing(out, c, name, filed):
    """The block order this frame's forward left, against the masks, ranges and n_contrib it left."""
    W, H = c["W"], c["H"]
    exp = (S.expected_block_queues(parity.to_np(out["ranges"]), parity.to_np(out["n_contrib"]), parity.to_np(out["masks"]), W, H) if filed
           else S.unfiled_block_queues())
    o = parity.to_np(out["block_order"])
    assert o.size == S.bo_ints(W, H), name
    S.check_block_order(o, exp, _tiles(W, H))


@pytest.mark.parametrize("grid", GRIDS[:-1], ids=GRID_IDS[:-1])
def test_every_tile_runs_whatever_the_cost_table_holds(grid):
    """A fresh workspace's bytes, then ten cost tables, on one workspace: each yields a permutation by class, no poisoned pixel
    survives, the oracle's integers exactly and its image within the forward contract, and the same bits under every table."""
    c = _case(*grid)
    W, H = c["W"], c["H"]
    n_tiles = _tiles(W, H)
    drv = Driver(c["sc"], _dev())
    first = None
    for name, table in [("fresh workspace", None)] + cost_tables(n_tiles):
        out, inherited, order = drv.frame(c["kw"], W, H, table)
        assert table is None or np.array_equal(inherited, table)
        S.check_fwd_order(order, inherited, n_tiles)
        left = drv.cost.cpu().numpy()                            # what this frame's waves left for the next one
        assert np.array_equal(left[4 * n_tiles:], inherited[4 * n_tiles:]), f"{name}: the blend wrote costs past the image's tiles"
        assert ((left[:4 * n_tiles] & 0xFFFF) == 0).all() and (left[:4 * n_tiles] >= 0).all(), f"{name}: a wave's cost is not (ticks << 16)"
        if first is None:
            _check_frame(out, c["ref"], name)
            _check_filing(out, c, name, filed=True)
            first = {k: out[k].clone() for k in FRAME_KEYS}
            continue
        for k in ("image", "depth", "final_Ts"):
            assert not bool(torch.isnan(out[k]).any()), f"{name}: a poisoned pixel of {k} survived: some tile never ran"
        for k in FRAME_KEYS:                                     # bit for bit (NaN-free, so torch.equal is a bit comparison up to -0)
            assert torch.equal(out[k], first[k]), f"cost table '{name}': {k} differs from the first frame's"


def test_past_the_limit_both_schedules_are_off():
    """4097 tiles: row-major forward (the cost table and the order are left as the test wrote them), header-only block order."""
    c = _case(*GRIDS[-1])
    W, H = c["W"], c["H"]
    assert _tiles(W, H) == S.FO_MAX_TILES + 1
    drv = Driver(c["sc"], _dev())
    table = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, 4 * S.FO_MAX_TILES).astype(np.int32)
    out, inherited, order = drv.frame(c["kw"], W, H, table)
    _check_frame(out, c["ref"], "4097 tiles")
    assert np.array_equal(drv.cost.cpu().numpy(), table), "the cost table of an image past the limit was written"
    assert (order == -3).all(), "the tile order of an image past the limit was written"
    _check_filing(out, c, "4097 tiles", filed=False)


def test_a_second_views_costs():
    """The trainer's case: three cameras in turn on one workspace, two rounds.  Every frame orders its tiles by the costs ANOTHER
    view left, and must render its own view."""
    W, H, N, px = LIMIT
    views = [_case(W, H, N, px, frame=f) for f in (0, 1, 2)]
    drv = Driver(views[0]["sc"], _dev())                         # one scene (the seed does not depend on the view) under three cameras
    assert all(np.array_equal(v["sc"]["means"], views[0]["sc"]["means"]) for v in views)
    for rnd in range(2):
        for i, v in enumerate(views):
            out, inherited, order = drv.frame(v["kw"], W, H)
            name = f"round {rnd}, view {i}"
            S.check_fwd_order(order, inherited, _tiles(W, H))
            if rnd or i:
                assert len(set(S.fwd_classes(inherited, _tiles(W, H)).tolist())) > 1, f"{name}: the inherited costs are flat -- nothing was ordered"
            _check_frame(out, v["ref"], name)
            _check_filing(out, v, name, filed=True)


# ---- through render_gaussians and backward(): the block order, and the backward that walks it ----
REPEATS = 4      # calls per dispatch behind the run-to-run spread


def _np_grads(g, extra=()):
    return {k: parity.to_np(g[k]).copy() for k in list(parity.GRAD_KEYS) + list(extra)}


def _render(c, dev, **more):
    sc = _to_dev(c["sc"], dev)
    kw = render_kwargs(sc, c["cam"], width=c["W"], height=c["H"], bg=BG)
    return sc, kw, sub("forward").render_gaussians(**kw, **more)


def _filing_of(buf, c, filed):
    masks, _, order = buf["point_list"]._gsr_block_masks
    out = {"ranges": buf["ranges"], "n_contrib": buf["n_contrib"], "masks": masks, "block_order": order}
    _check_filing(out, c, f"{c['W']}x{c['H']}", filed)


def _both_dispatches(c, sc, kw, buf, ordered, extra=(), **more):
    """backward() from the forward's own buffers (masks and block order), and with `ranges` cloned (identity broken: no masks, no
    order), REPEATS times each.  Returns (ordered, unordered) gradients after holding them to each other: per array, the first
    calls of the two dispatches differ by at most twice the run-to-run spread, which is the largest difference between any two
    calls of one dispatch (one pair alone is too noisy an estimate of a maximum over float-atomic orders: dL_drot's spread moved
    by 2x between pairs on the ill-conditioned splats of these scenes)."""
    bwd = sub("backward")
    run = lambda b: _np_grads(bwd.backward(**backward_kwargs(sc, c["cam"], kw, b, torch.as_tensor(c["dpix"]).to(buf["ranges"].device)), **more), extra)
    own = [run(buf) for _ in range(REPEATS)]
    assert bwd.backward.last_call_used_forward_masks
    loose = dict(buf, ranges=buf["ranges"].clone())
    other = [run(loose) for _ in range(REPEATS)]
    assert not bwd.backward.last_call_used_forward_masks
    rows = []
    for k in own[0]:
        spread = max(parity.grad_margin(runs[i][k], runs[j][k])[1] for runs in (own, other) for i in range(REPEATS) for j in range(i))
        diff = parity.grad_margin(own[0][k], other[0][k])[1]
        rows.append((k, diff, spread))
    print(f"\n{c['W']}x{c['H']} ({'ordered' if ordered else 'band order'} vs no masks): array, difference, run-to-run spread (max err / max|g|)")
    for r in rows:
        print("  %-16s %.3e   %.3e" % r)
    for k, diff, spread in rows:
        assert diff <= 2.0 * spread, f"{k}: the two dispatches differ by {diff:.3e} of max|g|, run-to-run spread {spread:.3e}"
    return own[0], other[0]


@pytest.mark.parametrize("grid", GRIDS + [LARGE], ids=GRID_IDS + ["1024x1024-large-splats"])
def test_block_order_is_what_the_masks_say_and_the_backward_walks_it(grid):
    c = _case(*grid)
    dev = _dev()
    tiles = _tiles(c["W"], c["H"])
    filed = tiles <= S.BO_MAX_TILES and c["D"] < 20 * c["N"]      # gsr_bwd_block_px: 8x4 blocks below 20 pairs per Gaussian
    assert filed == (grid is not LARGE and grid is not GRIDS[-1])
    sc, kw, (img, depth, buf) = _render(c, dev)
    for k in ("point_list", "ranges", "n_contrib"):
        parity.assert_exact(k, buf[k], c["ref"][2][k])
    _filing_of(buf, c, filed)
    own, other = _both_dispatches(c, sc, kw, buf, filed)
    ref = _oracle_backward(*grid)
    parity.compare_backward(own, ref)
    parity.compare_backward(other, ref)


def test_block_order_of_a_capacity_mode_frame():
    """K > D: the queues are filed from device-side counts; the masks buffer is K long, the lists end at D."""
    c = _case(*GRIDS[4])
    dev = _dev()
    D = c["D"]
    sc, kw, (img, depth, buf) = _render(c, dev, capacity=2 * D + 17, capacity_hint=D)
    assert sub("forward").rendered_count(buf) == (D, False)
    parity.assert_exact("ranges", buf["ranges"], c["ref"][2]["ranges"])
    parity.assert_exact("n_contrib", buf["n_contrib"], c["ref"][2]["n_contrib"])
    parity.assert_exact("point_list", buf["point_list"][:D], c["ref"][2]["point_list"])
    _filing_of(buf, c, True)
    g = sub("backward").backward(**backward_kwargs(sc, c["cam"], kw, buf, torch.as_tensor(c["dpix"]).to(dev)))
    assert sub("backward").backward.last_call_used_forward_masks
    parity.compare_backward(_np_grads(g), _oracle_backward(*GRIDS[4]))


def test_the_absgrad_and_aux_kernels_walk_the_same_order():
    """blend_backward_splat_kernel<8,4,true,AUX,ABS> on the 4096-tile grid.  The auxiliary images' gradients are zero, so that the
    nine arrays are still the oracle's (which has no auxiliary backward); the magnitudes column and dL_dinv_depths are held
    between the two dispatches."""
    c = _case(*LIMIT)
    dev = _dev()
    sc, kw, (img, depth, buf) = _render(c, dev)
    _filing_of(buf, c, True)
    zero = torch.zeros((c["H"], c["W"]), device=dev)
    own, other = _both_dispatches(c, sc, kw, buf, True, extra=("dL_dmean2D_abs", "dL_dinv_depths"), absgrad=True, dL_ddepth_image=zero,
                                  dL_dalpha_image=zero)
    assert np.abs(own["dL_dmean2D_abs"]).max() > 0
    ref = _oracle_backward(*LIMIT)
    parity.compare_backward(own, ref)
    parity.compare_backward(other, ref)


def test_the_antialiased_frame_orders_and_files_alike():
    """rasterize_mode="antialiased" on the 4096-tile grid: preprocess_kernel<AA> hosts its own copy of the order workgroup, and the
    frame's effective opacities feed the same filing.  The oracle has no antialiased mode; its blend backward, given this frame's
    own buffers (conic_opacity carries opacity * rho), states the three blend-stage gradients."""
    from oracle import oracle
    c = _case(*LIMIT)
    dev = _dev()
    host, L = sub("_host"), sub("_lib").lib()
    W, H, N = c["W"], c["H"], c["N"]
    _render(c, dev, rasterize_mode="antialiased")               # (the workspace now holds an antialiased frame's costs)
    torch.cuda.synchronize()
    gws = host.workspace("geom", L.gsr_geom_workspace_bytes(N), dev, host.raw_stream(dev))
    c_off, o_off = C.c_size_t(0), C.c_size_t(0)
    assert L.gsr_fwd_order_tables_offset(N, C.byref(c_off), C.byref(o_off)) == 0
    inherited = gws[c_off.value:c_off.value + 16 * S.FO_MAX_TILES].view(torch.int32).cpu().numpy().copy()
    gws[o_off.value:o_off.value + 4 * S.FO_MAX_TILES].view(torch.int32).fill_(0)
    sc, kw, (img, depth, buf) = _render(c, dev, rasterize_mode="antialiased")
    torch.cuda.synchronize()
    assert host.workspace("geom", L.gsr_geom_workspace_bytes(N), dev, host.raw_stream(dev)) is gws
    S.check_fwd_order(gws[o_off.value:o_off.value + 4 * S.FO_MAX_TILES].view(torch.int32).cpu().numpy(), inherited, _tiles(W, H))
    assert bool(torch.isfinite(img).all())
    _filing_of(buf, c, True)
    own, other = _both_dispatches(c, sc, kw, buf, True, rasterize_mode="antialiased")
    host_buf = {k: parity.to_np(v) for k, v in buf.items()}
    ref = oracle.backward(**backward_kwargs(c["sc"], c["cam"], c["kw"], host_buf, c["dpix"]))
    for k in ("dL_dcolor", "dL_dmean2D", "dL_dconic"):
        parity.assert_grad(k, own[k], ref[k])
        parity.assert_grad(k, other[k], ref[k])
