"""Capacity-mode binning (include/gsr_capacity.h) at the edges of its launch geometry, on frames of a few thousand pairs.  Every
capacity launch is sized from the capacity K and works on min(D, K) items, so what can go wrong sits where K and D meet a radix
block (D a whole number of 1024-item chunks, K = D with no spare slot, K one item into an empty block, K many empty blocks past
D), where K alone picks the tier or switches the super-block scan on (the thresholds are read from csrc/gsr_internal.h, so a retune
moves these cases with it), in the single partition pass that is both FINAL and fed by the expansion's histogram, in what a
caller-owned workspace held before, and in the accumulator hand-over between frames of different sizes through one cached
workspace.  For K >= D the outputs are the sized path's bit for bit; for D > K every write stays inside the K-sized buffers.
The last test runs this file again under each GSR_DEBUG path (the capacity twins of the kernels that tests/test_gpu_alt_paths.py
holds on the sized path).  tests/test_gpu_capacity.py has the cases at the workload's own sizes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG_NAME, ROOT, lego_camera, render_kwargs, sub
import parity
from test_gpu_capacity import BO_FLAG, _grads, _render, _same_floats, _same_ints, _staged_entries, _to_dev

pytestmark = pytest.mark.gpu

HEADER_NAMES = ("GSR_RADIX_TINY_CHUNK", "GSR_RADIX_TINY_N", "GSR_RADIX_SMALL_N", "GSR_RADIX_CHUNK", "GSR_RADIX_PREFIX_NB", "GSR_SMALL_SORT_N")
_header = {}


def _const(name):
    """A constant of csrc/gsr_internal.h, from the header's text (plain integers, shifts and products)."""
    if not _header:
        with open(os.path.join(ROOT, PKG_NAME, "csrc", "gsr_internal.h")) as f:
            text = f.read()
        for n in HEADER_NAMES:
            m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+(.+?)[ \t]*(?://.*)?$" % n, text, re.M)
            assert m, f"{n} is not defined in gsr_internal.h"
            expr = m.group(1)
            assert re.fullmatch(r"[0-9()<*+ \t]+", expr), f"{n}: cannot read '{expr}'"
            _header[n] = int(eval(expr, {"__builtins__": {}}))
            assert _header[n] > 0, n
    return _header[name]


def _chunk_up(D):
    c = _const("GSR_RADIX_TINY_CHUNK")
    return -(-D // c) * c


# K by name: D is only known once the frame has been rendered
CAPACITIES = {
    "D": lambda D: D,
    "D+1": lambda D: D + 1,
    "chunk_multiple": _chunk_up,                                  # the last block full or (D a multiple already) no spare slot
    "chunk_multiple+1": lambda D: _chunk_up(D) + 1,               # one item into an otherwise empty block
    "40_empty_blocks": lambda D: D + 40 * _const("GSR_RADIX_TINY_CHUNK") + 3,
    "TINY_N": lambda D: _const("GSR_RADIX_TINY_N"),               # the last K of the 1024-item tier
    "TINY_N+1": lambda D: _const("GSR_RADIX_TINY_N") + 1,         # K alone picks the 2048-item tier
    "SMALL_N+1": lambda D: _const("GSR_RADIX_SMALL_N") + 1,       # ... the GSR_RADIX_CHUNK tier
    "PREFIX_NB+1": lambda D: _const("GSR_RADIX_PREFIX_NB") * _const("GSR_RADIX_CHUNK") + 1,   # ... and the super-block scan
}
EVERY_FRAME = ["D", "D+1", "chunk_multiple", "chunk_multiple+1", "40_empty_blocks", "TINY_N", "TINY_N+1"]
LARGE = ["SMALL_N+1", "PREFIX_NB+1"]
FRAMES = ["giants", "tiny_grid", "two_pass", "one_plane", "nine_octaves", "mostly_culled"]


def _capacity(name, D):
    """K for a frame of D pairs, and that it is where its name says: D in the 1024-item tier without a super-block scan, the named
    K past the threshold it is named after."""
    tiny_c, tiny_n, small_n = _const("GSR_RADIX_TINY_CHUNK"), _const("GSR_RADIX_TINY_N"), _const("GSR_RADIX_SMALL_N")
    chunk, prefix_nb = _const("GSR_RADIX_CHUNK"), _const("GSR_RADIX_PREFIX_NB")
    assert tiny_n < small_n and tiny_c < chunk
    assert 0 < D and D + 40 * tiny_c + 3 < tiny_n, D                  # D, and every K built from D, in the 1024-item tier
    assert -(-D // tiny_c) <= prefix_nb
    K = CAPACITIES[name](D)
    assert K >= D
    if name in ("chunk_multiple", "chunk_multiple+1"):
        assert (K - (name == "chunk_multiple+1")) % tiny_c == 0 and K - D <= tiny_c
    if name == "TINY_N+1":
        assert K > tiny_n and K <= small_n
    if name == "SMALL_N+1":
        assert K > small_n and -(-K // chunk) <= prefix_nb
    if name == "PREFIX_NB+1":
        assert K > small_n and -(-K // chunk) > prefix_nb            # GSR_RADIX_CHUNK blocks, more of them than GSR_RADIX_PREFIX_NB
    return K


def _depth_scene(scenes, near, far, n):
    """The generator of test_gpu_parity.test_depth_ranges_and_the_device_side_pass_plan."""
    sc = scenes.synthetic_scene(n, 0.03, 0.5, int(near * 100) + n)
    rng = np.random.default_rng(n)
    depth = rng.uniform(near, far, n).astype(np.float32)
    depth[::7] = -depth[::7]
    sc["means"][:, 2] = -depth
    sc["means"][:, :2] = (rng.uniform(-0.4, 0.4, (n, 2)) * np.abs(depth)[:, None]).astype(np.float32)
    sc["scales"] *= np.abs(depth)[:, None] / 3.0
    return sc


def _build(name):
    scenes, cams = sub("scenes"), sub("cameras")
    if name == "giants":            # test_gpu_parity.test_expansion_by_output_block's giants_only: 12 Gaussians over all 256 tiles
        sc = scenes.synthetic_scene(12, 0.004, 0.2, 77 + 12)
        sc["scales"][:] = 8.0
        sc["means"] *= 0.2
        return sc, lego_camera(cams, 1, 256, 256)
    if name == "tiny_grid":         # test_gpu_handoff_matrix's shape: 3 x 2 partial tiles
        return scenes.synthetic_scene(300, 0.05, 0.6, 7), lego_camera(cams, 3, 40, 24)
    if name == "two_pass":          # 17 x 16 tiles: 9 tile bits, passes of 5 + 4
        return scenes.synthetic_scene(9001, 0.02, 0.5, 41), lego_camera(cams, 2, 272, 256)
    if name in ("one_plane", "nine_octaves"):
        near, far, n = (3.0, 3.0, 700) if name == "one_plane" else (0.25, 90.0, 9000)
        return _depth_scene(scenes, near, far, n), cams.nerf_camera(np.eye(4).tolist(), 208, 144, 0.6911112)
    assert name == "mostly_culled"
    n = 9001
    sc = scenes.synthetic_scene(n, 0.004, 0.2, 77 + n)
    cam = lego_camera(cams, 1, 256, 256)
    centre = np.asarray(cam["camera_center"], np.float32)
    away = sc["means"] - centre
    keep = np.arange(n) % 5 == 0
    sc["means"][~keep] = centre - away[~keep]
    return sc, cam


class Frame:
    """One frame's inputs, its sized render and sized backward: made once per process, never written afterwards."""

    def __init__(self, name):
        self.name = name
        self.dev = dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        self.sc_np, self.cam = _build(name)
        self.sc = _to_dev(self.sc_np, dev)
        self.kw = render_kwargs(self.sc, self.cam)
        self.H, self.W = self.kw["image_height"], self.kw["image_width"]
        sub("forward")._backward_seen = True        # the trainer's state: the forward pre-clears the backward workspace
        self.ref = _render(self.kw)
        self.D, self.N = int(self.ref[2]["point_list"].shape[0]), int(self.sc["means"].shape[0])
        tiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        visible = int((self.ref[2]["radii"] > 0).sum())
        if name == "giants":
            assert self.D == 3072 and self.D == 3 * _const("GSR_RADIX_TINY_CHUNK") and tiles == 256     # three whole chunks, 8 tile bits
        if name == "tiny_grid":
            assert tiles == 6 and self.D > 0
        if name == "two_pass":
            assert 256 < tiles <= 512 and self.N > _const("GSR_SMALL_SORT_N") and self.N % 256 != 0 and self.D > 2 * _const("GSR_RADIX_TINY_CHUNK")
        if name == "one_plane":
            assert self.N <= _const("GSR_SMALL_SORT_N") and self.D > self.N
        if name == "nine_octaves":
            assert self.N > _const("GSR_SMALL_SORT_N") and self.D > self.N
        if name == "mostly_culled":
            assert 0 < visible < self.N // 3 and self.D > 0
        rng = np.random.default_rng(1)
        self.dpix = torch.as_tensor((rng.normal(0, 1, (self.H, self.W, 3)) / (self.H * self.W * 3)).astype(np.float32)).to(dev)
        self.g_ref = _grads(self.sc, self.cam, self.kw, self.ref[2], self.dpix)
        self.filed = int(self.ref[2]["point_list"]._gsr_block_masks[2][BO_FLAG])
        self.staged = _staged_entries(self.ref[2], self.H, self.W)
        torch.cuda.synchronize()


_frames = {}


def _frame(name):
    if name not in _frames:
        _frames[name] = Frame(name)
    return _frames[name]


def _same_frame(f, got, K, ref=None):
    """A capacity frame with K >= D against the sized frame: integers, images, staged block masks, count and `filed` flag equal,
    the backward within parity.compare_backward's bounds (float-atomic order)."""
    ref = f.ref if ref is None else ref
    D = f.D
    assert got[2]["point_list"].shape[0] == K and sorted(got[2]) == sorted(ref[2])
    assert sub("forward").rendered_count(got[2]) == (D, False)
    _same_ints(got[2], ref[2], D)
    _same_floats(got, ref)
    m_got, m_ref = got[2]["point_list"]._gsr_block_masks[0], ref[2]["point_list"]._gsr_block_masks[0]
    assert torch.equal(m_got[f.staged], m_ref[f.staged]), "block_masks"
    assert int(got[2]["point_list"]._gsr_block_masks[2][BO_FLAG]) == f.filed
    parity.compare_backward(_grads(f.sc, f.cam, f.kw, got[2], f.dpix), f.g_ref)


def _same_sized(f, got):
    """A later sized frame against the first."""
    assert got[2]["point_list"].shape[0] == f.D
    _same_ints(got[2], f.ref[2], f.D)
    _same_floats(got, f.ref)


CASES = [(fr, k) for fr in FRAMES for k in EVERY_FRAME + (LARGE if fr in ("giants", "two_pass") else [])]


@pytest.mark.parametrize("frame,cap", CASES)
def test_every_capacity_from_D_up_gives_the_sized_frame(frame, cap):
    f = _frame(frame)
    K = _capacity(cap, f.D)
    got = _render(f.kw, capacity=K, capacity_hint=f.D)     # the hint: nothing but the buffers and the launches is sized from K
    _same_frame(f, got, K)
    torch.cuda.synchronize()


@pytest.mark.parametrize("frame", ["giants", "two_pass"])
def test_a_capacity_frame_against_the_oracle(oracle, frame):
    """The capacity path's own ground truth: K = D + 1 against the CPU oracle, not against the sized path."""
    f = _frame(frame)
    got = _render(f.kw, capacity=f.D + 1, capacity_hint=f.D)
    assert sub("forward").rendered_count(got[2]) == (f.D, False)
    ref = oracle.render_gaussians(**render_kwargs(f.sc_np, f.cam))
    assert int(parity.to_np(ref[2]["point_list"]).size) == f.D
    parity.compare_forward((got[0], got[1], dict(got[2], point_list=got[2]["point_list"][:f.D])), ref)


GUARD = 1 << 16


def _guarded_buffers(f, K, body, tail):
    """Caller-owned capacity buffers for K pairs, every byte `body`, each followed by a 64 KiB guard of `tail` bytes (the block
    masks' guard begins at K: the 16 spare bytes behind them are read, never written).  Returns (capacity_buffers, guards)."""
    need = int(sub("_lib").lib().gsr_binning_workspace_bytes(f.N, K, f.W, f.H))
    sizes = {"point_list": 4 * K, "block_masks": K, "binning_ws": need}
    raw = {}
    for k, n in sizes.items():
        raw[k] = torch.full((n + (16 if k == "block_masks" else 0) + GUARD,), tail, dtype=torch.uint8, device=f.dev)
        raw[k][:n] = body
    bufs = {"point_list": raw["point_list"][:4 * K].view(torch.int32), "block_masks": raw["block_masks"][:K], "binning_ws": raw["binning_ws"][:need]}
    return bufs, lambda: {k: raw[k][n:].clone() for k, n in sizes.items()}


def _guards_intact(guards, before, what):
    torch.cuda.synchronize()
    now = guards()
    for k in before:
        assert torch.equal(now[k], before[k]), f"{what} wrote past {k}"


@pytest.mark.parametrize("body", [0xFF, 0x00])
@pytest.mark.parametrize("cap", ["D", "chunk_multiple+1"])
@pytest.mark.parametrize("frame", ["giants", "tiny_grid", "two_pass"])
def test_a_frame_does_not_depend_on_what_its_buffers_held(frame, cap, body):
    f = _frame(frame)
    K = _capacity(cap, f.D)
    bufs, guards = _guarded_buffers(f, K, body, 0x3C)
    before = guards()
    got = _render(f.kw, capacity=K, capacity_hint=f.D, capacity_buffers=bufs)
    assert got[2]["point_list"].data_ptr() == bufs["point_list"].data_ptr()
    _guards_intact(guards, before, f"K={K}: the forward")
    _same_frame(f, got, K)                                   # (runs a backward on the frame)
    _guards_intact(guards, before, f"K={K}: the backward")


@pytest.mark.parametrize("frame", ["giants", "two_pass"])
def test_sized_and_capacity_frames_through_one_cached_workspace(frame):
    """Every pass clears the next pass's accumulator rows, as many as ITS item count asks for: K in one frame, D in the next, one
    row in an overflowed one -- through the library's cached (grow-only) workspaces, largest frame early."""
    f = _frame(frame)
    D, chunk = f.D, _const("GSR_RADIX_TINY_CHUNK")
    assert D > chunk
    first = _render(f.kw)
    _same_sized(f, first)
    steps = [("capacity", _capacity("PREFIX_NB+1", D)), ("capacity", D), ("overflow", chunk), ("capacity", D + 1), ("sized", None),
             ("capacity", _capacity("TINY_N+1", D)), ("overflow", 1), ("capacity", _chunk_up(D))]
    for i, (kind, K) in enumerate(steps):
        if kind == "sized":
            _same_sized(f, _render(f.kw))
            continue
        got = _render(f.kw, capacity=K, capacity_hint=D)
        if kind == "overflow":
            assert sub("forward").rendered_count(got[2]) == (D, True), (i, K)
        else:
            _same_frame(f, got, K, first)
    torch.cuda.synchronize()


OVERFLOWS = [("giants", k) for k in (0, 1, 1023, 1024, 1025, 2048, "D-1")] + [("two_pass", "chunk"), ("two_pass", "D-1")]


@pytest.mark.parametrize("frame,cap", OVERFLOWS)
def test_an_overflowed_frame_at_the_block_edges_stays_inside_its_buffers(frame, cap):
    """D > K with K below, on and just past a block boundary: the call succeeds, the count says so, the guard tails behind
    point_list, block_masks and the binning workspace are untouched by the forward and by a backward on that frame, ids and ranges
    stay inside the frame, and the sized path afterwards is undisturbed.  (Bounded by construction: if this ever faults, the
    out-of-range write is to be found from the guards and the code, not by running it again.)"""
    f = _frame(frame)
    D = f.D
    K = D - 1 if cap == "D-1" else _const("GSR_RADIX_TINY_CHUNK") if cap == "chunk" else cap
    assert 0 <= K < D
    bufs, guards = _guarded_buffers(f, K, 0x5A, 0xA5)
    before = guards()
    got = _render(f.kw, capacity=K, capacity_hint=D, capacity_buffers=bufs)
    assert sub("forward").rendered_count(got[2]) == (D, True)
    _guards_intact(guards, before, f"K={K}: the forward")
    if K > 0:
        assert int(got[2]["point_list"].min()) >= 0 and int(got[2]["point_list"].max()) < f.N
    rg = got[2]["ranges"]
    assert int(rg.min()) >= 0 and int(rg.max()) <= K and bool((rg[:, 0] <= rg[:, 1]).all())
    _grads(f.sc, f.cam, f.kw, got[2], f.dpix)
    _guards_intact(guards, before, f"K={K}: the backward")
    _same_sized(f, _render(f.kw))


FORCED = [32, 32 | 4096, 64, 128, 32 | 64 | 128, 256, 1024, 1024 | 2048]


@pytest.mark.parametrize("flags", FORCED)
def test_this_file_on_every_forced_path(flags):
    """GSR_DEBUG (gsr_internal.h has the table; read once per process, hence a child): 64-bit tile items in one pass (giants,
    tiny_grid) and narrowed by the first of two (two_pass); kept through both; the large chunks, the forced super-block scan,
    and both with wide items; always four depth passes; the multi-kernel depth stage for the small frames, with packed and with
    plain depth items.  The thresholds above still hold or are superseded, so the capacities are the same."""
    env = dict(os.environ, GSR_DEBUG=str(flags))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "not test_this_file_on_every_forced_path"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
