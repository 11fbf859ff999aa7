"""Frames built on the host from a seed, for the stages that replay the forward blend's weights over a finished frame's tile lists
(csrc/frame_walk.h: features.hip, distortion.hip, normal_render.hip and, as DEPTH_STAGES, plane_depth.hip and the two depth models
of median_depth.hip), and their kernels behind the C ABI on such a frame.
The kernels clip everything they read, so any n_contrib within a tile's range, any mask bytes and any ids make a valid frame; the
blend forward is not run.  Shared by tools/frame_walk_bits.py and tests/test_gpu_frame_walk.py."""
import ctypes as C
import importlib

import numpy as np
import torch

gsr = importlib.import_module("3dgs-native_amd")
_lib, _host = gsr._lib, gsr._host

LENS = (0, 1, 255, 256, 257, 640)     # list lengths, cycled over the tiles: no batch, one (partial, full), two, three
STAGES = ("features", "distortion", "normal_render")
DEPTH_STAGES = ("plane_depth", "median_depth", "plane_median")   # for tools/frame_walk_bits.py; the contracts of tests/test_gpu_frame_walk.py run over STAGES
# the backwards end in float atomics: their bits repeat only where no destination receives more than two addends -- one tile, every
# Gaussian listed once, one or two waves with pixels (see build_frame's `blocks`)
BACKWARD_SHAPES = {"8x8": dict(W=8, H=8), "16x8": dict(W=16, H=8), "16x16 two blocks": dict(W=16, H=16, empty_blocks=(1, 2))}
PAST = 40                             # with once_per_tile: the last PAST entries of a list lie past every pixel's n_contrib


def build_frame(seed, W, H, lens=LENS, N=700, masks=None, bad_ids=True, once_per_tile=False, empty_blocks=(), record_view=False):
    """Host arrays of one frame.  masks: None, "ff" or "random".  once_per_tile: every list is a prefix of one permutation of the
    Gaussians (each listed once per tile) and n_contrib stays PAST entries short of the list's end.  empty_blocks: 8x8 blocks
    (0-3) of every tile whose pixels get n_contrib = 0.  record_view: xy, conic_opacity and 1/depth are columns of one [N][16] array."""
    rng = np.random.default_rng(seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tile_len = [lens[t % len(lens)] for t in range(gx * gy)]
    starts = np.concatenate([[0], np.cumsum(tile_len)]).astype(np.int64)
    D = int(starts[-1])
    xy = np.stack([rng.uniform(-4, W + 4, N), rng.uniform(-4, H + 4, N)], 1).astype(np.float32)
    a, c = rng.uniform(0.01, 0.2, N), rng.uniform(0.01, 0.2, N)
    b = rng.uniform(-0.9, 0.9, N) * np.sqrt(a * c)
    b[::37] = 3.0 * np.sqrt(a * c)[::37]                      # a few indefinite conics: power > 0 at some pixels
    co = np.stack([a, b, c, rng.uniform(0.02, 1.0, N)], 1).astype(np.float32)
    invd = rng.uniform(0.1, 2.0, N).astype(np.float32)
    point_list = np.zeros(D, np.int32)
    n_contrib = np.zeros((H, W), np.int32)
    perm = rng.permutation(N)
    for t, ln in enumerate(tile_len):
        ids = perm[:ln] if once_per_tile else rng.integers(0, N, ln)
        assert len(ids) == ln, "once_per_tile needs N >= the longest list"
        point_list[starts[t]:starts[t] + ln] = ids
        ty, tx = divmod(t, gx)
        h, w = min(16, H - 16 * ty), min(16, W - 16 * tx)
        top = max(0, ln - PAST) if once_per_tile else ln
        nc = rng.integers(0, top + 1, (h, w))
        nc[rng.random((h, w)) < 0.15] = top                   # the whole list
        for m in (32, 4, 3):                                  # applied counts that are multiples of 32, 4 and 3, and that are not
            sel = rng.random((h, w)) < 0.1
            nc[sel] = nc[sel] // m * m
        nc[rng.random((h, w)) < 0.1] = 0
        for blk in empty_blocks:
            nc[8 * (blk >> 1):8 * (blk >> 1) + 8, 8 * (blk & 1):8 * (blk & 1) + 8] = 0
        n_contrib[16 * ty:16 * ty + h, 16 * tx:16 * tx + w] = nc
    bad = np.zeros(D, bool)
    if bad_ids and D:
        bad = rng.random(D) < 0.04
        point_list[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1 - rng.integers(0, 1000, int(bad.sum())), N + rng.integers(0, 1000, int(bad.sum())))
    ranges = np.stack([starts[:-1], starts[1:]], 1).astype(np.int32)
    mask = None if masks is None else np.full(D, 0xFF, np.uint8) if masks == "ff" else rng.integers(0, 256, D).astype(np.uint8)
    nrm = rng.normal(0, 1, (N, 3))
    fr = dict(W=W, H=H, N=N, D=D, xy=xy, co=co, invd=invd, point_list=point_list, ranges=ranges, n_contrib=n_contrib, masks=mask, bad=bad,
              normals=(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32), record_view=record_view,
              features=rng.normal(0, 1, (N, 64)).astype(np.float32), g_image=rng.normal(0, 1, (H, W, 64)).astype(np.float32),
              acc_seed=(rng.normal(0, 1, (N, 16)) * 1e-3).astype(np.float32), tile_len=tile_len, starts=starts)
    # the plane stages' slopes, drawn last so that every array above keeps its values: of the size of 1/depth over a few pixels (some
    # entries meet the clamp inside a tile), a fifth of the Gaussians at (0, 0) exactly
    fr["slopes"] = (rng.normal(0, 0.15, (N, 2)) * invd[:, None]).astype(np.float32)
    fr["slopes"][rng.random(N) < 0.2] = 0
    return fr


def other_bad_ids(fr, seed):
    """The same frame with every out-of-range id replaced by another out-of-range value."""
    rng = np.random.default_rng(seed)
    out = dict(fr)
    pl = fr["point_list"].copy()
    k = int(fr["bad"].sum())
    pl[fr["bad"]] = np.where(pl[fr["bad"]] < 0, fr["N"] + 5 + rng.integers(0, 1 << 20, k), -7 - rng.integers(0, 1 << 20, k))
    where = np.flatnonzero(fr["bad"])
    pl[where[:1]], pl[where[1:2]] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    out["point_list"] = pl
    return out


def past_every_pixel(fr):
    """Gaussians of a once_per_tile frame whose every list entry lies at or past each pixel's n_contrib."""
    gx = (fr["W"] + 15) // 16
    seen = np.zeros(fr["N"], bool)
    for t, ln in enumerate(fr["tile_len"]):
        ty, tx = divmod(t, gx)
        top = int(fr["n_contrib"][16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].max(initial=0))
        ids = fr["point_list"][fr["starts"][t]:fr["starts"][t] + min(top, ln)]
        seen[ids[(ids >= 0) & (ids < fr["N"])]] = True
    return ~seen


class DeviceFrame:
    """A frame on the device and the kernels of STAGES and DEPTH_STAGES on it, through the C ABI."""

    def __init__(self, fr, dev=None):
        self.fr, self.dev = fr, dev or torch.device("cuda", 0)
        t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(self.dev)
        self.W, self.H, self.N = fr["W"], fr["H"], fr["N"]
        if fr["record_view"]:
            rec = np.zeros((self.N, 16), np.float32)
            rec[:, 0:2], rec[:, 2:6], rec[:, 9] = fr["xy"], fr["co"], fr["invd"]
            self.rec = t(rec)
            base = self.rec.data_ptr()
            xy, co, invd, strides = base, base + 8, base + 36, (16, 16, 16)
        else:
            self.xy, self.co, self.invd = t(fr["xy"]), t(fr["co"]), t(fr["invd"])
            xy, co, invd, strides = self.xy.data_ptr(), self.co.data_ptr(), self.invd.data_ptr(), (2, 4, 1)
        self.point_list, self.ranges, self.n_contrib, self.masks = t(fr["point_list"]), t(fr["ranges"]), t(fr["n_contrib"]), t(fr["masks"])
        self.normals, self.slopes = t(fr["normals"]), t(fr["slopes"])
        common = (self.W, self.H, self.N, fr["D"], xy, strides[0], co, strides[1], _host.ptr(self.point_list), _host.ptr(self.ranges),
                  _host.ptr(self.n_contrib), _host.ptr(self.masks))
        self.frame = _lib.GsrFeaturesFrame(*common)
        self.dframe = _lib.GsrDistortionFrame(*common, invd, strides[2])
        self.L, self.stream = _lib.lib(), _host.raw_stream(self.dev)

    def _new(self, *shape, fill=float("nan")):
        return torch.full(shape, fill, dtype=torch.float32, device=self.dev)

    def accumulators(self, seeded):
        return torch.as_tensor(self.fr["acc_seed"]).to(self.dev) if seeded else torch.zeros((self.N, 16), device=self.dev)

    def forward(self, stage, Cn=3):
        """The stage's forward outputs, as a tuple of tensors."""
        p = _host.ptr
        if stage == "features":
            F = torch.as_tensor(np.ascontiguousarray(self.fr["features"][:, :Cn])).to(self.dev)
            out = self._new(self.H, self.W, Cn)
            _lib.check(self.L.gsr_features_forward(C.byref(self.frame), Cn, p(F), p(out), self.stream))
            return (out,)
        if stage == "distortion":
            dist, mom = self._new(self.H, self.W), self._new(self.H, self.W, 4)
            _lib.check(self.L.gsr_distortion_forward(C.byref(self.dframe), p(dist), p(mom), self.stream))
            return dist, mom
        if stage == "plane_depth":
            out = self._new(self.H, self.W)
            _lib.check(self.L.gsr_plane_depth_forward(C.byref(self.dframe), p(self.slopes), p(out), self.stream))
            return (out,)
        if stage in ("median_depth", "plane_median"):
            med, contrib = self._new(self.H, self.W), torch.full((self.H, self.W), -1, dtype=torch.int32, device=self.dev)
            if stage == "median_depth":
                _lib.check(self.L.gsr_median_depth_forward(C.byref(self.dframe), p(med), p(contrib), self.stream))
            else:
                _lib.check(self.L.gsr_pmed_forward(C.byref(self.dframe), p(self.slopes), p(med), p(contrib), self.stream))
            return med, contrib
        out = self._new(self.H, self.W, 3)
        _lib.check(self.L.gsr_normal_render_forward(C.byref(self.frame), p(self.normals), p(out), self.stream))
        return (out,)

    def backward(self, stage, Cn=3, seeded=False):
        """The stage's backward outputs (accumulators last where it has them), from its own forward's outputs and a seeded image gradient."""
        p = _host.ptr
        g = torch.as_tensor(np.ascontiguousarray(self.fr["g_image"][:, :, :Cn])).to(self.dev)
        if stage == "features":
            dF = self._new(self.N, Cn)
            _lib.check(self.L.gsr_features_backward(C.byref(self.frame), Cn, p(g), p(dF), self.stream))
            return (dF,)
        acc = self.accumulators(seeded)
        if stage == "distortion":
            _, mom = self.forward(stage)
            g1 = g[:, :, 0].contiguous()
            _lib.check(self.L.gsr_distortion_backward(C.byref(self.dframe), p(g1), p(mom), p(acc), self.stream))
            return (acc,)
        if stage in DEPTH_STAGES:   # the medians are fed their own forward's contributor image; the moments start from zeros
            g1, mom = g[:, :, 0].contiguous(), torch.zeros((self.N, 3), device=self.dev)
            if stage == "plane_depth":
                (img,) = self.forward(stage)
                _lib.check(self.L.gsr_plane_depth_backward(C.byref(self.dframe), p(self.slopes), p(g1), p(img), p(acc), p(mom), self.stream))
                return mom, acc
            _, contrib = self.forward(stage)
            if stage == "median_depth":
                _lib.check(self.L.gsr_median_depth_backward(C.byref(self.dframe), p(g1), p(contrib), p(acc), self.stream))
                return (acc,)
            _lib.check(self.L.gsr_pmed_backward(C.byref(self.dframe), p(self.slopes), p(g1), p(contrib), p(mom), self.stream))
            return (mom,)
        (img,) = self.forward(stage)
        g3, dn = g[:, :, :3].contiguous(), self._new(self.N, 3)
        _lib.check(self.L.gsr_normal_render_backward(C.byref(self.frame), p(self.normals), p(g3), p(img), p(acc), p(dn), self.stream))
        return dn, acc
