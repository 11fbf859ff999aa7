"""
Adaptive density control: the trainer's `densification_and_pruning`
(reference train.py:351-713) over the HIP row movers of csrc/densify.hip.

`GaussianModel` carries what the reference keeps on its trainer object -- `params`, `grads`, `adam_m`,
`adam_v`, `num_points`, `scene_extent`, `config` (train.py:119-173) -- and `densification_and_pruning(it)` is the
same sequence: clone -> split (+ removal of the split originals) -> opacity prune -> opacity reset, with the
optimizer state re-created as zeros after every change of the point count (train.py:470-475).  Behaviours of the
reference that this keeps, because a drop-in must:

* every count is the LAST ENTRY of an exclusive scan (`int(prefix_sum.numpy()[-1])`, train.py:433/497/581/641), so the
  last row's own flag is never counted: a flagged last row is not cloned / split, and a compaction keeps one row
  fewer than the mask says whenever the last row is valid (the reference writes that row past the end of its
  output array; here it is dropped);
* the split pass runs over the post-clone arrays but the gradient norms were taken before the clone
  (train.py:408 vs 478-494): rows added by the clone have no gradient (the reference reads past `avg_grads`
  there; here the norm is 0, so a fresh clone is never split in the same call);
* position noise comes from Warp's stateless `randf(uint32)` hash, seeded by the row index (optimizer.py:297-299,
  353-355), so the same call always yields the same offsets.

`densify_statistic="screen"` (config key; include/gsr_densify_stats.h) replaces what is tested, not the sequence: the model owns
a `DensifyStats` -- per Gaussian, the norm of the screen-space mean gradient summed over the views that saw it, their count and
its largest screen radius, fed by `DensifyStats.update` after every backward -- and marks from the average, prunes also by
screen radius and world size, and starts a zeroed set after every density-control call that ran.  "reference" (the default) is
the code path above, untouched.
"""
import ctypes as C

import numpy as np
import torch

from . import _args, _host, _lib
from .optimizer import GROUPS

_WIDTH = {"positions": 3, "scales": 3, "rotations": 4, "opacities": 1, "shs": 48}


def _params_struct(params, n):
    for k in GROUPS:
        if not _args.is_packed(params[k], n * _WIDTH[k]):
            raise ValueError(f"densify: '{k}' must be a contiguous float32 device tensor with {n * _WIDTH[k]} elements")
    return _lib.GsrParams(n, *[_host.ptr(params[k]) for k in GROUPS])


def alloc_params(n, dev):
    """Zeroed parameter arrays in the trainer's shapes (train.py:446-452)."""
    return {"positions": torch.zeros(n, 3, dtype=torch.float32, device=dev), "scales": torch.zeros(n, 3, dtype=torch.float32, device=dev),
            "rotations": torch.zeros(n, 4, dtype=torch.float32, device=dev), "opacities": torch.zeros(n, dtype=torch.float32, device=dev),
            "shs": torch.zeros(n * 16, 3, dtype=torch.float32, device=dev)}


def _num_points(params):
    return int(params["opacities"].numel())


# ---- one wrapper per reference kernel -----------------------------------------------------------------------------
def mark_candidates(params, pos_grad, grad_threshold, scene_extent, percent_dense, split):
    """mark_clone_candidates / mark_split_candidates (optimizer.py:180-239) with compute_grad_norms (train.py:398-406)
    folded in.  `pos_grad` may have fewer rows than `params` (rows past it have norm 0)."""
    n = _num_points(params)
    dev = params["positions"].device
    p = _params_struct(params, n)
    n_grad = 0 if pos_grad is None else int(pos_grad.numel() // 3)
    if n_grad and not _args.is_packed(pos_grad):
        raise ValueError("densify: pos_grad must be a contiguous float32 device tensor")
    mask = torch.empty(n, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_densify_mark(C.byref(p), _host.ptr(pos_grad) if n_grad else None, min(n_grad, n), float(grad_threshold),
                                               float(scene_extent), float(percent_dense), _lib.MARK_SPLIT if split else _lib.MARK_CLONE,
                                               _host.ptr(mask), _host.stream_ptr(dev)))
    return mask


def prune_mask(params, opacity_threshold):
    """prune_gaussians (optimizer.py:367-385): 1 = keep."""
    n = _num_points(params)
    dev = params["positions"].device
    p = _params_struct(params, n)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_prune_mark(C.byref(p), float(opacity_threshold), _host.ptr(valid), _host.stream_ptr(dev)))
    return valid


def split_removal_mask(split_mask, n_total):
    """mark_split_originals_for_removal + invert_mask (train.py:547-576): 1 = keep."""
    dev = split_mask.device
    valid = torch.empty(n_total, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_split_removal_mask(n_total, int(split_mask.numel()), _host.ptr(split_mask), _host.ptr(valid),
                                                     _host.stream_ptr(dev)))
    return valid


def exclusive_scan(mask):
    """wp.utils.array_scan(mask, out, inclusive=False) and the count the reference reads from it (its last entry)."""
    n = int(mask.numel())
    dev = mask.device
    L = _lib.lib()
    prefix = torch.empty(n, dtype=torch.int32, device=dev)
    nbytes = int(L.gsr_mask_scan_workspace_bytes(n))
    scratch = _host.workspace("mask_scan", nbytes, dev)
    count = C.c_int32(0)
    with _host.on_device(dev):
        _lib.check(L.gsr_mask_scan(n, _host.ptr(mask), _host.ptr(prefix), C.byref(count), _host.ptr(scratch), nbytes, _host.stream_ptr(dev)))
    return prefix, int(count.value)


def clone_gaussians(params, mask, prefix, total, noise_scale=0.01):
    """clone_gaussians (optimizer.py:312-365) into freshly allocated arrays of N + total rows."""
    n = _num_points(params)
    dev = params["positions"].device
    out = alloc_params(n + total, dev)
    pin, pout = _params_struct(params, n), _params_struct(out, n + total)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_clone_gaussians(C.byref(pin), _host.ptr(mask), _host.ptr(prefix), float(noise_scale), C.byref(pout),
                                                  _host.stream_ptr(dev)))
    return out


def split_gaussians(params, mask, prefix, total, n_split=2, scale_factor=0.8):
    """split_gaussians (optimizer.py:242-309) into freshly allocated arrays of N + total*n_split rows."""
    n = _num_points(params)
    dev = params["positions"].device
    out = alloc_params(n + total * n_split, dev)
    pin, pout = _params_struct(params, n), _params_struct(out, n + total * n_split)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_split_gaussians(C.byref(pin), _host.ptr(mask), _host.ptr(prefix), int(n_split), float(scale_factor),
                                                  C.byref(pout), _host.stream_ptr(dev)))
    return out


def compact_gaussians(params, valid, prefix, count):
    """compact_gaussians (optimizer.py:387-416) into freshly allocated arrays of `count` rows."""
    n = _num_points(params)
    dev = params["positions"].device
    out = alloc_params(count, dev)
    pin, pout = _params_struct(params, n), _params_struct(out, count)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_compact_gaussians(C.byref(pin), _host.ptr(valid), _host.ptr(prefix), C.byref(pout), _host.stream_ptr(dev)))
    return out


def reset_opacities(opacities, max_opacity=0.01):
    """reset_opacities (optimizer.py:141-156), in place."""
    dev = opacities.device
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_reset_opacities(int(opacities.numel()), float(max_opacity), _host.ptr(opacities), _host.stream_ptr(dev)))
    _host.written_in_place(opacities)


class DensifyStats:
    """The three statistics arrays of include/gsr_densify_stats.h for `n` Gaussians: `grad_accum` (float32), `vis_count` and
    `max_radii` (int32), zeroed.

        out = backward(..., absgrad=True)
        stats.update(radii, out, use_abs=True)      # on the backward's stream, after it

    `update` uses device atomics, so views rendered on different streams (dist.ViewStreams) may update one set concurrently.  A
    capacity-mode frame that overflowed must not be counted: check the overflow first (forward.py), as for every use of such a
    frame.  Several ranks: dist.reduce_densify_stats once per density-control call."""

    def __init__(self, n, device):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.n, self.device = int(n), dev
        self.grad_accum = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.vis_count = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.max_radii = torch.zeros(self.n, dtype=torch.int32, device=dev)

    def struct(self):
        return _lib.GsrDensifyStats(self.n, _host.ptr(self.grad_accum), _host.ptr(self.vis_count), _host.ptr(self.max_radii))

    def reset(self):
        self.grad_accum.zero_()
        self.vis_count.zero_()
        self.max_radii.zero_()

    def update(self, radii, backward_out, use_abs=False):
        """Add one view: `radii` is the forward's (N,) int32 radii, `backward_out` the dict backward() returned for that view.
        The accumulators are reached through the tag backward() put on its `dL_dmean2D`; a workspace written since is refused."""
        tag = getattr(backward_out.get("dL_dmean2D"), "_gsr_backward_ws", None)
        if tag is None:
            raise ValueError("DensifyStats.update needs the dict backward() returned (its dL_dmean2D carries the workspace)")
        ws, ver, has_abs, n = tag
        if use_abs and not has_abs:
            raise ValueError("use_abs=True needs a backward(..., absgrad=True) result: the absolute columns of this one are zero")
        if ws._version != ver:
            raise ValueError("the backward workspace was written after backward() returned: its accumulators are not that call's")
        if n != self.n:
            raise ValueError(f"DensifyStats holds {self.n} Gaussians, the backward had {n}")
        dev = self.device
        if not (isinstance(radii, torch.Tensor) and radii.dtype == torch.int32 and radii.device == dev and radii.is_contiguous()
                and radii.numel() == n and radii.data_ptr() % 16 == 0):
            radii = _host.to_dev(radii, torch.int32, dev, (-1,))
            if radii.numel() != n:
                raise ValueError(f"radii has {radii.numel()} entries, the statistics {n}")
        st = self.struct()
        with _host.on_device(dev):
            _lib.check(_lib.lib().gsr_densify_stats_update(C.byref(st), _host.ptr(radii), _host.ptr(ws), ws.numel(), 1 if use_abs else 0,
                                                           _host.stream_ptr(dev)))


def mark_candidates_stats(params, stats, grad_threshold, scene_extent, percent_dense, split):
    """gsr_densify_mark_stats: mark_candidates' rule on grad_accum / max(vis_count, 1).  `stats` may hold fewer rows than `params`
    (rows a clone added since have average 0)."""
    n = _num_points(params)
    dev = params["positions"].device
    p, st = _params_struct(params, n), stats.struct()
    mask = torch.empty(n, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_densify_mark_stats(C.byref(p), C.byref(st), float(grad_threshold), float(scene_extent), float(percent_dense),
                                                     _lib.MARK_SPLIT if split else _lib.MARK_CLONE, _host.ptr(mask), _host.stream_ptr(dev)))
    return mask


def prune_mask_stats(params, stats, opacity_threshold, max_screen_radius=0.0, max_world_scale=0.0):
    """gsr_prune_mark_stats: 1 = keep.  A size term <= 0 is off."""
    n = _num_points(params)
    dev = params["positions"].device
    p, st = _params_struct(params, n), stats.struct()
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_prune_mark_stats(C.byref(p), C.byref(st), float(opacity_threshold), float(max_screen_radius),
                                                   float(max_world_scale), _host.ptr(valid), _host.stream_ptr(dev)))
    return valid


def init_gaussian_params(num_points, init_scale=0.1, device="cuda"):
    """The trainer's initial point set (train.py:37-92, 193-214): seeded by the row index alone, so every rank and every run
    starts from the same Gaussians."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    out = alloc_params(int(num_points), dev)
    p = _params_struct(out, int(num_points))
    with _host.on_device(dev):
        _lib.check(_lib.lib().gsr_init_gaussians(C.byref(p), float(init_scale), _host.stream_ptr(dev)))
    return out


def calculate_scene_extent(camera_centers, camera_extent_factor=1.0):
    """Radius of the camera positions around their centroid, at least 1 (train.py:233-257)."""
    c = np.asarray(camera_centers)
    if c.size == 0:
        return 1.0
    c = c.reshape(-1, 3)
    centre = np.mean(c, axis=0)
    radius = 0.0
    for pos in c:
        radius = max(radius, float(np.linalg.norm(pos - centre)))
    return max(radius * camera_extent_factor, 1.0)


class GaussianModel:
    """The part of NeRFGaussianSplattingTrainer (train.py:119-173) that densification touches."""

    def __init__(self, params, config=None, scene_extent=1.0):
        self.params = params
        self.num_points = _num_points(params)
        self.config = {"background_color": [0.0, 0.0, 0.0]}
        self.config.update(config or {})
        self.scene_extent = float(scene_extent)
        self.grads = self.create_gradient_arrays()
        self.adam_m = self.create_gradient_arrays()
        self.adam_v = self.create_gradient_arrays()
        self.densify_statistic = self.config.get("densify_statistic", "reference")
        if self.densify_statistic not in ("reference", "screen"):
            raise ValueError("densify_statistic must be 'reference' or 'screen'")
        self.stats = DensifyStats(self.num_points, params["positions"].device) if self.densify_statistic == "screen" else None

    def create_gradient_arrays(self):
        """train.py:216-231"""
        return alloc_params(self.num_points, self.params["positions"].device)

    def _replace(self, params):
        """train.py:470-475: new arrays in, gradients and both Adam moments back to zero."""
        self.params = params
        self.num_points = _num_points(params)
        self.grads = self.create_gradient_arrays()
        self.adam_m = self.create_gradient_arrays()
        self.adam_v = self.create_gradient_arrays()

    def densification_and_pruning(self, iteration):
        """train.py:351-713.  Returns a dict of what happened (the reference prints it)."""
        cfg = self.config
        densify_from_iter = cfg.get("densify_from_iter", 500)
        densify_until_iter = cfg.get("densify_until_iter", 15000)
        densification_interval = cfg.get("densification_interval", 100)
        opacity_reset_interval = cfg.get("opacity_reset_interval", 3000)
        log = {"cloned": 0, "split": 0, "split_removed": 0, "pruned": 0, "prune_skipped": False, "opacity_reset": False}

        if self.densify_statistic == "screen":
            return self._densification_and_pruning_screen(iteration, log)

        if iteration > densify_from_iter and iteration < densify_until_iter and iteration % densification_interval == 0:
            pos_grads = self.grads["positions"]          # the norms of train.py:408 are taken from this snapshot
            grad_threshold = cfg.get("densify_grad_threshold", 0.0002)
            percent_dense = cfg.get("percent_dense", 0.01)

            # --- step 1: clone small Gaussians with high gradients (train.py:414-475)
            clone_mask = mark_candidates(self.params, pos_grads, grad_threshold, self.scene_extent, percent_dense, split=False)
            clone_prefix, total_to_clone = exclusive_scan(clone_mask)
            if total_to_clone > 0:
                self._replace(clone_gaussians(self.params, clone_mask, clone_prefix, total_to_clone, 0.01))
                log["cloned"] = total_to_clone

            # --- step 2: split large Gaussians with high gradients (train.py:477-626)
            split_mask = mark_candidates(self.params, pos_grads, grad_threshold, self.scene_extent, percent_dense, split=True)
            split_prefix, total_to_split = exclusive_scan(split_mask)
            if total_to_split > 0:
                self._replace(split_gaussians(self.params, split_mask, split_prefix, total_to_split, 2, 0.8))
                log["split"] = total_to_split
                valid = split_removal_mask(split_mask, self.num_points)
                prefix, valid_count = exclusive_scan(valid)
                if valid_count < self.num_points:
                    log["split_removed"] = self.num_points - valid_count
                    self._replace(compact_gaussians(self.params, valid, prefix, valid_count))

            # --- step 3: opacity pruning (train.py:628-692)
            valid = prune_mask(self.params, cfg.get("cull_opacity_threshold", 0.005))
            prefix, valid_count = exclusive_scan(valid)
            min_valid_points = cfg.get("min_valid_points", 1000)
            max_valid_points = cfg.get("max_valid_points", 1000000)
            max_prune_ratio = cfg.get("max_allowed_prune_ratio", 0.5)
            prune_count = self.num_points - valid_count
            prune_ratio = prune_count / self.num_points if self.num_points > 0 else 0
            if (valid_count >= min_valid_points and valid_count <= max_valid_points and prune_ratio <= max_prune_ratio
                    and valid_count < self.num_points):
                log["pruned"] = prune_count
                self._replace(compact_gaussians(self.params, valid, prefix, valid_count))
            else:
                log["prune_skipped"] = True

        # --- opacity reset (train.py:695-713)
        background_is_white = all(c == 1.0 for c in cfg["background_color"])
        if iteration % opacity_reset_interval == 0 or (background_is_white and iteration == densify_from_iter):
            reset_opacities(self.params["opacities"], 0.01)
            log["opacity_reset"] = True
        return log

    def _densification_and_pruning_screen(self, iteration, log):
        """The same sequence on the screen-space statistics (include/gsr_densify_stats.h).  Clone and split masks both come from
        the statistics as they stood on entry -- rows the clone adds lie past them, have average 0 and are never split in the same
        call, the reference path's "snapshot before the clone" rule.  The prune adds the two size terms once iteration >
        opacity_reset_interval (the usual rule: before the first reset the radii are those of the initial blobs).  A call that ran
        ends with a zeroed statistics set of the new size."""
        cfg = self.config
        densify_from_iter = cfg.get("densify_from_iter", 500)
        densify_until_iter = cfg.get("densify_until_iter", 15000)
        densification_interval = cfg.get("densification_interval", 100)
        opacity_reset_interval = cfg.get("opacity_reset_interval", 3000)
        if iteration > densify_from_iter and iteration < densify_until_iter and iteration % densification_interval == 0:
            stats = self.stats
            if stats.n != self.num_points:
                raise ValueError(f"the statistics hold {stats.n} Gaussians, the model {self.num_points}")
            grad_threshold = cfg.get("densify_grad_threshold", 0.0002)
            percent_dense = cfg.get("percent_dense", 0.01)

            clone_mask = mark_candidates_stats(self.params, stats, grad_threshold, self.scene_extent, percent_dense, split=False)
            clone_prefix, total_to_clone = exclusive_scan(clone_mask)
            if total_to_clone > 0:
                self._replace(clone_gaussians(self.params, clone_mask, clone_prefix, total_to_clone, 0.01))
                log["cloned"] = total_to_clone

            split_mask = mark_candidates_stats(self.params, stats, grad_threshold, self.scene_extent, percent_dense, split=True)
            split_prefix, total_to_split = exclusive_scan(split_mask)
            prune_stats = stats
            if total_to_split > 0:
                self._replace(split_gaussians(self.params, split_mask, split_prefix, total_to_split, 2, 0.8))
                log["split"] = total_to_split
                valid = split_removal_mask(split_mask, self.num_points)
                prefix, valid_count = exclusive_scan(valid)
                if valid_count < self.num_points:
                    log["split_removed"] = self.num_points - valid_count
                    # the compaction moves rows: the prune's screen-radius term follows them (index bookkeeping once per call;
                    # rows added by the clone and the split have radius 0, and the last valid row is dropped as the compaction drops it)
                    radii = torch.zeros(self.num_points, dtype=torch.int32, device=stats.device)
                    radii[:stats.n] = stats.max_radii
                    prune_stats = DensifyStats(valid_count, stats.device)
                    prune_stats.max_radii = radii[valid == 1][:valid_count].contiguous()
                    self._replace(compact_gaussians(self.params, valid, prefix, valid_count))

            size_terms = iteration > opacity_reset_interval
            max_screen = float(cfg.get("prune_screen_size", 0.0)) if size_terms else 0.0
            max_world = float(cfg.get("prune_world_size", 0.0)) * self.scene_extent if size_terms else 0.0
            valid = prune_mask_stats(self.params, prune_stats, cfg.get("cull_opacity_threshold", 0.005), max_screen, max_world)
            prefix, valid_count = exclusive_scan(valid)
            min_valid_points = cfg.get("min_valid_points", 1000)
            max_valid_points = cfg.get("max_valid_points", 1000000)
            max_prune_ratio = cfg.get("max_allowed_prune_ratio", 0.5)
            prune_count = self.num_points - valid_count
            prune_ratio = prune_count / self.num_points if self.num_points > 0 else 0
            if (valid_count >= min_valid_points and valid_count <= max_valid_points and prune_ratio <= max_prune_ratio
                    and valid_count < self.num_points):
                log["pruned"] = prune_count
                self._replace(compact_gaussians(self.params, valid, prefix, valid_count))
            else:
                log["prune_skipped"] = True
            self.stats = DensifyStats(self.num_points, stats.device)

        background_is_white = all(c == 1.0 for c in cfg["background_color"])
        if iteration % opacity_reset_interval == 0 or (background_is_white and iteration == densify_from_iter):
            reset_opacities(self.params["opacities"], 0.01)
            log["opacity_reset"] = True
        return log
