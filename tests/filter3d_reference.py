"""
A float64 statement of the 3D smoothing filter (include/gsr_filter3d.h), written from its definition and from Mip-Splatting's
published formulae, not from the kernel.  Test helper like tests/antialias_reference.py, not a test file.  It also holds the case
matrix that tests/test_filter3d_reference.py (CPU) and tests/test_gpu_filter3d.py share.

Sampling rate: with p_view = (p, 1) @ view (row vectors), view v sees Gaussian i when
    p_view.z > 0.2      |p_view.x / p_view.z * focal| <= 1.15 W / 2      |p_view.y / p_view.z * focal| <= 1.15 H / 2
nu_i = max over seeing views of focal_v / z_v; an unseen Gaussian takes the smallest seen nu; nothing seen: filter 0;
filter_3d = sqrt(variance) / nu.  nu and filter_3d come from explicit loops over the views.

The map is plain tensor code: s' = sqrt(s^2 + f^2), opacity' = opacity * prod_k |s_k| / s'_k, f == 0 a pass-through.  Its transpose
comes from AUTOGRAD through the map; transpose_closed is the header's closed form, which the CPU test holds against autograd.

Inputs are the float32 values the kernels read, widened: positions, view matrices, focal lengths (rounded by the c_float store) and
the variance.
"""
import json
import os

import numpy as np
import torch

D = torch.float64
NEAR = 0.2
MARGIN = 0.15
EPS32 = float(np.finfo(np.float32).eps)
HERE = os.path.dirname(os.path.abspath(__file__))


def view_records(cams):
    """[(view (4, 4) float64, focal, W, H)] from camera dicts (cameras.nerf_camera) or (viewmatrix, focal, W, H) tuples, every
    float rounded to float32 first: what GsrFilterView holds."""
    out = []
    for c in cams:
        if isinstance(c, dict):
            view, focal, W, H = c["world_to_camera"], c["width"] / (2.0 * float(c["tan_fovx"])), c["width"], c["height"]
        else:
            view, focal, W, H = c
        v32 = np.asarray(view, np.float64).reshape(-1)[:16].astype(np.float32).reshape(4, 4)
        out.append((torch.as_tensor(v32.astype(np.float64)), float(np.float32(focal)), int(W), int(H)))
    return out


def sampling_f64(means, cams, variance=0.2):
    """dict: `seen` (V, N) bool, `nu_view` (V, N) focal / z, `margins` (V, N, 3) the relative distance of each of the three visibility
    tests from its threshold, `z_cond` (V, N) the conditioning (|p_x v02| + |p_y v12| + |p_z v22| + |v32|) / |z| of the one
    cancellation, `nu` (N,) (0 where no view sees the Gaussian), `argmax` (N,) the view that gave it, `any_seen` (N,) and `filter_3d`
    (N,), all float64 / numpy."""
    P = torch.as_tensor(np.asarray(means, np.float32).reshape(-1, 3).astype(np.float64))
    N = P.shape[0]
    views = view_records(cams)
    V = len(views)
    seen = np.zeros((V, N), bool)
    nu_view, margins, z_cond = np.zeros((V, N)), np.zeros((V, N, 3)), np.zeros((V, N))
    for v, (M, focal, W, H) in enumerate(views):
        pv = torch.cat([P, torch.ones(N, 1, dtype=D)], 1) @ M
        x, y, z = pv[:, 0], pv[:, 1], pv[:, 2]
        zs = torch.where(z.abs() > 0, z, torch.ones_like(z))
        ax, ay = (x / zs * focal).abs(), (y / zs * focal).abs()
        lim_x, lim_y = (1.0 + MARGIN) * W / 2.0, (1.0 + MARGIN) * H / 2.0
        seen[v] = ((z > NEAR) & (ax <= lim_x) & (ay <= lim_y)).numpy()
        margins[v] = torch.stack([(z - NEAR).abs() / NEAR, (ax - lim_x).abs() / lim_x, (ay - lim_y).abs() / lim_y], 1).numpy()
        nu_view[v] = (focal / zs).numpy()
        z_cond[v] = (((P[:, 0] * M[0, 2]).abs() + (P[:, 1] * M[1, 2]).abs() + (P[:, 2] * M[2, 2]).abs() + M[3, 2].abs()) / zs.abs()).numpy()
    nu, argmax = np.zeros(N), np.full(N, -1)
    for i in range(N):
        for v in range(V):
            if seen[v, i] and nu_view[v, i] > nu[i]:
                nu[i], argmax[i] = nu_view[v, i], v
    any_seen = nu > 0
    var = float(np.float32(variance))
    filt = np.zeros(N)
    if any_seen.any():
        filt = np.sqrt(var) / np.where(any_seen, nu, nu[any_seen].min())
    return {"seen": seen, "nu_view": nu_view, "margins": margins, "z_cond": z_cond, "nu": nu, "argmax": argmax, "any_seen": any_seen,
            "filter_3d": filt}


def near_threshold(sampling, rel=1e-4):
    """(V, N): Gaussian/view pairs one of whose visibility tests sits within `rel` (relative) of its threshold."""
    return (sampling["margins"] <= rel).any(2)


def apply_f64(scales, opacity, filt):
    """(s', opacity') as float64 tensors; differentiable in `scales` and `opacity` when they are tensors that require grad."""
    s = scales if isinstance(scales, torch.Tensor) else torch.as_tensor(np.asarray(scales, np.float32).reshape(-1, 3).astype(np.float64))
    o = opacity if isinstance(opacity, torch.Tensor) else torch.as_tensor(np.asarray(opacity, np.float32).reshape(-1).astype(np.float64))
    f = torch.as_tensor(np.asarray(filt, np.float64).reshape(-1))
    on = (f != 0)[:, None]
    sp = torch.sqrt(s * s + (f * f)[:, None])
    r = s.abs() / torch.where(on, sp, torch.ones_like(sp))
    sp = torch.where(on, sp, s)
    coef = torch.where(on[:, 0], r.prod(1), torch.ones_like(f))
    return sp, o * coef


def transpose_autograd(scales, opacity, filt, g_s, g_o):
    """dL/d(scales, opacity) from the cotangents (g_s (N, 3), g_o (N,)) of (s', opacity'): autograd through apply_f64."""
    s = torch.as_tensor(np.asarray(scales, np.float32).reshape(-1, 3).astype(np.float64)).requires_grad_(True)
    o = torch.as_tensor(np.asarray(opacity, np.float32).reshape(-1).astype(np.float64)).requires_grad_(True)
    sp, op = apply_f64(s, o, filt)
    L = (sp * torch.as_tensor(np.asarray(g_s, np.float64).reshape(-1, 3))).sum() + (op * torch.as_tensor(np.asarray(g_o, np.float64).reshape(-1))).sum()
    ds, do = torch.autograd.grad(L, (s, o))
    return ds.numpy(), do.numpy()


def transpose_closed(scales, opacity, filt, g_s, g_o):
    """The header's closed form, and the sum of the magnitudes of its two scale terms (the scale of the float32 error model):
    (dL_dscale, dL_dopacity, |g_s' s / s'| + |g_o' opacity d(coef)/ds|)."""
    s = np.asarray(scales, np.float32).reshape(-1, 3).astype(np.float64)
    o = np.asarray(opacity, np.float32).reshape(-1).astype(np.float64)
    f = np.asarray(filt, np.float64).reshape(-1)
    g_s, g_o = np.asarray(g_s, np.float64).reshape(-1, 3), np.asarray(g_o, np.float64).reshape(-1)
    on = f != 0
    sp = np.sqrt(s * s + (f * f)[:, None])
    sp_safe = np.where(on[:, None], sp, 1.0)
    r = np.abs(s) / sp_safe
    others = np.stack([r[:, 1] * r[:, 2], r[:, 0] * r[:, 2], r[:, 0] * r[:, 1]], 1)
    t1 = g_s * s / sp_safe
    t2 = (g_o * o)[:, None] * np.sign(s) * others * (f * f)[:, None] / sp_safe ** 3
    ds = np.where(on[:, None], t1 + t2, g_s)
    do = np.where(on, g_o * r.prod(1), g_o)
    return ds, do, np.where(on[:, None], np.abs(t1) + np.abs(t2), np.abs(g_s))


def mip_splatting_compute_3d_filter(xyz, cams, screen_margin=0.15):
    """A literal transcription of Mip-Splatting's GaussianModel.compute_3D_filter (float64, its own statements and order): R and T
    of each camera, the pixel coordinates about the image CORNER, the screen test, the smallest z, the largest focal length.
    `screen_margin` is its literal 0.15 of the full image size on each side, i.e. |x - W/2| <= 0.65 W = 1.3 W/2;
    screen_margin = 0.075 is the test of gsr_filter3d.h, |x - W/2| <= 1.15 W/2."""
    xyz = torch.as_tensor(np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64))
    distance = torch.ones(xyz.shape[0], dtype=D) * 100000.0
    valid_points = torch.zeros(xyz.shape[0], dtype=torch.bool)
    focal_length = 0.0
    for M, focal, W, H in view_records(cams):
        R, T = M[:3, :3], M[3, :3]
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * focal + W / 2.0
        y = y / z * focal + H / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -screen_margin * W, x <= W * (1.0 + screen_margin)),
                                      torch.logical_and(y >= -screen_margin * H, y <= (1.0 + screen_margin) * H))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < focal:
            focal_length = focal
    if not valid_points.any():
        return np.zeros(xyz.shape[0])
    distance[~valid_points] = distance[valid_points].max()
    return (distance / focal_length * (float(np.float32(0.2)) ** 0.5)).numpy()


# ---- the case matrix ----
NS = (1, 63, 64, 65, 255, 256, 257, 3000)
VS = (1, 3, 8)
EXTENT = 6.0          # the cameras orbit at distance 4: positions in (-6, 6)^3 lie behind them, outside their margins and in front
MAX_EXCLUDED = 0.01   # at most this share of a case's Gaussians may have a pair within 1e-4 of a threshold


def lego_cameras(cameras_mod, V, sizes=((96, 72),), angle_scale=(1.0,)):
    """The first V poses of tests/golden/lego_train_poses.json; view k is sizes[k % len] pixels with the field of view scaled by
    angle_scale[k % len] (so the focal lengths differ when more than one is given)."""
    with open(os.path.join(HERE, "golden", "lego_train_poses.json")) as f:
        d = json.load(f)
    return [cameras_mod.nerf_camera(d["frames"][k]["transform_matrix"], sizes[k % len(sizes)][0], sizes[k % len(sizes)][1],
                                    d["camera_angle_x"] * angle_scale[k % len(angle_scale)]) for k in range(V)]


def make_case(scenes_mod, cameras_mod, name):
    """One case: {"name", "scene" (synthetic_scene arrays; scales log-uniform in [1e-4, 1]), "cams"}.  Names: "N-V" for the matrix,
    "mixed" (three focal lengths and image sizes, none above 64 x 48), "negative" (every tenth Gaussian has a negative scale)."""
    if name == "mixed":
        N, cams = 257, lego_cameras(cameras_mod, 8, sizes=((64, 48), (48, 48), (32, 24)), angle_scale=(1.0, 0.7, 1.4))
    elif name == "negative":
        N, cams = 257, lego_cameras(cameras_mod, 3)
    else:
        N, V = (int(x) for x in name.split("-"))
        cams = lego_cameras(cameras_mod, V)
    seed = 1000 + sum(ord(ch) * (k + 1) for k, ch in enumerate(name))
    sc = scenes_mod.synthetic_scene(N, 0.05, 0.6, seed, extent=EXTENT)
    rng = np.random.default_rng(seed + 1)
    sc["scales"] = np.exp(rng.uniform(np.log(1e-4), 0.0, (N, 3))).astype(np.float32)
    if name == "negative":
        sc["scales"][::10, 1] *= -1.0
    return {"name": name, "scene": sc, "cams": cams}


CASE_NAMES = tuple(f"{n}-{v}" for n in NS for v in VS) + ("mixed", "negative")
