"""
A float64 statement of the antialiased mode (include/gsr_antialias.h): the opacity compensation of the 0.3-pixel blur, forward
and backward.  Test helper like tests/f64_reference.py (whose building blocks it imports and does not edit), not a test file.

With h = 0.3, (a0, b, c0) the projected covariance before the blur and a = a0 + h, c = c0 + h after it,
    det0 = a0 c0 - b^2      det1 = a c - b^2      r = det0 / det1      rho = sqrt(max(0.000025, r))
and every Gaussian is blended with opacity * rho.  Nothing else of the forward changes.

The backward is f64_reference.backward_f64's three steps with two additions, both linear in their cotangents:
  (1) dL_dopacity is multiplied by the forward's rho;
  (2) the autograd VJP of rho(cov2d(mean, Sigma3D)) under the same switches as the conic's (q1_textbook_backward,
      frustum_clamp_grad), with cotangent opacity * g (g = dL/d(opacity * rho) from the blend), is added to the mean term and to
      dL_dcov3D (with the vec6_offdiag_param factor) before cov3d_backward_f64 runs.
The 1/(det^2 + 1e-7) of the conic inversion (denom_eps) is not applied to the rho term.

camera_gradient_aa_f64 extends tests/camera_grad_reference.py the same way: rho joins the per-Gaussian geometry whose camera
leaves autograd differentiates.
"""
from unittest import mock

import numpy as np
import torch

import camera_grad_reference as CR
import f64_reference as F

D = torch.float64
H_BLUR = 0.3
FLOOR = 0.000025


# The blend's alpha cap as the float32 kernels hold it.  It is the one constant of the blend whose float32 value a discrete test can
# tell from its float64 literal: behind two capped layers T = (1 - cap)^2, which for cap = 0.99 is 1e-4 exactly, so the stop test
# T < 1e-4 (forward.py:486-488) is a tie that float64 arithmetic on the literal 0.99 decides one way (1.0000000000000002e-4: go on)
# and the reference's float32 code, whose cap is float32(0.99) = 0.9900000095..., the other (9.99998e-5: stop; that layer and
# everything behind it are dropped, up to 0.01 |colour - background| per pixel).  Opacity * rho, or plain opacities of 0.999 under
# large splats, put whole regions of an image behind two capped layers.  With the cap widened from float32 like every other input
# the tie is gone (a margin of 2e-6, thirty float32 roundings); everything else is f64_reference's blend, statement for statement.
ALPHA_CAP = float(np.float32(0.99))


def _blend_tile(xy, conic, op, col, inv_depth, idx, px, py, bg, alpha_cap_grad):
    """f64_reference._blend_tile with ALPHA_CAP in place of the literal 0.99."""
    L = idx.numel()
    P = px.numel()
    if L == 0:
        return (bg[None, :].expand(P, 3).clone(), torch.zeros(P, dtype=D), torch.ones(P, dtype=D), torch.zeros(P, dtype=torch.int64))
    g = lambda a: a[idx]
    dx = g(xy)[None, :, 0] - px[:, None]
    dy = g(xy)[None, :, 1] - py[:, None]
    cg = g(conic)
    power = -0.5 * (cg[None, :, 0] * dx * dx + cg[None, :, 2] * dy * dy) - cg[None, :, 1] * dx * dy
    G = torch.exp(power)
    a_raw = g(op)[None, :] * G
    capped = a_raw > ALPHA_CAP
    at_cap = (a_raw - a_raw.detach() + ALPHA_CAP) if alpha_cap_grad else torch.full_like(a_raw, ALPHA_CAP)
    alpha = torch.where(capped, at_cap, a_raw)
    with torch.no_grad():
        keep = (power <= 0) & (alpha >= 1.0 / 255.0)
        om = torch.where(keep, 1.0 - alpha, torch.ones_like(alpha))
        T_in = torch.cumprod(torch.cat([torch.ones(P, 1, dtype=D), om[:, :-1]], 1), 1)
        stop = keep & (T_in * om < 1e-4)
        pos = torch.arange(L)[None, :].expand(P, L)
        first_stop = torch.where(stop, pos, torch.full_like(pos, L)).min(1).values
        active = keep & (pos < first_stop[:, None])
        n_contrib = torch.where(active, pos + 1, torch.zeros_like(pos)).max(1).values
    omv = torch.where(active, 1.0 - alpha, torch.ones_like(alpha))
    T_excl = torch.cumprod(torch.cat([torch.ones(P, 1, dtype=D), omv[:, :-1]], 1), 1)
    w = torch.where(active, alpha * T_excl, torch.zeros_like(alpha))
    T_final = torch.prod(omv, 1)
    rgb = w @ g(col) + T_final[:, None] * bg[None, :]
    inv_d = w @ g(inv_depth)
    return rgb, inv_d, T_final, n_contrib


def blend_f64(*args, **kwargs):
    """f64_reference.blend_f64 (its tile loop and its tile-by-tile differentiation, unchanged) over the tile function above."""
    with mock.patch.object(F, "_blend_tile", _blend_tile):
        return F.blend_f64(*args, **kwargs)


def rho_of(a0, b, c0):
    """(rho, r): the opacity scale and the determinant ratio it is the clamped square root of."""
    det0 = a0 * c0 - b * b
    det1 = (a0 + H_BLUR) * (c0 + H_BLUR) - b * b
    r = det0 / det1
    return torch.sqrt(torch.clamp(r, min=FLOOR)), r


def rho_grad_closed(a0, b, c0):
    """d rho / d(a, b, c) in the header's closed forms (b the one parameter that fills both off-diagonal entries): zero on the floor."""
    h = H_BLUR
    a, c = a0 + h, c0 + h
    det1 = a * c - b * b
    rho, r = rho_of(a0, b, c0)
    k = torch.where(r > FLOOR, 1.0 / (2.0 * rho * det1 * det1), torch.zeros_like(r))
    return k * h * (c * (c - h) + b * b), -k * 2.0 * b * h * (a + c - h), k * h * (a * (a - h) + b * b)


def _forward_cov2d(pre, scene, kw, scale_modifier):
    N = pre["N"]
    c6 = F.cov3d(F._t(scene["scales"], (N, 3)), F._t(scene["rotations"], (N, 4)), scale_modifier)
    return F.cov2d(pre["p_view"][:, :3], c6, pre["cam"], "forward")


def preprocess_aa_f64(scene, kw, degree, scale_modifier):
    """f64_reference.preprocess_f64 plus rho: `opacity` is the effective one (opacity * rho), `opacity_raw` the scene's, `rho` the
    scale (0 for culled Gaussians, as every per-Gaussian output), `rho_r` the ratio before the clamp and `rho_cond` =
    (a0 c0 + b^2) / |det0|, the conditioning of the one cancellation a float32 rho goes through."""
    pre = F.preprocess_f64(scene, kw, degree, scale_modifier)
    a0, b0, c0 = _forward_cov2d(pre, scene, kw, scale_modifier)
    rho, r = rho_of(a0, b0, c0)
    keep = torch.as_tensor(~pre["culled"]).to(D)
    pre = dict(pre)
    pre["opacity_raw"] = pre["opacity"]
    pre["rho"] = rho * keep
    pre["rho_r"] = r.detach().numpy()
    det0 = (a0 * c0 - b0 * b0).abs()
    pre["rho_cond"] = ((a0 * c0 + b0 * b0) / torch.where(det0 > 0, det0, torch.ones_like(det0))).detach().numpy()
    pre["opacity"] = pre["opacity_raw"] * pre["rho"]
    return pre


def render_aa_f64(scene, kw, point_list, ranges, pre=None):
    """(image, inverse depth, final_T, n_contrib) of the antialiased forward over given lists, float64 numpy."""
    if pre is None:
        pre = preprocess_aa_f64(scene, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    cam = pre["cam"]
    with torch.no_grad():
        out = blend_f64(pre["xy"], pre["conic"], pre["opacity"], pre["colour"], pre["depth"], point_list, ranges, cam.bg, cam.W, cam.H)
    return tuple(o.numpy() for o in out)


def rho_vjp_f64(scene, kw, visible, cotangent, switches=None, cov3D=None):
    """The VJP of (mean3D, Sigma3D (VEC6)) -> rho under the backward's conventions, with `cotangent` (N,) = opacity * g.  Returns
    (dL_dmean3D part, dL_dcov3D part) as float64 tensors, zero for Gaussians outside `visible`."""
    s = F._sw(switches)
    cam = F.Camera(kw)
    N = np.asarray(scene["means"]).reshape(-1, 3).shape[0]
    vf = torch.as_tensor(np.asarray(visible, dtype=bool)).to(D)
    means = F._t(scene["means"], (N, 3)).requires_grad_(True)
    if cov3D is None:
        c6 = F.cov3d(F._t(scene["scales"], (N, 3)), F._t(scene["rotations"], (N, 4)), float(kw["scale_modifier"]))
    else:
        c6 = torch.as_tensor(np.asarray(cov3D, np.float64)).reshape(N, 6)
    c6 = c6.detach().requires_grad_(True)
    t = (F._homog(means) @ cam.view)[:, :3]
    a0, b0, c0 = F.cov2d(t, c6, cam, "textbook" if s["q1_textbook_backward"] else "forward", true_clamp_grad=not s["frustum_clamp_grad"])
    rho, _ = rho_of(a0, b0, c0)
    cot = torch.as_tensor(np.asarray(cotangent, np.float64)).reshape(N) * vf
    g_mean, g_cov = torch.autograd.grad((rho * cot).sum(), (means, c6))
    if not s["vec6_offdiag_param"]:
        g_cov = g_cov * torch.tensor([1.0, 0.5, 0.5, 1.0, 0.5, 1.0], dtype=D)
    return g_mean.detach(), g_cov.detach()


def backward_aa_f64(scene, kw, point_list, ranges, dL_dpixels, switches=None, pre=None, cov3D=None):
    """The antialiased backward: the nine arrays of f64_reference.backward_f64 as float64 numpy, plus `_g_eff_opacity` (the blend
    stage's dL/d(opacity * rho)) and `_rho`."""
    s = F._sw(switches)
    if pre is None:
        pre = preprocess_aa_f64(scene, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    cam, N = pre["cam"], pre["N"]
    xy = pre["xy"].detach().clone().requires_grad_(True)
    con = pre["conic"].detach().clone().requires_grad_(True)
    op = pre["opacity"].detach().clone().requires_grad_(True)                  # the effective opacity
    col = pre["colour"].detach().clone().requires_grad_(True)
    *_, (gxy, gcon, gop, gcol) = blend_f64(xy, con, op, col, pre["depth"].detach(), point_list, ranges, cam.bg, cam.W, cam.H,
                                             alpha_cap_grad=s["alpha_cap_passes_grad"], dL_dpixels=dL_dpixels, wrt=(xy, con, op, col))
    dL_dmean2D = torch.zeros(N, 3, dtype=D)
    dL_dmean2D[:, 0] = gxy[:, 0] * (0.5 * cam.W)
    dL_dmean2D[:, 1] = gxy[:, 1] * (0.5 * cam.H)
    dL_dconic = torch.zeros(N, 4, dtype=D)
    dL_dconic[:, 0], dL_dconic[:, 3] = gcon[:, 0], gcon[:, 2]
    dL_dconic[:, 1] = gcon[:, 1] * (0.5 if s["conic_b_half"] else 1.0)
    visible = ~pre["culled"]
    m3, dshs, dcov6, _ = F.geometry_vjp_f64(scene, kw, int(kw["degree"]), visible, pre["clamped"], dL_dmean2D, dL_dconic, gcol, switches,
                                            cov3D=cov3D)
    r_mean, r_cov = rho_vjp_f64(scene, kw, visible, pre["opacity_raw"].detach() * gop, switches, cov3D=cov3D)
    m3, dcov6 = m3 + r_mean, dcov6 + r_cov
    dsc, drot = F.cov3d_backward_f64(scene, kw, visible, dcov6, switches)
    n = lambda x: x.detach().numpy()
    return {
        "dL_dmean3D": n(m3), "dL_dcolor": n(gcol), "dL_dshs": n(dshs), "dL_dopacity": n(gop * pre["rho"].detach()), "dL_dscale": n(dsc),
        "dL_drot": n(drot), "dL_dmean2D": n(dL_dmean2D), "dL_dconic": n(dL_dconic), "dL_dcov3D": np.zeros((N, 6)),
        "_dL_dcov3D_local": n(dcov6), "_g_eff_opacity": n(gop), "_rho": n(pre["rho"]),
    }


def near_floor(pre, rel=1e-3):
    """Gaussians whose ratio r sits within `rel` (relative) of the floor: rho has a kink there, so its gradient is left out of
    comparisons.  Visible ones only."""
    return (np.abs(pre["rho_r"] - FLOOR) <= rel * FLOOR) & ~pre["culled"]


# ---- the camera gradient (extends tests/camera_grad_reference.py) ----
def _rho_of_camera(sub, kw, cam, view, scale_modifier):
    """rho per Gaussian as a function of per-Gaussian view matrices (N, 4, 4): the forward's Sigma2D, as camera_grad_reference's
    geometry forms it."""
    N = int(np.asarray(sub["means"]).reshape(-1, 3).shape[0])
    Ph = F._homog(F._t(sub["means"], (N, 3)))
    t = torch.einsum("ni,nij->nj", Ph, view)[:, :3]
    c6 = F.cov3d(F._t(sub["scales"], (N, 3)), F._t(sub["rotations"], (N, 4)), scale_modifier)
    tx, ty, tz = F._frustum_t(t, cam, True)
    fx, fy = cam.W / (2.0 * cam.tanx), cam.H / (2.0 * cam.tany)
    J = torch.zeros(N, 2, 3, dtype=D)
    J[:, 0, 0] = fx / tz
    J[:, 0, 2] = -fx * tx / (tz * tz)
    J[:, 1, 1] = fy / tz
    J[:, 1, 2] = -fy * ty / (tz * tz)
    T = J @ view[:, :3, :3]
    S2 = T @ F.unvec6(c6) @ T.transpose(1, 2)
    return rho_of(S2[:, 0, 0], S2[:, 0, 1], S2[:, 1, 1])[0]


def camera_gradient_aa_f64(scene, kw, radii, point_list, ranges, dpix):
    """camera_grad_reference.camera_gradient_f64 for an antialiased frame: (grad (36,), scale (36,))."""
    cam = CR.Cam(kw)
    degree, sm = int(kw["degree"]), float(kw["scale_modifier"])
    sub, idx, N = CR._visible(scene, radii)
    n = int(idx.numel())
    if n == 0:
        return np.zeros(36), np.zeros(36)
    Vn0 = cam.view.expand(n, 4, 4)
    with torch.no_grad():
        geo = CR.geometry(sub, kw, cam, cam.view, cam.proj, cam.campos, degree, sm)
        rho = _rho_of_camera(sub, kw, cam, Vn0, sm)
    xy, con, col, invd = CR._scatter(N, idx, *geo)
    op_raw = F._t(sub["opacities"], (n,))
    op = CR._scatter(N, idx, op_raw * rho)[0]
    leaves = [x.detach().clone().requires_grad_(True) for x in (xy, con, op, col)]
    depth = torch.where(invd > 0, 1.0 / torch.where(invd > 0, invd, torch.ones_like(invd)), torch.zeros_like(invd))
    *_, (gxy, gcon, gop, gcol) = blend_f64(leaves[0], leaves[1], leaves[2], leaves[3], depth, point_list, ranges, cam.bg, cam.W, cam.H,
                                             dL_dpixels=dpix, wrt=tuple(leaves))
    gxy, gcon, gop, gcol = gxy[idx], gcon[idx], gop[idx], gcol[idx]
    Vn = cam.view.expand(n, 4, 4).clone().requires_grad_(True)
    Pn = cam.proj.expand(n, 4, 4).clone().requires_grad_(True)
    Cn = cam.campos.expand(n, 3).clone().requires_grad_(True)
    xy, con, col, invd = CR.geometry(sub, kw, cam, Vn, Pn, Cn, degree, sm)
    L = (xy * gxy).sum() + (con * gcon).sum() + (col * gcol).sum() + (_rho_of_camera(sub, kw, cam, Vn, sm) * (op_raw * gop)).sum()
    gV, gP, gC = torch.autograd.grad(L, (Vn, Pn, Cn), allow_unused=True)
    gV, gP, gC = [torch.zeros_like(x) if g is None else g for g, x in zip((gV, gP, gC), (Vn, Pn, Cn))]
    terms = torch.cat([gV.reshape(n, 16), gP.reshape(n, 16), gC, torch.zeros(n, 1, dtype=D)], 1)
    return terms.sum(0).numpy(), terms.abs().sum(0).numpy()
