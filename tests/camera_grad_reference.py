"""
A float64 statement of the camera gradient (include/gsr_camera_grads.h): autograd of blend o preprocess with the view matrix,
the full projection and the camera position as leaves.  Test helper like tests/f64_reference.py (whose pieces it reuses, without
changing it), not a test file.

f64_reference.Camera widens campos through numpy, so it cannot carry a leaf; `Cam` here is its own camera object.  Every
Gaussian gets its own copy of the three leaves (per-Gaussian (N, 4, 4), (N, 4, 4), (N, 3) tensors holding the same values): the
sum over Gaussians of their gradients is the gradient with respect to the shared camera, and the per-Gaussian terms give the
scale a float32 sum of those terms rounds against (sum |term|, not |sum|, which cancels).

The forward is this library's own (the true derivative is the target, not the reference backward's conventions): NDC from
p_hom.xy / (p_hom.w + 1e-7), Sigma2D = J W Sigma3D W^T J^T with the frustum clamp differentiated, the 0.3 blur and 1/det^2,
1/depth, and the colour through the normalised view direction.  Visibility, tile lists and the sort order are inputs (the
forward's own), as they are piecewise constant.  The blend stage is differentiated tile by tile and its cotangents chained into
the per-Gaussian geometry, as f64_reference.backward_f64 does.

camera_gradient_from_cotangents is that second stage alone, fed the blend-stage cotangents the kernels left in their
accumulator records (and the forward's colour-clamp state): it runs at millions of Gaussians, where the tile-by-tile blend
would not, and it isolates the camera kernels' own arithmetic from the blend backward's.  tests/test_camera_grad_split.py
checks that the two stages together are camera_gradient_f64.
"""
import numpy as np
import torch

import f64_reference as F

D = torch.float64


class Cam:
    """The float32 camera inputs of one render call, widened to float64; view / proj / campos may be replaced by leaves."""

    def __init__(self, kw):
        self.W, self.H = int(kw["image_width"]), int(kw["image_height"])
        self.view = F._t(kw["viewmatrix"], (4, 4))
        self.proj = F._t(kw["projmatrix"], (4, 4))
        self.campos = torch.as_tensor(np.asarray(kw["campos"], np.float32)[:3].astype(np.float64))
        self.tanx = float(np.float32(kw["tan_fovx"]))
        self.tany = float(np.float32(kw["tan_fovy"]))
        self.bg = F._t(np.asarray(kw["background"])[:3])


def geometry(scene, kw, cam, view, proj, campos, degree, scale_modifier):
    """Per-Gaussian blend inputs as functions of the camera: xy (pixels), conic (A, B, C), colour (clamped), 1/depth.  view and
    proj are (4, 4) or per-Gaussian (N, 4, 4), campos (3,) or (N, 3)."""
    xy, con, raw, invd = _geometry_raw(scene, kw, cam, view, proj, campos, degree, scale_modifier)
    colour = torch.where(raw < 0, torch.zeros_like(raw), raw)
    return xy, con, colour, invd


def _geometry_raw(scene, kw, cam, view, proj, campos, degree, scale_modifier):
    """geometry() with the colour before the clamp (SH + 0.5): the clamp is then the caller's, e.g. the forward's own."""
    N = int(np.asarray(scene["means"]).reshape(-1, 3).shape[0])
    means = F._t(scene["means"], (N, 3))
    Ph = F._homog(means)
    vw = view.expand(N, 4, 4) if view.dim() == 2 else view
    pj = proj.expand(N, 4, 4) if proj.dim() == 2 else proj
    t = torch.einsum("ni,nij->nj", Ph, vw)[:, :3]
    ph = torch.einsum("ni,nij->nj", Ph, pj)
    pw = 1.0 / (ph[:, 3] + 1e-7)
    ndc = ph[:, :2] * pw[:, None]
    xy = torch.stack([F._ndc2pix(ndc[:, 0], cam.W), F._ndc2pix(ndc[:, 1], cam.H)], 1)
    c6 = F.cov3d(F._t(scene["scales"], (N, 3)), F._t(scene["rotations"], (N, 4)), scale_modifier)
    tx, ty, tz = F._frustum_t(t, cam, True)
    fx, fy = cam.W / (2.0 * cam.tanx), cam.H / (2.0 * cam.tany)
    J = torch.zeros(N, 2, 3, dtype=D)
    J[:, 0, 0] = fx / tz
    J[:, 0, 2] = -fx * tx / (tz * tz)
    J[:, 1, 1] = fy / tz
    J[:, 1, 2] = -fy * ty / (tz * tz)
    T = J @ vw[:, :3, :3]
    S2 = T @ F.unvec6(c6) @ T.transpose(1, 2)
    con = F.conic_of(S2[:, 0, 0], S2[:, 0, 1], S2[:, 1, 1])[0]
    invd = 1.0 / tz
    cp = campos.expand(N, 3) if campos.dim() == 1 else campos
    d = means - cp
    l2 = (d * d).sum(1)
    ln = torch.sqrt(torch.where(l2 > 0, l2, torch.ones_like(l2)))
    dirs = torch.where((l2 > 0)[:, None], d / ln[:, None], torch.zeros_like(d))   # direction 0 (and no gradient) at campos
    raw = F.sh_colour(F._t(scene["shs"], (N, 16, 3)), dirs, degree)
    return xy, con, raw, invd


def blend_cotangents(xy, con, op, col, invd, point_list, ranges, cam, dpix=None, ddep=None, dalpha=None, alpha_cap_grad=True):
    """dL/d(xy, conic, colour, 1/depth) of L = sum dpix . image + sum ddep . inverse depth + sum dalpha . (1 - final_T)."""
    leaves = [x.detach().clone().requires_grad_(True) for x in (xy, con, col, invd)]
    grads = [torch.zeros_like(x) for x in leaves]
    pl = torch.as_tensor(np.asarray(point_list, dtype=np.int64))
    cot = lambda a, shape: None if a is None else torch.as_tensor(np.asarray(a, np.float64)).reshape(shape)
    gP, gD, gA = cot(dpix, (cam.H, cam.W, 3)), cot(ddep, (cam.H, cam.W)), cot(dalpha, (cam.H, cam.W))
    for s, e, yy, xx in F._tiles(cam.W, cam.H, ranges):
        if e <= s:
            continue
        yt, xt = torch.as_tensor(yy), torch.as_tensor(xx)
        rgb, inv_d, T, _ = F._blend_tile(leaves[0], leaves[1], op, leaves[2], leaves[3], pl[s:e], xt.to(D), yt.to(D), cam.bg,
                                         alpha_cap_grad)
        L = 0.0
        if gP is not None:
            L = L + (rgb * gP[yt, xt]).sum()
        if gD is not None:
            L = L + (inv_d * gD[yt, xt]).sum()
        if gA is not None:
            L = L + ((1.0 - T) * gA[yt, xt]).sum()
        if not torch.is_tensor(L):
            continue
        for acc, g in zip(grads, torch.autograd.grad(L, leaves, allow_unused=True)):
            if g is not None:
                acc += g
    return grads


def _visible(scene, radii):
    """The scene restricted to the Gaussians with radius > 0, and their indices."""
    N = int(np.asarray(scene["means"]).reshape(-1, 3).shape[0])
    idx = np.nonzero(np.asarray(radii).reshape(-1) > 0)[0]
    sub = {k: np.asarray(scene[k]).reshape(N, -1)[idx] for k in ("means", "scales", "rotations", "opacities", "shs")}
    return sub, torch.as_tensor(idx), N


def _scatter(N, idx, *xs):
    out = []
    for x in xs:
        full = torch.zeros((N,) + tuple(x.shape[1:]), dtype=D)
        full[idx] = x
        out.append(full)
    return out


def camera_gradient_f64(scene, kw, radii, point_list, ranges, dpix=None, ddep=None, dalpha=None, alpha_cap_grad=True):
    """(grad (36,), scale (36,)) in the layout of gsr_backward_camera: view 0-15, proj 16-31, campos 32-34, 0.  `scale` is
    sum over Gaussians of |that Gaussian's term|.  radii / point_list / ranges: the forward's (visibility and lists)."""
    cam = Cam(kw)
    degree, sm = int(kw["degree"]), float(kw["scale_modifier"])
    sub, idx, N = _visible(scene, radii)
    n = int(idx.numel())
    if n == 0:
        return np.zeros(36), np.zeros(36)
    with torch.no_grad():
        geo = geometry(sub, kw, cam, cam.view, cam.proj, cam.campos, degree, sm)
    xy, con, col, invd = _scatter(N, idx, *geo)
    op = _scatter(N, idx, F._t(sub["opacities"], (n,)))[0]
    cot = blend_cotangents(xy, con, op, col, invd, point_list, ranges, cam, dpix, ddep, dalpha, alpha_cap_grad)
    gxy, gcon, gcol, ginv = [g[idx] for g in cot]
    Vn = cam.view.expand(n, 4, 4).clone().requires_grad_(True)
    Pn = cam.proj.expand(n, 4, 4).clone().requires_grad_(True)
    Cn = cam.campos.expand(n, 3).clone().requires_grad_(True)
    xy, con, col, invd = geometry(sub, kw, cam, Vn, Pn, Cn, degree, sm)
    L = (xy * gxy).sum() + (con * gcon).sum() + (col * gcol).sum() + (invd * ginv).sum()
    gV, gP, gC = torch.autograd.grad(L, (Vn, Pn, Cn), allow_unused=True)
    gV, gP, gC = [torch.zeros_like(x) if g is None else g for g, x in zip((gV, gP, gC), (Vn, Pn, Cn))]
    terms = torch.cat([gV.reshape(n, 16), gP.reshape(n, 16), gC, torch.zeros(n, 1, dtype=D)], 1)
    return terms.sum(0).numpy(), terms.abs().sum(0).numpy()


def camera_gradient_from_cotangents(scene, kw, radii, clamped, g_ndc, g_conic, g_colour, g_invd=None, chunk=262144):
    """camera_gradient_f64's second stage alone: the per-Gaussian geometry() VJP of given blend-stage cotangents, in the
    kernel's layout (the accumulator records gsr_backward_camera reads, include/gsr_camera_grads.h):
        g_ndc    (N, >= 2)  dL/dndc (not pixels: xy = ((ndc + 1) W - 1) / 2)
        g_conic  (N, 4)     dL/dA, HALF of dL/dB (conic_b_half), unused, dL/dC
        g_colour (N, 3)     dL/d(clamped colour); `clamped` (N, 3), the forward's clamped_state, says which channels pass
        g_invd   (N,)       dL/d(1/depth), or None (zero)
    Same (grad (36,), scale (36,)) as camera_gradient_f64.  The visible Gaussians (radii > 0) go through in chunks of `chunk`
    (per-Gaussian camera leaves: memory stays bounded at millions of Gaussians); terms and |terms| are summed in float64."""
    cam = Cam(kw)
    degree, sm = int(kw["degree"]), float(kw["scale_modifier"])
    N = int(np.asarray(scene["means"]).reshape(-1, 3).shape[0])
    idx = np.nonzero(np.asarray(radii).reshape(-1) > 0)[0]
    rows = lambda a: np.asarray(a).reshape(N, -1)
    arrays = {k: rows(scene[k]) for k in ("means", "scales", "rotations", "shs")}
    g_ndc, g_conic, g_colour, clamped = rows(g_ndc)[:, :2], rows(g_conic), rows(g_colour), rows(clamped)
    g_invd = None if g_invd is None else np.asarray(g_invd).reshape(N)
    grad, scale = torch.zeros(36, dtype=D), torch.zeros(36, dtype=D)
    w64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    for s in range(0, idx.size, chunk):
        ii = idx[s:s + chunk]
        n = ii.size
        sub = {k: a[ii] for k, a in arrays.items()}
        Vn = cam.view.expand(n, 4, 4).clone().requires_grad_(True)
        Pn = cam.proj.expand(n, 4, 4).clone().requires_grad_(True)
        Cn = cam.campos.expand(n, 3).clone().requires_grad_(True)
        xy, con, raw, invd = _geometry_raw(sub, kw, cam, Vn, Pn, Cn, degree, sm)
        gxy = w64(g_ndc[ii]) * torch.tensor([2.0 / cam.W, 2.0 / cam.H], dtype=D)     # dxy/dndc = (W / 2, H / 2)
        gc = w64(g_conic[ii])
        gcon = torch.stack([gc[:, 0], 2.0 * gc[:, 1], gc[:, 3]], 1)
        gcol = w64(g_colour[ii]) * (w64(clamped[ii]) == 0)                          # clamped channels pass nothing
        L = (xy * gxy).sum() + (con * gcon).sum() + (raw * gcol).sum()
        if g_invd is not None:
            L = L + (invd * w64(g_invd[ii])).sum()
        gV, gP, gC = torch.autograd.grad(L, (Vn, Pn, Cn), allow_unused=True)
        gV, gP, gC = [torch.zeros_like(x) if g is None else g for g, x in zip((gV, gP, gC), (Vn, Pn, Cn))]
        terms = torch.cat([gV.reshape(n, 16), gP.reshape(n, 16), gC, torch.zeros(n, 1, dtype=D)], 1)
        grad += terms.sum(0)
        scale += terms.abs().sum(0)
    return grad.numpy(), scale.numpy()


def loss_f64(scene, kw, view, proj, campos, radii, point_list, ranges, dpix=None, ddep=None, dalpha=None):
    """The float64 loss itself at a (view, proj, campos), with the forward's visibility and lists held fixed: what the
    finite differences of the yardstick are taken of."""
    cam = Cam(kw)
    sub, idx, N = _visible(scene, radii)
    n = int(idx.numel())
    with torch.no_grad():
        geo = geometry(sub, kw, cam, view, proj, campos, int(kw["degree"]), float(kw["scale_modifier"]))
        xy, con, col, invd = _scatter(N, idx, *geo)
        op = _scatter(N, idx, F._t(sub["opacities"], (n,)))[0]
        pl = torch.as_tensor(np.asarray(point_list, dtype=np.int64))
        total = torch.zeros((), dtype=D)
        cot = lambda a, shape: None if a is None else torch.as_tensor(np.asarray(a, np.float64)).reshape(shape)
        gP, gD, gA = cot(dpix, (cam.H, cam.W, 3)), cot(ddep, (cam.H, cam.W)), cot(dalpha, (cam.H, cam.W))
        for s, e, yy, xx in F._tiles(cam.W, cam.H, ranges):
            yt, xt = torch.as_tensor(yy), torch.as_tensor(xx)
            rgb, inv_d, T, _ = F._blend_tile(xy, con, op, col, invd, pl[s:e], xt.to(D), yt.to(D), cam.bg, True)
            if gP is not None:
                total += (rgb * gP[yt, xt]).sum()
            if gD is not None:
                total += (inv_d * gD[yt, xt]).sum()
            if gA is not None:
                total += ((1.0 - T) * gA[yt, xt]).sum()
    return float(total)
