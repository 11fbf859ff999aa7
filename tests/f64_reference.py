"""
An independent float64 statement of what the reference's forward and backward compute (torch, CPU, autograd).

Test helper like tests/parity.py, not a test file.  It is written from SURVEY.md sections 2.2 and 8 and the reference's
Python (the line numbers below are those of the reference's forward.py / backward.py), not from oracle/ or the kernels:
the oracle restates the reference line by line in float32 and the kernels reproduce the oracle's expression order, so a
misreading shared by both would pass every parity test.  Here every operation is the plain mathematical one, in float64,
and the backward is autograd except for the one step (the cov3d backward) that is not the gradient of anything the
forward computes.  Nothing under the product package or oracle/ imports this module.

Inputs are the float32 arrays the kernels see (matrices, tan(fov), campos and the background rounded to float32 as the
reference's launch does, forward.py:694-695), widened to float64, so what a comparison measures is arithmetic, not
input rounding.

The reference's backward is not the gradient of its forward.  It is the textbook EWA gradient with a short
list of departures; each is a named switch in SWITCHES, defaulting to the reference's behaviour.  Flipping one away from
the reference (tests/test_f64_reference.py::test_each_reference_convention_is_load_bearing) must make the oracle
comparison fail, which is the evidence that a kernel getting that convention wrong would fail too.
"""
import numpy as np
import torch

TILE = 16
D = torch.float64

# Every way the reference's backward departs from the true gradient of the EWA model.  True = the reference's behaviour.
SWITCHES = {
    # backward.py:700 accumulates -0.5*gdx*d_y*dL_dG into dL_dconic[1]: HALF the derivative with respect to the stored conic
    # entry B (power = -0.5(A dx^2 + C dy^2) - B dx dy); backward.py:382 multiplies it by 2 in dL_db.
    "conic_b_half": True,
    # backward.py:377: the conic -> Sigma2D step scales by 1/(denom^2 + 1e-7), not 1/denom^2.
    "denom_eps": True,
    # Q1: the blend sees the forward's Sigma2D = J W Sigma W^T J^T (forward.py:118-141); the backward differentiates the
    # textbook form J W^T Sigma W J^T (backward.py:333-356), W = view[0:3, 0:3] as stored.
    "q1_textbook_backward": True,
    # Q2: dL_dscale / dL_drot come from M = S R with the 1-2(y^2+z^2) rotation matrix (backward.py:478-499), dL_dM = 2 M dSigma
    # (:514), columns of R and dL_dM in dL_dscale (:521-526) and the literal quaternion formula (:533-556).  False: the
    # true gradient of the forward's Sigma3D = R S S^T R^T with Warp's quat_to_matrix (forward.py:147-186).
    "q2_cov3d_literal": True,
    # Q16: backward() never passes scale_modifier to backward_preprocess (backward.py:1155-1182; default 1.0 at :805).
    "q16_bwd_scale_modifier_one": True,
    # Q3: (dL_dt, 1.0) * transpose(view) (backward.py:433-434) adds view[j][3] to dL_dmean3D[j]: zero under train.py's
    # world_to_camera, the translation under render.py's un-transposed world_to_view.
    "q3_view_column_term": True,
    # backward.py:303-319: outside the 1.3*tan limit the tx (ty) gradient is zeroed (:319) and the tz terms use the clamped
    # tx as if it were free (:312-318).  False: the true gradient of tx = clamp(tx/tz) * tz.
    "frustum_clamp_grad": True,
    # backward.py:107: no SH gradient at all (dL_dshs nor the direction term) where |mean - campos| < 1e-8.
    "sh_skip_at_campos": True,
    # backward.py:390-400 and :506-510: dL_dcov3D's off-diagonal entries are derivatives with respect to the packed VEC6
    # parameter (both symmetric matrix entries), and the cov3d backward halves them back into dL_dSigma.  False: the cov2d
    # step writes the per-matrix-entry derivative (half), the cov3d step still halves it.
    "vec6_offdiag_param": True,
    # Found while writing this module (not on the issue's list): backward.py:683 forms dL_dG = opacity * dL_dalpha whether or
    # not alpha = min(0.99, opacity * G) (:652) sat at the 0.99 cap, so the gradient passes the cap.  False: zero past the cap.
    "alpha_cap_passes_grad": True,
    # Found while writing this module: dnormvdv returns zero when |v|^2 < 1e-10 (backward.py:53), i.e. the SH direction
    # term of dL_dmean3D is dropped for 1e-8 <= |mean - campos| < 1e-5.  False: the true derivative of v / |v|.
    "dnormvdv_floor": True,
}

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)


def _sw(switches):
    s = dict(SWITCHES)
    if switches:
        unknown = set(switches) - set(SWITCHES)
        assert not unknown, f"unknown switches {unknown}"
        s.update(switches)
    return s


def _t(x, shape=None):
    """float32 rounding (what the kernel sees), then float64.  A float64 tensor passes through (autograd leaves)."""
    if torch.is_tensor(x):
        return x.reshape(shape) if shape is not None else x
    a = torch.as_tensor(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))
    return a.reshape(shape) if shape is not None else a


def _grad_through(x, k):
    """Value x, gradient scaled by k (k is not differentiated)."""
    k = k.detach()
    return x * k + (x - x * k).detach()


class Camera:
    """The float32 camera inputs of one render call, widened to float64."""

    def __init__(self, kw):
        self.W, self.H = int(kw["image_width"]), int(kw["image_height"])
        self.view = _t(kw["viewmatrix"], (4, 4))
        self.proj = _t(kw["projmatrix"], (4, 4))
        self.campos = _t(np.asarray(kw["campos"])[:3])
        self.tanx = float(np.float32(kw["tan_fovx"]))
        self.tany = float(np.float32(kw["tan_fovy"]))
        self.bg = _t(np.asarray(kw["background"])[:3])


def _homog(p):
    return torch.cat([p, torch.ones_like(p[:, :1])], dim=1)


def quat_to_matrix_warp(q):
    """Q4: (x,y,z,w) storage; column i of R is quat_rotate(q, e_i) = e_i(2w^2-1) + cross(q.xyz, e_i) 2w + q.xyz dot(q.xyz, e_i) 2."""
    v, w = q[:, :3], q[:, 3]
    N = q.shape[0]
    cols = []
    for i in range(3):
        e = torch.zeros(N, 3, dtype=q.dtype)
        e[:, i] = 1.0
        cols.append(e * (2 * w * w - 1)[:, None] + torch.cross(v, e, dim=1) * (2 * w)[:, None] + v * (2 * v[:, i])[:, None])
    return torch.stack(cols, dim=2)


def quat_to_matrix_std(q):
    """The 1 - 2(y^2+z^2) form the cov3d backward builds (backward.py:478-488), (x,y,z,w) storage, not normalised."""
    x, y, z, r = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
        torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
        torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def vec6(S):
    """VEC6 upper-triangle order (xx, xy, xz, yy, yz, zz) (forward.py:186)."""
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def unvec6(c):
    r0 = torch.stack([c[:, 0], c[:, 1], c[:, 2]], 1)
    r1 = torch.stack([c[:, 1], c[:, 3], c[:, 4]], 1)
    r2 = torch.stack([c[:, 2], c[:, 4], c[:, 5]], 1)
    return torch.stack([r0, r1, r2], 1)


def cov3d(scales, rots, scale_modifier):
    """forward.py:147-186: Sigma = (R S)(R S)^T, R = quat_to_matrix (Warp), S = diag(scale_modifier * scale)."""
    M = quat_to_matrix_warp(rots) * (scale_modifier * scales)[:, None, :]
    return vec6(M @ M.transpose(1, 2))


def sh_colour(shs, dirs, degree):
    """forward.py:310-352: SH evaluation of degree 0..3 + 0.5 (before the clamp).  shs (N,16,3), dirs (N,3) unit or 0."""
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    r = SH_C0 * shs[:, 0]
    if degree > 0:
        r = r - SH_C1 * y * shs[:, 1] + SH_C1 * z * shs[:, 2] - SH_C1 * x * shs[:, 3]
        if degree > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            r = (r + SH_C2[0] * xy * shs[:, 4] + SH_C2[1] * yz * shs[:, 5] + SH_C2[2] * (2 * zz - xx - yy) * shs[:, 6]
                 + SH_C2[3] * xz * shs[:, 7] + SH_C2[4] * (xx - yy) * shs[:, 8])
            if degree > 2:
                r = (r + SH_C3[0] * y * (3 * xx - yy) * shs[:, 9] + SH_C3[1] * xy * z * shs[:, 10]
                     + SH_C3[2] * y * (4 * zz - xx - yy) * shs[:, 11] + SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * shs[:, 12]
                     + SH_C3[4] * x * (4 * zz - xx - yy) * shs[:, 13] + SH_C3[5] * z * (xx - yy) * shs[:, 14]
                     + SH_C3[6] * x * (xx - 3 * yy) * shs[:, 15])
    return r + 0.5


def _absmm(p, M):
    """|[p, 1]| @ |M|: the magnitude a float32 dot product of [p, 1] with the columns of M rounds against."""
    return _homog(p).abs() @ M.abs()


def _sh_terms(shs, dirs, degree):
    """sum_k |basis_k(dir) sh_k| per channel: the magnitude the float32 SH sum rounds against."""
    n = (degree + 1) ** 2
    e = torch.eye(16, dtype=D)
    basis = torch.stack([sh_colour(e[k].expand(dirs.shape[0], 16)[:, :, None].expand(-1, 16, 3), dirs, degree)[:, 0] - 0.5
                         for k in range(n)], 1)
    return (basis[:, :, None].abs() * shs[:, :n].abs()).sum(1)


def _frustum_t(t, cam, true_clamp_grad):
    """forward.py:107-113 / backward.py:303-319: tx, ty clamped to 1.3 tan(fov) * tz."""
    tz = t[:, 2]
    out = []
    for k, tan in ((0, cam.tanx), (1, cam.tany)):
        lim = 1.3 * tan
        r = t[:, k] / tz
        clamped = (r < -lim) | (r > lim)
        c = torch.clamp(r, -lim, lim) * tz
        out.append(c if true_clamp_grad else torch.where(clamped, c.detach(), t[:, k]))
    return out[0], out[1], tz


def cov2d(t, cov6, cam, form, true_clamp_grad=True, info=None):
    """Sigma2D as (a, b, c) before the 0.3 blur.  form "forward": T = J W, J W Sigma W^T J^T (forward.py:118-141, Q1);
    form "textbook": J W^T Sigma W J^T (backward.py:333-356).  W = view[0:3, 0:3] as stored (row-vector convention)."""
    tx, ty, tz = _frustum_t(t, cam, true_clamp_grad)
    fx, fy = cam.W / (2.0 * cam.tanx), cam.H / (2.0 * cam.tany)
    N = t.shape[0]
    J = torch.zeros(N, 2, 3, dtype=D)
    J[:, 0, 0] = fx / tz
    J[:, 0, 2] = -fx * tx / (tz * tz)
    J[:, 1, 1] = fy / tz
    J[:, 1, 2] = -fy * ty / (tz * tz)
    Wm = cam.view[:3, :3]
    T = J @ (Wm if form == "forward" else Wm.T)
    S2 = T @ unvec6(cov6) @ T.transpose(1, 2)
    if info is not None:
        info["T_absmax"] = T.detach().abs().amax((1, 2))
    return S2[:, 0, 0], S2[:, 0, 1], S2[:, 1, 1]


def conic_of(a, b, c, denom_eps=False):
    """forward.py:265-285: the blurred Sigma2D's inverse as (A, B, C) = (c, -b, a) / det.  With denom_eps the gradient
    (not the value) carries the reference backward's 1/(det^2 + 1e-7) (backward.py:377) instead of 1/det^2."""
    a, c = a + 0.3, c + 0.3
    det = a * c - b * b
    con = torch.stack([c / det, -b / det, a / det], 1)
    if denom_eps:
        d2 = (det * det).detach()
        con = _grad_through(con, (d2 / (d2 + 1e-7))[:, None])
    return con, a, b, c, det


def _ndc2pix(v, size):
    return ((v + 1.0) * size - 1.0) * 0.5


def preprocess_f64(scene, kw, degree, scale_modifier):
    """forward.py:190-382 in float64.  Returns a dict of float64 tensors / numpy masks; culled entries are zero (Q11:
    cov3D is written unless the near-plane test culled).  Rectangles use C truncation (Q12)."""
    cam = Camera(kw)
    N = int(scene["means"].shape[0])
    means = _t(scene["means"], (N, 3))
    scales, rots = _t(scene["scales"], (N, 3)), _t(scene["rotations"], (N, 4))
    shs = _t(scene["shs"], (N, 16, 3))
    op = _t(scene["opacities"], (N,))
    p_view = _homog(means) @ cam.view
    p_hom = _homog(means) @ cam.proj
    p_w = 1.0 / (p_hom[:, 3] + 1e-7)                                       # forward.py:255
    ndc = p_hom[:, :2] * p_w[:, None]
    c6 = cov3d(scales, rots, scale_modifier)
    a0, b0, c0 = cov2d(p_view[:, :3], c6, cam, "forward")
    con, a, b, c, det = conic_of(a0, b0, c0)
    mid = 0.5 * (a + c)
    l1 = mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))            # forward.py:288-292
    l2 = mid - torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    radius_f = 3.0 * torch.sqrt(torch.maximum(l1, l2))                     # the value ceil() rounds
    radius = torch.ceil(radius_f)
    pix = torch.stack([_ndc2pix(ndc[:, 0], cam.W), _ndc2pix(ndc[:, 1], cam.H)], 1)
    gx, gy = (cam.W + TILE - 1) // TILE, (cam.H + TILE - 1) // TILE
    pn, rn = pix.detach().numpy(), radius.detach().numpy()
    rect_f = np.stack([(pn[:, 0] - rn) / TILE, (pn[:, 1] - rn) / TILE,
                       (pn[:, 0] + rn + TILE - 1) / TILE, (pn[:, 1] + rn + TILE - 1) / TILE], 1)   # forward.py:64-76
    rect = np.clip(np.trunc(rect_f), 0, [gx, gy, gx, gy]).astype(np.int64)
    near = (p_view[:, 2] < 0.2).numpy()                                    # forward.py:250
    zero_det = (det == 0).numpy()
    empty = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]) == 0     # forward.py:301
    culled = near | zero_det | empty
    d = means - cam.campos
    ln = torch.sqrt((d * d).sum(1))
    dirs = torch.where((ln > 0)[:, None], d / torch.where(ln > 0, ln, torch.ones_like(ln))[:, None], torch.zeros_like(d))
    raw = sh_colour(shs, dirs, degree)
    clamped = (raw < 0).detach().numpy()
    colour = torch.where(torch.as_tensor(clamped), torch.zeros_like(raw), raw)   # forward.py:354-358 (clamped=True)
    keep = torch.as_tensor(~culled)
    k1 = keep[:, None].to(D)
    return {
        "cam": cam, "N": N, "culled": culled, "near": near, "clamped": clamped & ~culled[:, None],
        "radii": np.where(culled, 0, rn).astype(np.int64), "radius_f": radius_f.detach().numpy(), "rect": rect, "rect_f": rect_f,
        "xy": pix * k1, "ndc": ndc, "depth": p_view[:, 2] * keep, "cov3D": c6 * (~torch.as_tensor(near))[:, None].to(D),
        "conic": con * k1, "opacity": op * keep, "colour": colour * k1,
        "det": det, "p_view": p_view,
        # magnitudes for the float32 error models of tests/test_f64_reference.py
        "ndc_scale": (p_w.abs()[:, None] * (_absmm(means, cam.proj[:, :2]) + ndc.abs() * _absmm(means, cam.proj[:, 3:4]))).detach().numpy(),
        "w_cond": torch.clamp(p_w.abs() * _absmm(means, cam.proj[:, 3:4])[:, 0], min=1.0).detach().numpy(),
        "kappa": (l1 / (mid - torch.sqrt(torch.clamp(mid * mid - det, min=0.0)))).detach().numpy(),
        "depth_scale": _absmm(means, cam.view[:, 2:3])[:, 0].detach().numpy(),
        "colour_raw": raw.detach().numpy(),
        "colour_scale": _sh_terms(shs, dirs, degree).detach().numpy(),
    }


def _blend_tile(xy, conic, op, col, inv_depth, idx, px, py, bg, alpha_cap_grad):
    """One 16x16 tile, front to back over `idx` (its slice of point_list), dense [pixels x list] (forward.py:385-515).
    The discrete decisions are taken in float64 under no_grad; the values carry gradients."""
    L = idx.numel()
    P = px.numel()
    if L == 0:
        return (bg[None, :].expand(P, 3).clone(), torch.zeros(P, dtype=D), torch.ones(P, dtype=D),
                torch.zeros(P, dtype=torch.int64))
    g = lambda a: a[idx]
    dx = g(xy)[None, :, 0] - px[:, None]
    dy = g(xy)[None, :, 1] - py[:, None]
    cg = g(conic)
    power = -0.5 * (cg[None, :, 0] * dx * dx + cg[None, :, 2] * dy * dy) - cg[None, :, 1] * dx * dy
    G = torch.exp(power)
    a_raw = g(op)[None, :] * G
    capped = a_raw > 0.99
    # value min(0.99, o G); past the cap the gradient is o G's (backward.py:683) or, flipped, zero (the true derivative)
    at_cap = (a_raw - a_raw.detach() + 0.99) if alpha_cap_grad else torch.full_like(a_raw, 0.99)
    alpha = torch.where(capped, at_cap, a_raw)
    with torch.no_grad():
        keep = (power <= 0) & (alpha >= 1.0 / 255.0)                      # forward.py:476, :481
        om = torch.where(keep, 1.0 - alpha, torch.ones_like(alpha))
        T_in = torch.cumprod(torch.cat([torch.ones(P, 1, dtype=D), om[:, :-1]], 1), 1)
        stop = keep & (T_in * om < 1e-4)                                   # forward.py:486-488: the stopping one is excluded
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


def _tiles(W, H, ranges):
    gx = (W + TILE - 1) // TILE
    ranges = np.asarray(ranges).reshape(-1, 2)
    for tid in range(ranges.shape[0]):
        tx, ty = tid % gx, tid // gx
        xs = np.arange(tx * TILE, min(W, tx * TILE + TILE))
        ys = np.arange(ty * TILE, min(H, ty * TILE + TILE))
        yy, xx = np.meshgrid(ys, xs, indexing="ij")
        yield int(ranges[tid, 0]), int(ranges[tid, 1]), yy.ravel(), xx.ravel()


def blend_f64(xy, conic, opacity, colour, depth, point_list, ranges, bg, W, H, alpha_cap_grad=True, dL_dpixels=None,
              wrt=None):
    """Front-to-back blend (forward.py:385-515) in float64.  Returns (image (H,W,3), inverse depth, final_T, n_contrib).
    With `dL_dpixels` the blend is also differentiated tile by tile (bounded memory) and the gradients with respect to the
    tensors in `wrt` (a tuple) are returned as a 5th item.  Without it the outputs are one differentiable graph."""
    pl = torch.as_tensor(np.asarray(point_list, dtype=np.int64))
    inv_depth = torch.where(depth > 0, 1.0 / torch.where(depth > 0, depth, torch.ones_like(depth)), torch.zeros_like(depth))
    img = torch.zeros(H, W, 3, dtype=D)
    dep, fT = torch.zeros(H, W, dtype=D), torch.zeros(H, W, dtype=D)
    nc = torch.zeros(H, W, dtype=torch.int64)
    grads = None
    if dL_dpixels is not None:
        dpix = torch.as_tensor(np.asarray(dL_dpixels, dtype=np.float64)).reshape(H, W, 3)
        grads = [torch.zeros_like(t) for t in wrt]
    out_img, out_dep, out_T = [], [], []
    for s, e, yy, xx in _tiles(W, H, ranges):
        yt, xt = torch.as_tensor(yy), torch.as_tensor(xx)
        rgb, inv_d, T, n = _blend_tile(xy, conic, opacity, colour, inv_depth, pl[s:e], xt.to(D), yt.to(D), bg, alpha_cap_grad)
        if grads is not None:
            if e > s:
                gs = torch.autograd.grad((rgb * dpix[yt, xt]).sum(), wrt, allow_unused=True, retain_graph=False)
                for acc, gg in zip(grads, gs):
                    if gg is not None:
                        acc += gg
            rgb, inv_d, T = rgb.detach(), inv_d.detach(), T.detach()
            img[yt, xt], dep[yt, xt], fT[yt, xt] = rgb, inv_d, T
        else:
            out_img.append((yt, xt, rgb)); out_dep.append(inv_d); out_T.append(T)
        nc[yt, xt] = n
    if grads is None:
        idx = torch.cat([yt * W + xt for yt, xt, _ in out_img]) if out_img else torch.zeros(0, dtype=torch.int64)
        order = torch.argsort(idx)
        img = torch.cat([r for _, _, r in out_img])[order].reshape(H, W, 3)
        dep = torch.cat(out_dep)[order].reshape(H, W)
        fT = torch.cat(out_T)[order].reshape(H, W)
        return img, dep, fT, nc
    return img, dep, fT, nc, grads


def geometry_vjp_f64(scene, kw, degree, visible, clamped, dL_dndc, dL_dconic, dL_dcolour, switches=None, cov3D=None):
    """Stage 2 of the backward: the VJP of the BACKWARD-convention geometry (mean3D, Sigma3D (VEC6), SH) ->
    (NDC xy, conic, colour) with the blend stage's cotangents, for the Gaussians in `visible` (radii > 0); `clamped` is the
    forward's colour-clamp state; `cov3D` the forward's Sigma3D buffer (default: recomputed in float64).  dL_dconic is as the reference stores it ((N,4): A, B-as-stored, unused, C).  Returns
    (dL_dmean3D, dL_dshs (N*16,3), dL_dcov3D (N,6)) as float64 tensors, and the three parts of dL_dmean3D separately
    followed by a dict of magnitudes for error models."""
    s = _sw(switches)
    cam = Camera(kw)
    N = np.asarray(scene["means"]).reshape(-1, 3).shape[0]
    vis = torch.as_tensor(np.asarray(visible, dtype=bool))
    means = _t(scene["means"], (N, 3)).requires_grad_(True)
    shs = _t(scene["shs"], (N, 16, 3)).requires_grad_(True)
    if cov3D is None:
        c6 = cov3d(_t(scene["scales"], (N, 3)), _t(scene["rotations"], (N, 4)), float(kw["scale_modifier"]))
    else:                                  # the forward buffer the backward reads (backward.py:1113), widened
        c6 = torch.as_tensor(np.asarray(cov3D, np.float64)).reshape(N, 6)
    c6 = c6.detach().requires_grad_(True)
    vf = vis[:, None].to(D)
    dndc = torch.as_tensor(np.asarray(dL_dndc, np.float64)).reshape(N, 3)[:, :2] * vf
    dcon = torch.as_tensor(np.asarray(dL_dconic, np.float64)).reshape(N, 4)
    b_mul = 2.0                                                             # backward.py:382 (factor 2 in dL_db)
    dcon = torch.stack([dcon[:, 0], b_mul * dcon[:, 1], dcon[:, 3]], 1) * vf
    dcol = torch.as_tensor(np.asarray(dL_dcolour, np.float64)).reshape(N, 3) * vf
    # projection (backward.py:709-768): the true derivative of p_hom.xy / (p_hom.w + 1e-7)
    ph = _homog(means) @ cam.proj
    ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    g_proj = torch.autograd.grad((ndc * dndc).sum(), means)[0]
    # cov2d (backward.py:259-435)
    t = (_homog(means) @ cam.view)[:, :3]
    info = {}
    a0, b0, c0 = cov2d(t, c6, cam, "textbook" if s["q1_textbook_backward"] else "forward",
                       true_clamp_grad=not s["frustum_clamp_grad"], info=info)
    con, a, b, c, det = conic_of(a0, b0, c0, denom_eps=s["denom_eps"])
    # magnitude the float32 cov2d step rounds against (before cancellation): |T|^2 (a + |b| + c)^2 |dL_dconic|_1 / det^2
    info["cov_scale"] = (info["T_absmax"] ** 2 * (a + b.abs() + c) ** 2 * dcon.abs().sum(1) / det ** 2).detach()
    g_cov, dcov6 = torch.autograd.grad((con * dcon).sum(), (means, c6))
    if s["q3_view_column_term"]:
        g_cov = g_cov + cam.view[:3, 3][None, :] * vf                      # backward.py:433-434
    if not s["vec6_offdiag_param"]:
        dcov6 = dcov6 * torch.tensor([1.0, 0.5, 0.5, 1.0, 0.5, 1.0], dtype=D)
    # SH (backward.py:69-255)
    d = means - cam.campos
    ln2 = (d * d).sum(1)
    ln = torch.sqrt(ln2.detach())
    skip = (ln < 1e-8) if s["sh_skip_at_campos"] else torch.zeros(N, dtype=torch.bool)
    safe = torch.where(ln > 0, ln, torch.ones_like(ln))
    frozen = (ln2.detach() < 1e-10) if s["dnormvdv_floor"] else (ln == 0)   # backward.py:53: no direction term
    d_n = torch.where(frozen[:, None], d.detach() / safe[:, None],
                      d / torch.sqrt(torch.where(frozen, torch.ones_like(ln2), ln2))[:, None])
    d_n = torch.where((ln > 0)[:, None], d_n, torch.zeros_like(d_n))       # forward.py:306-308: direction 0 at campos
    raw = sh_colour(shs, d_n, degree)
    keep_c = torch.as_tensor(~np.asarray(clamped, dtype=bool).reshape(N, 3)).to(D)
    w_sh = (dcol * keep_c * (~skip)[:, None].to(D))
    g_sh_mean, dshs = torch.autograd.grad((raw * w_sh).sum(), (means, shs), allow_unused=True)
    g_sh_mean = torch.zeros_like(means) if g_sh_mean is None else g_sh_mean    # degree 0: no direction term
    out = g_proj + g_cov + g_sh_mean
    return out.detach(), dshs.detach().reshape(N * 16, 3), dcov6.detach(), (g_proj.detach(), g_cov.detach(), g_sh_mean.detach(), info)


def cov3d_backward_f64(scene, kw, visible, dL_dcov3D, switches=None):
    """Stage 3 (backward.py:439-556): dL_dscale (N,3), dL_drot (N,4; (x,y,z,w)) from dL_dcov3D.

    The reference step is not the gradient of anything the forward computes (Q2), but it has a closed form that autograd
    reproduces: it is the VJP of (scale, q) -> R_std(q) diag(s), s = scale_modifier_bwd * scale, with the constant
    cotangent G = 2 diag(s) R_std(q) dSigma, where R_std is the 1-2(y^2+z^2) matrix of backward.py:478-488 and dSigma the
    symmetric matrix of dL_dcov3D with halved off-diagonal entries (:506-510).  (dL_dscale[k] = sum_j R[j][k] G[j][k] is
    :521-526; the quaternion formula of :533-556 is d/dq sum_ij G[j][i] s_i R_std[j][i].)"""
    s = _sw(switches)
    N = np.asarray(scene["means"]).reshape(-1, 3).shape[0]
    vf = torch.as_tensor(np.asarray(visible, dtype=bool))[:, None].to(D)
    scales = _t(scene["scales"], (N, 3)).requires_grad_(True)
    q = _t(scene["rotations"], (N, 4)).requires_grad_(True)
    dc = torch.as_tensor(np.asarray(dL_dcov3D, np.float64)).reshape(N, 6) * vf
    sm = 1.0 if s["q16_bwd_scale_modifier_one"] else float(kw["scale_modifier"])
    if s["q2_cov3d_literal"]:
        R = quat_to_matrix_std(q)
        sv = sm * scales
        with torch.no_grad():
            dSig = unvec6(dc * torch.tensor([1.0, 0.5, 0.5, 1.0, 0.5, 1.0], dtype=D))
            G = 2.0 * (sv[:, :, None] * R) @ dSig
        f = (G * (R * sv[:, None, :])).sum()
    else:
        f = (cov3d(scales, q, sm) * dc).sum()
    gs, gq = torch.autograd.grad(f, (scales, q))
    return (gs * vf).detach(), (gq * vf).detach()


def backward_f64(scene, kw, point_list, ranges, dL_dpixels, switches=None, pre=None):
    """The reference's backward (backward.py:955-1196) as two chained VJPs plus the cov3d step:
      1. autograd of blend_f64 with cotangent dL_dpixels -> gradients w.r.t. NDC xy, the forward conic, opacity, colour;
      2. geometry_vjp_f64 (backward-convention geometry) with those cotangents -> dL_dmean3D, dL_dshs, dL_dcov3D;
      3. cov3d_backward_f64 -> dL_dscale, dL_drot.
    Returns the reference's nine arrays as float64 numpy (dL_dcov3D all zero: backward.py:1119 returns it unfilled), plus
    `_dL_dcov3D_local` and `_mean3D_parts`."""
    s = _sw(switches)
    if pre is None:
        pre = preprocess_f64(scene, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    cam, N = pre["cam"], pre["N"]
    xy = pre["xy"].detach().clone().requires_grad_(True)
    con = pre["conic"].detach().clone().requires_grad_(True)
    op = pre["opacity"].detach().clone().requires_grad_(True)
    col = pre["colour"].detach().clone().requires_grad_(True)
    *_, (gxy, gcon, gop, gcol) = blend_f64(xy, con, op, col, pre["depth"].detach(), point_list, ranges, cam.bg, cam.W, cam.H,
                                           alpha_cap_grad=s["alpha_cap_passes_grad"], dL_dpixels=dL_dpixels,
                                           wrt=(xy, con, op, col))
    dL_dmean2D = torch.zeros(N, 3, dtype=D)
    dL_dmean2D[:, 0] = gxy[:, 0] * (0.5 * cam.W)                            # d pix / d ndc (backward.py:690-693)
    dL_dmean2D[:, 1] = gxy[:, 1] * (0.5 * cam.H)
    dL_dconic = torch.zeros(N, 4, dtype=D)
    dL_dconic[:, 0], dL_dconic[:, 3] = gcon[:, 0], gcon[:, 2]
    dL_dconic[:, 1] = gcon[:, 1] * (0.5 if s["conic_b_half"] else 1.0)     # backward.py:700
    visible = ~pre["culled"]
    m3, dshs, dcov6, parts = geometry_vjp_f64(scene, kw, int(kw["degree"]), visible, pre["clamped"], dL_dmean2D, dL_dconic,
                                              gcol, switches)
    dsc, drot = cov3d_backward_f64(scene, kw, visible, dcov6, switches)
    n = lambda x: x.detach().numpy()
    return {
        "dL_dmean3D": n(m3), "dL_dcolor": n(gcol), "dL_dshs": n(dshs), "dL_dopacity": n(gop), "dL_dscale": n(dsc),
        "dL_drot": n(drot), "dL_dmean2D": n(dL_dmean2D), "dL_dconic": n(dL_dconic), "dL_dcov3D": np.zeros((N, 6)),
        "_dL_dcov3D_local": n(dcov6), "_mean3D_parts": tuple(n(p) for p in parts[:3]),
    }
