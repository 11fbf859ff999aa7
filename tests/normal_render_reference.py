"""
Float64 yardstick for the Gaussians' normals, their image and the depth-normal consistency term (include/gsr_normal_render.h), and a
float32 restatement of the header's steps.

Test helper, not a test file.

  (a), (b)  normals_f64: torch float64, the header's definition; its VJP by torch autograd (vjp_f64).  A Gaussian whose
            |n_c . p_v| / |p_v| is below UNDECIDED (1e-4) is marked undecided: the side it faces is a float32 decision there, and its
            VJP row is left out of comparisons.  c* is exact on float32 inputs and needs no mask.
  (c), (d)  yardstick: the gradients are ONE pass of blend_grad_reference.blend_grads_f64 with colour = the normals, background 0
            and dL_dpixels = G.  c_k . dL_dpixels is then u_k = G . n_k, so the pass's dL_dmean2D, dL_dconic and dL_dopacity are the
            stage's accumulator columns with their `scale` units, its dL_dcolor is dL/d(normals), and its pixel mask is the module's.
            The image itself is the sum of the weights times the normals, the weights handed out by a pass with dL_dpixels = 1 as in
            features_reference.
  (e)       consistency_f64: torch float64 with autograd for the two gradients.  Pixels with |sqrt(L2) - 1e-3| < LENGTH_NEAR (1e-6)
            are marked: the count decision is a float32 one there.

The float32 restatement (numpy) takes nothing from float64: normals_f32 / normals_backward_f32 replay (a) and (b), render_f32 and
render_backward_f32 replay (c) and (d) on the same buffers with frame_walk_reference's walk, fma32 (one fused multiply-add per term)
and backward_block (the block sums in the header's order), with this stage's u = G . n and tail w G -- and consistency_f32 replays (e).
"""
import numpy as np
import torch

import blend_grad_reference as B
import frame_walk_reference as FWR

f32 = np.float32
EPS32 = FWR.EPS32
UNDECIDED = 1e-4
LENGTH_NEAR = 1e-6
MIN_LENGTH = f32(1e-3)
MIN_AXIS2 = f32(1e-24)
OUTPUTS = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dnormals")
COLUMNS = {"dL_dmean2D": (3, 4), "dL_dconic": (6, 7, 8, 9), "dL_dopacity": (10,)}
TOUCHED = (3, 4, 6, 7, 9, 10)
UNTOUCHED = (0, 1, 2, 5, 8, 11, 12, 13, 14, 15)
_np, criterion, rows_error = FWR.to_np, FWR.criterion, FWR.rows_error


def golden():
    """tests/golden/normal_render_margins.json: "E_f32" {frame: {output: the restatement's error on the CPU oracle's buffers}},
    "floor" (the smallest of them), "E_kernel" (what an MI355X run measured per frame, tools/record_normal_render_margins.py)."""
    return FWR.golden("normal_render_margins")


# ---- (a), (b) ----
def axis_index(scales):
    """c*: the smallest scale by strict < in index order (exact)."""
    s = _np(scales)
    c = np.zeros(len(s), np.int64)
    c = np.where(s[:, 1] < s[np.arange(len(s)), c], 1, c)
    c = np.where(s[:, 2] < s[np.arange(len(s)), c], 2, c)
    return c


def _axis_torch(q, c):
    """Column c (N,) of sigma3d.h's rotation matrix for quaternions q (N, 4) = (x, y, z, w), torch, any dtype."""
    v = torch.nn.functional.one_hot(torch.as_tensor(c), 3).to(q.dtype)
    qv, w = q[:, :3], q[:, 3:4]
    cs = 2.0 * w * w - 1.0
    cr = torch.linalg.cross(qv, v)
    d = (qv * v).sum(1, keepdim=True)
    return v * cs + cr * w * 2.0 + qv * d * 2.0


def normals_f64(scales, rots, means, view, q_tensor=None):
    """dict: n (N, 3) float64, c (N,), sigma (N,), ok (N,) bool, undecided (N,) bool; with q_tensor (a torch float64 leaf) also
    n_t, the torch result with c and sigma held constant."""
    c = axis_index(scales)
    q = torch.tensor(_np(rots, np.float64)) if q_tensor is None else q_tensor
    V = torch.tensor(_np(view, np.float64).reshape(4, 4))
    p = torch.tensor(_np(means, np.float64))
    a = _axis_torch(q, c)
    l2 = (a * a).sum(1)
    ok = (l2 >= float(MIN_AXIS2)) & (q.detach() != 0).any(1)
    ah = a / torch.sqrt(torch.where(ok, l2, torch.ones_like(l2)))[:, None]
    nc = ah @ V[:3, :3]
    pv = p @ V[:3, :3] + V[3, :3]
    t = (nc * pv).sum(1).detach()
    sigma = torch.where(t > 0, -1.0, 1.0).to(torch.float64)
    n = torch.where(ok[:, None], sigma[:, None] * nc, torch.zeros_like(nc))
    und = (t.abs() / pv.norm(dim=1).clamp_min(1e-300) < UNDECIDED) & ok
    out = dict(n=n.detach().numpy(), c=c, sigma=sigma.numpy(), ok=ok.numpy(), undecided=und.numpy())
    if q_tensor is not None:
        out["n_t"] = n
    return out


def vjp_f64(scales, rots, means, view, g):
    """(dq (N, 4) float64 by autograd, scale (N, 4): the sum of the magnitudes a float32 evaluation rounds against, r of normals_f64)."""
    q = torch.tensor(_np(rots, np.float64), requires_grad=True)
    r = normals_f64(scales, rots, means, view, q_tensor=q)
    gt = torch.tensor(_np(g, np.float64))
    (dq,) = torch.autograd.grad((r["n_t"] * gt).sum(), q)
    # the unit: every term of the header's formula with magnitudes taken
    qn = _np(rots, np.float64)
    V = _np(view, np.float64).reshape(4, 4)[:3, :3]
    c = r["c"]
    v = np.eye(3)[c]
    a = _axis_torch(torch.tensor(qn), c).numpy()
    l2 = (a * a).sum(1)
    s = np.sqrt(np.where(r["ok"], l2, 1.0))
    ah = a / s[:, None]
    gw = np.abs(_np(g, np.float64)) @ np.abs(V).T
    ga = (gw + np.abs(ah) * (np.abs(ah) * gw).sum(1, keepdims=True)) / s[:, None]
    x, w = np.abs(qn[:, :3]), np.abs(qn[:, 3:4])
    X = np.stack([v[:, 1] * ga[:, 2] + v[:, 2] * ga[:, 1], v[:, 2] * ga[:, 0] + v[:, 0] * ga[:, 2], v[:, 0] * ga[:, 1] + v[:, 1] * ga[:, 0]], 1)
    k =(x * ga).sum(1, keepdims=True)
    qc = x[np.arange(len(c)), c][:, None]
    cr = np.abs(np.cross(qn[:, :3], v))
    sc = np.concatenate([2 * w * X + 2 * qc * ga + 2 * k * v, 4 * w * ga[np.arange(len(c)), c][:, None] + 2 * (ga * cr).sum(1, keepdims=True)], 1)
    sc = np.where(r["ok"][:, None], sc, 0.0)
    return dq.numpy(), sc, r


def _walk_axis_f32(scales, rots):
    s, q = _np(scales, f32), _np(rots, f32)
    c = axis_index(s)
    v = np.eye(3, dtype=f32)[c]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    cs = f32(2) * w * w - f32(1)
    cr = np.stack([y * v[:, 2] - z * v[:, 1], z * v[:, 0] - x * v[:, 2], x * v[:, 1] - y * v[:, 0]], 1)
    d = x * v[:, 0]
    d = d + y * v[:, 1]
    d = d + z * v[:, 2]
    a = np.stack([(v[:, r] * cs + cr[:, r] * w * f32(2)) + q[:, r] * d * f32(2) for r in range(3)], 1)
    l2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    ok = (l2 >= MIN_AXIS2) & (q != 0).any(1)
    ln = np.sqrt(np.where(ok, l2, f32(1)))
    return c, v, q, cr, a / ln[:, None], ln, ok


def _facing_f32(ah, means, view):
    V, p = _np(view, f32).reshape(4, 4), _np(means, f32)
    nc = np.stack([(ah[:, 0] * V[0, j] + ah[:, 1] * V[1, j]) + ah[:, 2] * V[2, j] for j in range(3)], 1)
    pv = np.stack([((V[0, j] * p[:, 0] + V[1, j] * p[:, 1]) + V[2, j] * p[:, 2]) + V[3, j] for j in range(3)], 1)
    t = (nc[:, 0] * pv[:, 0] + nc[:, 1] * pv[:, 1]) + nc[:, 2] * pv[:, 2]
    return nc, np.where(t > 0, f32(-1), f32(1)), V


def normals_f32(scales, rots, means, view):
    """(n (N, 3) float32, c, sigma) by the header's (a)."""
    with np.errstate(all="ignore"):
        c, v, q, cr, ah, ln, ok = _walk_axis_f32(scales, rots)
        nc, sigma, _ = _facing_f32(ah, means, view)
        return np.where(ok[:, None], sigma[:, None] * nc, f32(0)).astype(f32), c, sigma


def normals_backward_f32(scales, rots, means, view, g):
    """dq (N, 4) float32 by the header's (b) (the addend)."""
    with np.errstate(all="ignore"):
        c, v, q, cr, ah, ln, ok = _walk_axis_f32(scales, rots)
        nc, sigma, V = _facing_f32(ah, means, view)
        gc = sigma[:, None] * _np(g, f32)
        gw = np.stack([(V[r, 0] * gc[:, 0] + V[r, 1] * gc[:, 1]) + V[r, 2] * gc[:, 2] for r in range(3)], 1)
        e = (ah[:, 0] * gw[:, 0] + ah[:, 1] * gw[:, 1]) + ah[:, 2] * gw[:, 2]
        ga = (gw - ah * e[:, None]) / ln[:, None]
        k = (q[:, 0] * ga[:, 0] + q[:, 1] * ga[:, 1]) + q[:, 2] * ga[:, 2]
        X = np.stack([v[:, 1] * ga[:, 2] - v[:, 2] * ga[:, 1], v[:, 2] * ga[:, 0] - v[:, 0] * ga[:, 2], v[:, 0] * ga[:, 1] - v[:, 1] * ga[:, 0]], 1)
        ar = np.arange(len(c))
        qc, gac, w = q[ar, c], ga[ar, c], q[:, 3]
        dq = [((f32(2) * w) * X[:, r] + (f32(2) * qc) * ga[:, r]) + (f32(2) * k) * v[:, r] for r in range(3)]
        dw = (f32(4) * w) * gac + f32(2) * ((ga[:, 0] * cr[:, 0] + ga[:, 1] * cr[:, 1]) + ga[:, 2] * cr[:, 2])
        return np.where(ok[:, None], np.stack(dq + [dw], 1), f32(0)).astype(f32)


# ---- (c), (d) ----
def yardstick(buf, W, H, normals, G):
    """One pass.  normals (N, 3), G (H, W, 3) dL/d(image); G is zeroed at the masked pixels on this side (the caller zeroes it there
    too).  Returns dict: image (H, W, 3) float64, mask (H, W) bool, G (the zeroed one), and one {"signed", "abs", "scale"} dict
    per OUTPUTS key."""
    xy, co, pl, rg = FWR.arrays(buf)
    n64 = _np(normals, np.float64)
    image = np.zeros((H, W, 3))
    ones = np.ones((H, W, 3))

    # the weights: colour-independent, so a first pass with dL_dpixels = 1 hands them out (terms["dL_dcolor"][:, :, 0])
    def on_tile(tile, xs, ys, idx, active, terms, masked):
        image[ys, xs] = terms["dL_dcolor"][:, :, 0] @ n64[idx]

    B.blend_grads_f64(xy, co[:, :3], co[:, 3], n64, np.zeros(len(n64)), pl, rg, np.zeros(3), W, H, ones, on_tile=on_tile)
    G64 = _np(G, np.float64).reshape(H, W, 3)
    ref = B.blend_grads_f64(xy, co[:, :3], co[:, 3], n64, np.zeros(len(n64)), pl, rg, np.zeros(3), W, H, G64, forward_n_contrib=buf["n_contrib"])
    r = dict(image=image, mask=ref["mask"], G=np.where(ref["mask"][..., None], 0.0, G64))
    for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity"):
        r[k] = ref[k]
    r["dL_dnormals"] = ref["dL_dcolor"]
    return r


def render_f32(buf, W, H, normals):
    """(H, W, 3) float32 by the header's (c)."""
    n32 = _np(normals, f32)
    fr = FWR.frame_of_buffers(buf, W, H)
    out = np.zeros((H, W, 3), f32)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        inside = (xs < W) & (ys < H)
        xs_, ys_ = xs[inside], ys[inside]
        acc, T = np.zeros((len(xs_), 3), f32), np.ones(len(xs_), f32)
        for applied, alpha, G, dx, dy, i, *_ in FWR.walk_f32(fr, s, e, xs_, ys_, np.ones(len(xs_), bool)):
            w = alpha * T
            T = np.where(applied, T * (f32(1) - alpha), T)
            for c in range(3):
                acc[:, c] = np.where(applied, FWR.fma32(w, n32[i, c], acc[:, c]), acc[:, c])
        out[ys_, xs_] = acc
    return out


def render_backward_f32(buf, W, H, normals, G, image, drop_suffix=False):
    """(acc (N, 16), dnormals (N, 3)) float32 by the header's (d) (only the six columns it adds to are non-zero).  drop_suffix: a
    WRONG backward that forgets the suffix term of dL/dalpha, for the test that shows the criterion sees it."""
    n32, G32, img = _np(normals, f32), _np(G, f32).reshape(H, W, 3), _np(image, f32).reshape(H, W, 3)
    fr = FWR.frame_of_buffers(buf, W, H)
    acc, dn = np.zeros((fr["N"], 16), f32), np.zeros((fr["N"], 3), f32)
    for tile, s, e, xs, ys in FWR.tiles(fr):
        for bx, by, inside in FWR.blocks(xs, ys, W, H):
            g, im = FWR.block_values(G32, bx, by, inside), FWR.block_values(img, bx, by, inside)
            total = (g[:, 0] * im[:, 0] + g[:, 1] * im[:, 1]) + g[:, 2] * im[:, 2]

            def entry(i, dx, dy, w):
                n = n32[i]
                return (g[:, 0] * n[0] + g[:, 1] * n[1]) + g[:, 2] * n[2], (w * g[:, 0], w * g[:, 1], w * g[:, 2])

            for i, tail in FWR.backward_block(fr, s, e, bx, by, inside, total, entry, acc, drop_suffix):
                dn[i] += tail
    return acc, dn


def layout(acc, dn, key):
    return FWR.layout(acc, key, COLUMNS, dn)


def backward_errors(acc, dn, r):
    """{key: worst per-Gaussian error in the key's scale}."""
    return FWR.backward_errors(acc, r, OUTPUTS, COLUMNS, dn)


def spread(a, b, r):
    """The worst difference of two runs' (acc, dnormals) in the same units."""
    return FWR.spread(a, b, r, OUTPUTS, COLUMNS)


def image_error(img, r):
    """max |img - image64| over the unmasked pixels (the normals are unit vectors: the unit is 1)."""
    d = np.abs(_np(img, np.float64).reshape(r["image"].shape) - r["image"])[~r["mask"]]
    return float(d.max()) if d.size else 0.0


# ---- (e) ----
def consistency_f64(Nimg, nd, valid, m, weight, W, H):
    """dict: sums (2,), gN, gnd (H, W, 3) float64 by autograd, counted (H, W) bool, near (H, W) bool (the undecided pixels), th."""
    N = torch.tensor(_np(Nimg, np.float64).reshape(H, W, 3), requires_grad=True)
    d = torch.tensor(_np(nd, np.float64).reshape(H, W, 3), requires_grad=True)
    mm = torch.ones(H, W, dtype=torch.float64) if m is None else torch.tensor(_np(m, np.float64).reshape(H, W))
    ln = N.detach().norm(dim=2)
    counted = (torch.tensor(_np(valid).reshape(H, W)) != 0) & (ln >= float(MIN_LENGTH))
    near = ((ln - float(MIN_LENGTH)).abs() < LENGTH_NEAR).numpy()
    th = N / torch.where(counted, N.norm(dim=2), torch.ones_like(ln))[..., None]
    terms = torch.where(counted, mm * (1.0 - (d * th).sum(2)), torch.zeros_like(mm))
    total = terms.sum()
    gN, gnd = torch.autograd.grad(total * (weight / (W * H)), (N, d))
    return dict(sums=np.array([float(total.detach()), float(torch.where(counted, mm, torch.zeros_like(mm)).sum())]), gN=gN.numpy(), gnd=gnd.numpy(),
                counted=counted.numpy(), near=near, th=th.detach().numpy(), terms=terms.detach().numpy())


def consistency_f32(Nimg, nd, valid, m, weight, W, H):
    """(sums (2,) float32, gN, gnd (H, W, 3) float32, counted) by the header's (e); the two sums are added in float64 and rounded
    once, as the kernel's tree does (its order differs: float64 addition of float32 terms is exact to 2^-29 of the total)."""
    N, d = _np(Nimg, f32).reshape(H, W, 3), _np(nd, f32).reshape(H, W, 3)
    mm = np.ones((H, W), f32) if m is None else _np(m, f32).reshape(H, W)
    c = f32(float(weight) / (float(W) * float(H)))
    with np.errstate(all="ignore"):
        L2 = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
        counted = (_np(valid).reshape(H, W) != 0) & (L2 >= MIN_LENGTH * MIN_LENGTH)
        s = np.sqrt(np.where(counted, L2, f32(1)))
        th = N / s[..., None]
        dot = (d[..., 0] * th[..., 0] + d[..., 1] * th[..., 1]) + d[..., 2] * th[..., 2]
        term = mm * (f32(1) - dot)
        km = c * mm
        gN = -((km[..., None] * (d - th * dot[..., None])) / s[..., None])
        gnd = -(km[..., None] * th)
    z = f32(0)
    sums = np.array([np.where(counted, term, z).astype(np.float64).sum(), np.where(counted, mm, z).astype(np.float64).sum()]).astype(f32)
    return sums, np.where(counted[..., None], gN, z).astype(f32), np.where(counted[..., None], gnd, z).astype(f32), counted


CPU_FRAMES = ("n300_50x37", "n2000_64x48", "n900_faint_48x32", "n1500_opaque_48x48", "toy", "one_gaussian_40x40", "behind_n300")


def case(scenes_mod, cameras_mod, name):
    """(scene, camera, render kwargs) of a CPU_FRAMES name: features_reference.SCENES and the three of test_gpu_features._case."""
    import features_reference as FR
    from conftest import lego_camera, render_kwargs
    if name in FR.SCENES:
        return FR.scene(scenes_mod, cameras_mod, name)
    if name == "toy":
        sc, cam = scenes_mod.toy_scene(), cameras_mod.toy_camera(image_width=120, image_height=90)
        return sc, cam, render_kwargs(sc, cam, train_convention=False)
    if name == "one_gaussian_40x40":
        cam = lego_camera(cameras_mod, 0, width=40, height=40)
        sc = scenes_mod.synthetic_scene(1, 0.05, 0.6, 1)
        sc["means"][:] = 0.0
        sc["scales"][:] = 3.0
        sc["opacities"][:] = 0.6
        return sc, cam, render_kwargs(sc, cam, width=40, height=40)
    if name == "behind_n300":
        cam = lego_camera(cameras_mod, 0, width=50, height=37)
        sc = scenes_mod.synthetic_scene(300, 0.05, 0.6, 5)
        c = np.asarray(cam["camera_center"], np.float32)
        fwd = np.asarray(cam["world_to_camera"], np.float64)[:3, 2]
        sc["means"] = (c - 3.0 * fwd + 0.1 * sc["means"]).astype(np.float32)
        return sc, cam, render_kwargs(sc, cam, width=50, height=37)
    raise KeyError(name)


def draw_G(H, W, seed=7):
    """dL/d(image) from U(-1, 1) / (W H): signed, as the consistency term's gradient is, and uneven, so that a swapped pixel shows."""
    return (np.random.default_rng(seed).uniform(-1, 1, (H, W, 3)) / (W * H)).astype(f32)


def draw_gaussians(N, seed=5, special=True):
    """scales (N, 3), rotations (N, 4), means (N, 3) float32 for (a) and (b): random, with ties between scales, non-unit quaternions
    and a zero quaternion mixed in where N allows."""
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(-3, 0, (N, 3))).astype(f32)
    q = rng.normal(0, 1, (N, 4)).astype(f32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    p = rng.uniform(-1.5, 1.5, (N, 3)).astype(f32)
    if special:
        q[::3] *= rng.uniform(0.3, 3.0, (len(q[::3]), 1)).astype(f32)          # non-unit
        s[1::5, 1] = s[1::5, 0]                                               # a tie between x and y
        s[2::7] = s[2::7, :1]                                                 # all equal: c* = 0
        if N > 4:
            q[4] = 0                                                          # a zero quaternion: the zero normal
    return s, q, p
