"""The float64 yardstick of include/gsr_normals.h: normals from the rendered depth, their gradient back to the inverse-depth and alpha
images, and the cosine loss against a normal prior.  Never the kernel: numpy and torch on the CPU.

Validity is a float32 decision (the header spells out every operation), so decide() restates exactly those operations in numpy
float32 and everything else here takes its validity pattern from it: `valid` is compared with the kernel's exactly.  Values are
float64 from the float32 inputs (A = 1 - final_T is the float32 difference, as the header has it).

    reference(case)        normals, loss sums and gradients in float64; the gradients by torch autograd
    closed_form(case)      the header's gather written out in float64 numpy: agrees with autograd to 1e-10 (test_normals_reference.py)
    restatement32(case)    the same formulas in numpy float32: what a float32 implementation can be expected to reach
    kappa(case)            the cancellation factor: the largest |P| / min(|a|, |b|) over valid pixels.  The differences a and b are
                           formed from points of size |P|, so they carry eps32 |P| of rounding, a share eps32 kappa of themselves.
                           Errors of normals are stated in units of eps32 kappa, errors of gradients in eps32 kappa max|ref|.
"""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
MIN_NORM2 = np.float32(1e-12)          # GSR_NORMALS_MIN_NORM2
ALPHA_MIN = 0.5                        # GSR_NORMALS_ALPHA_MIN
FLT_MAX = np.finfo(np.float32).max


def camera(W, H, tan_fovx=0.5, tan_fovy=None):
    """A camera dict as normals.py takes it; the tangents are float32 values, as the library receives them."""
    tan_fovy = tan_fovx * H / W if tan_fovy is None else tan_fovy
    return {"tan_fovx": float(np.float32(tan_fovx)), "tan_fovy": float(np.float32(tan_fovy)), "width": int(W), "height": int(H)}


def _shift(a, dy, dx, fill=np.nan):
    """out[y, x] = a[y + dy, x + dx], `fill` where that lies outside."""
    out = np.full_like(a, fill)
    H, W = a.shape[:2]
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def rays(cam, dtype=np.float64):
    """(rx (W,), ry (H,)) in `dtype`, each operation rounded in it (float32: the header's operations)."""
    f = dtype
    W, H = cam["width"], cam["height"]
    rx = ((2 * np.arange(W) + 1).astype(f) / f(W) - f(1)) * f(cam["tan_fovx"])
    ry = ((2 * np.arange(H) + 1).astype(f) / f(H) - f(1)) * f(cam["tan_fovy"])
    return rx, ry


def frames(z, cam, dtype=np.float64):
    """P, a, b, N, |N|^2 of every pixel from z (H, W; NaN where not defined), in `dtype`; NaN wherever a neighbour is missing."""
    rx, ry = rays(cam, dtype)
    z = z.astype(dtype)
    P = np.stack([z * rx[None, :], z * ry[:, None], z], -1)
    a = _shift(P, 1, 0) - _shift(P, -1, 0)
    b = _shift(P, 0, 1) - _shift(P, 0, -1)
    N = _cross(a, b)
    return P, a, b, N, _dot(N, N)


def decide(Dinv, final_T, cam, alpha_min=ALPHA_MIN):
    """The header's float32 decisions: A (float32), defined, valid (bool), z (float32, NaN where not defined)."""
    f = np.float32
    D, T = np.asarray(Dinv, f), np.asarray(final_T, f)
    with np.errstate(all="ignore"):
        A = f(1) - T
        defined = np.isfinite(A) & np.isfinite(D) & (A >= f(alpha_min)) & (D > 0)
        z = np.where(defined, A / np.where(defined, D, f(1)), f(np.nan)).astype(f)
        _, a, b, N, nn = frames(z, cam, f)
        five = defined & _shift(defined, 1, 0, False) & _shift(defined, -1, 0, False) & _shift(defined, 0, 1, False) & _shift(defined, 0, -1, False)
        valid = five & (nn > MIN_NORM2 * (_dot(a, a) * _dot(b, b))) & (nn <= FLT_MAX)
    return {"A": A, "defined": defined, "valid": valid, "z": z}


def normals_from_z(z, cam):
    """Float64 unit normals (H, W, 3) of a float64 depth image z (NaN: not defined), NaN where a neighbour is missing."""
    _, _, _, N, nn = frames(np.asarray(z, np.float64), cam)
    with np.errstate(all="ignore"):
        return N / np.sqrt(nn)[..., None]


def target_unit(target, R, dtype=np.float64):
    """(t^ (H, W, 3) in `dtype`, t_ok): the rotated, normalised target; t_ok is the header's float32 decision."""
    f = np.float32
    Rm = np.eye(3, dtype=f) if R is None else np.asarray(R, f).reshape(3, 3)

    def rot(d):
        t, M = np.asarray(target, f).astype(d), Rm.astype(d)
        return np.stack([(M[i, 0] * t[..., 0] + M[i, 1] * t[..., 1]) + M[i, 2] * t[..., 2] for i in range(3)], -1)
    with np.errstate(all="ignore"):
        s32 = rot(f)
        ss32 = _dot(s32, s32)
        t_ok = (ss32 > 0) & (ss32 <= FLT_MAX)
        s = rot(dtype)
        th = s / np.sqrt(_dot(s, s))[..., None]
    return np.where(t_ok[..., None], th, dtype(0)), t_ok


def gather(Dinv, dec, cam, g, dtype):
    """The header's gather in `dtype`: (normals, gD, gA) for dL/dn = g (H, W, 3; rows of pixels that are not valid ignored)."""
    f = dtype
    valid, defined = dec["valid"], dec["defined"]
    z = np.where(defined, dec["A"].astype(f) / np.where(defined, np.asarray(Dinv, np.float32), 1).astype(f), f(np.nan)).astype(f)
    with np.errstate(all="ignore"):
        P, a, b, N, nn = frames(z, cam, f)
        ln = np.sqrt(nn)
        n = np.where(valid[..., None], N / ln[..., None], f(0))
        g = np.where(valid[..., None], np.asarray(g).astype(f), f(0))
        ng = _dot(n, g)
        u = (g - n * ng[..., None]) / ln[..., None]
        c1 = np.where(valid[..., None], _cross(b, u), f(0))
        c2 = np.where(valid[..., None], _cross(u, a), f(0))
        gP = ((_shift(c1, -1, 0, 0) - _shift(c1, 1, 0, 0)) + _shift(c2, 0, -1, 0)) - _shift(c2, 0, 1, 0)
        rx, ry = rays(cam, f)
        gz = (rx[None, :] * gP[..., 0] + ry[:, None] * gP[..., 1]) + gP[..., 2]
        D = np.asarray(Dinv, np.float32).astype(f)
        gD = np.where(defined, gz * (-z / D), f(0)) + f(0)
        gA = np.where(defined, gz * (f(1) / D), f(0)) + f(0)
    return n.astype(f), gD.astype(f), gA.astype(f), P, a, b


def loss_direction(case, dtype=np.float64):
    """(g, th, ok): dL/dn = -(weight m) t^ of the fused loss in `dtype`, and the pixels that count (valid normal, usable target)."""
    th, t_ok = target_unit(case["target"], case["R"], dtype)
    ok = case["dec"]["valid"] & t_ok
    m = np.ones(ok.shape, dtype) if case["mask"] is None else np.asarray(case["mask"], np.float32).astype(dtype)
    g = np.where(ok[..., None], (-(dtype(case["weight32"]) * m))[..., None] * th, dtype(0))
    return g, th, ok, m


def _loss(case, dtype):
    g, th, ok, m = loss_direction(case, dtype)
    n, gD, gA, *_ = gather(case["Dinv"], case["dec"], case["cam"], g, dtype)
    terms = np.where(ok, m.astype(np.float64) * (1.0 - _dot(n.astype(np.float64), th.astype(np.float64))), 0.0)
    return {"normals": n, "valid": case["dec"]["valid"], "sums": (float(terms.sum()), float(np.where(ok, m, 0).astype(np.float64).sum())),
            "gD": gD, "gA": gA}


def closed_form(case):
    """The fused loss by the header's gather, float64."""
    return _loss(case, np.float64)


def restatement32(case):
    """The fused loss by the header's formulas in numpy float32 (the sums in float64 of the float32 terms, as the header has them)."""
    return _loss(case, np.float32)


def closed_form_vjp(case, g, dtype=np.float64):
    """(gD, gA) of an arbitrary dL/dn by the header's gather."""
    return gather(case["Dinv"], case["dec"], case["cam"], g, dtype)[1:3]


def torch_normals(D, A, dec, cam):
    """Float64 torch: unit normals (H, W, 3) differentiable in D and A, zeros where not valid."""
    F = torch.nn.functional
    defined, valid = torch.as_tensor(dec["defined"]), torch.as_tensor(dec["valid"])
    rx, ry = (torch.as_tensor(r) for r in rays(cam))
    z = torch.where(defined, A / torch.where(defined, D, torch.ones_like(D)), torch.zeros_like(D))
    P = torch.stack([z * rx[None, :], z * ry[:, None], z], 0)                     # (3, H, W)
    Pp = F.pad(P, (1, 1, 1, 1))
    a = Pp[:, 2:, 1:-1] - Pp[:, :-2, 1:-1]
    b = Pp[:, 1:-1, 2:] - Pp[:, 1:-1, :-2]
    N = torch.linalg.cross(a, b, dim=0)
    N = torch.where(valid[None], N, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)[:, None, None])
    return torch.where(valid[None], N / N.norm(dim=0, keepdim=True), torch.zeros_like(N)).permute(1, 2, 0)


def autograd_vjp(case, g):
    """(normals, gD, gA): d(sum g . n)/d(Dinv, A) by torch autograd in float64."""
    D = torch.tensor(np.asarray(case["Dinv"], np.float64), requires_grad=True)
    A = torch.tensor(case["dec"]["A"].astype(np.float64), requires_grad=True)
    n = torch_normals(D, A, case["dec"], case["cam"])
    gD, gA = torch.autograd.grad((n * torch.as_tensor(np.asarray(g, np.float64))).sum(), (D, A))
    return n.detach().numpy(), gD.numpy(), gA.numpy()


def reference(case):
    """The fused loss in float64: normals, valid, sums = (loss_sum, weight_sum), gD and gA = weight32 d loss_sum / d(Dinv, A) by autograd."""
    th, t_ok = target_unit(case["target"], case["R"])
    ok = case["dec"]["valid"] & t_ok
    m = np.ones(ok.shape) if case["mask"] is None else np.asarray(case["mask"], np.float64)
    D = torch.tensor(np.asarray(case["Dinv"], np.float64), requires_grad=True)
    A = torch.tensor(case["dec"]["A"].astype(np.float64), requires_grad=True)
    n = torch_normals(D, A, case["dec"], case["cam"])
    terms = torch.as_tensor(np.where(ok, m, 0.0)) * (1.0 - (n * torch.as_tensor(th)).sum(-1))
    loss_sum = terms.sum()
    if ok.any():
        gD, gA = torch.autograd.grad(case["weight32"] * loss_sum, (D, A))
        gD, gA = gD.numpy(), gA.numpy()
    else:
        gD, gA = np.zeros(ok.shape), np.zeros(ok.shape)
    return {"normals": n.detach().numpy(), "valid": case["dec"]["valid"], "sums": (float(loss_sum.detach()), float(np.where(ok, m, 0.0).sum())), "gD": gD, "gA": gA}


def kappa(case):
    """The cancellation factor of a case (0 without a valid pixel)."""
    dec = case["dec"]
    if not dec["valid"].any():
        return 0.0
    with np.errstate(all="ignore"):
        P, a, b, _, _ = frames(dec["z"].astype(np.float64), case["cam"])
        k = np.sqrt(_dot(P, P)) / np.minimum(np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)))
    return float(k[dec["valid"]].max())


def error_ratios(got, ref, kap):
    """{"normals", "gD", "gA", "sums"}: the errors of `got` against `ref` in the units of the module docstring."""
    out = {"normals": 0.0, "gD": 0.0, "gA": 0.0, "sums": 0.0}
    if kap > 0:
        out["normals"] = float(np.abs(np.asarray(got["normals"], np.float64) - ref["normals"]).max()) / (EPS32 * kap)
        for k in ("gD", "gA"):
            if got.get(k) is not None and np.abs(ref[k]).max() > 0:
                out[k] = float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()) / (EPS32 * kap * float(np.abs(ref[k]).max()))
    for s, r in zip(got["sums"], ref["sums"]):
        if r != 0:
            out["sums"] = max(out["sums"], abs(float(np.float32(s)) - r) / abs(r) / EPS32)
    return out


# ------------------------------------------------------------------------------------------------------------------- the cases
def plane_depth(cam, n0=(0.3, -0.2, -0.93), d=-3.0):
    """z (H, W) float64 of the plane n0 . P = d under the camera's rays, and the unit normal facing the camera."""
    n0 = np.asarray(n0, np.float64) / np.linalg.norm(n0)
    rx, ry = rays(cam)
    return d / (n0[0] * rx[None, :] + n0[1] * ry[:, None] + n0[2]), n0


def wavy_depth(cam, rng, noise=0.01):
    W, H = cam["width"], cam["height"]
    x, y = np.meshgrid(np.arange(W) / max(W, 8), np.arange(H) / max(H, 8))
    z = 3.0 + 0.4 * np.sin(5.0 * x + 1.0) * np.cos(4.0 * y) + 0.3 * x - 0.2 * y
    return z * (1.0 + noise * rng.uniform(-1, 1, (H, W)))


def _case(name, W, H, z, rng, *, holes=None, mask=False, rot=False, want_grad=True, degenerate=False, finite_only=False, Dinv=None, final_T=None):
    cam = camera(W, H, 0.5 if W >= H else 0.5 * W / H)
    T = rng.uniform(0.0, 0.3, (H, W)).astype(np.float32) if final_T is None else final_T
    if holes is not None:
        T = np.where(holes, np.float32(0.8), T).astype(np.float32)             # A = 0.2 < alpha_min
    if Dinv is None:
        Dinv = ((np.float32(1) - T).astype(np.float64) / z).astype(np.float32)
    dec = decide(Dinv, T, cam)
    # the target: the surface's own normal turned by up to ~25 degrees, of any length; a few zero vectors (not valid for the loss)
    with np.errstate(all="ignore"):
        n = np.nan_to_num(normals_from_z(np.where(dec["defined"], dec["z"], np.nan).astype(np.float64), cam), nan=0.0, posinf=0.0, neginf=0.0)
    t = n + 0.3 * rng.normal(0, 1, (H, W, 3))
    t = t * rng.uniform(0.5, 2.0, (H, W, 1))
    t[rng.uniform(0, 1, (H, W)) < 0.02] = 0.0
    R = None
    if rot:                                                                    # a rotation about a skew axis: the target is stored turned back
        ax = np.array([0.3, 0.8, -0.5]) / np.linalg.norm([0.3, 0.8, -0.5])
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K).astype(np.float32)
        t = t @ R.astype(np.float64)                                           # rows R^T t: R turns them back
    m = rng.uniform(0.0, 2.0, (H, W)).astype(np.float32) if mask else None
    if m is not None:
        m[rng.uniform(0, 1, (H, W)) < 0.1] = 0.0
    weight = 0.7
    return {"name": name, "W": W, "H": H, "cam": cam, "Dinv": Dinv, "final_T": T, "target": t.astype(np.float32), "R": R, "mask": m,
            "weight": weight, "weight32": float(np.float32(weight / (W * H))), "want_grad": want_grad, "degenerate": degenerate,
            "finite_only": finite_only, "dec": dec}


def border_holes(W, H, rng, tile_w, tile_h):
    """5 % of the pixels: 2 % anywhere, 3 % on the first and last columns and rows of the kernel's tiles (a tenth of those pixels)."""
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    border = (x % tile_w == 0) | (x % tile_w == tile_w - 1) | (y % tile_h == 0) | (y % tile_h == tile_h - 1)
    u = rng.uniform(0, 1, (H, W))
    return (u < 0.02) | (border & (u > 0.9))


def all_cases(tile_w, tile_h, max_blocks):
    """The case matrix of tests/test_gpu_normals.py.  Every case that is not degenerate has a valid normal at no less than half of
    its interior pixels (the (W - 2)(H - 2) that have four neighbours), asserted here so that no test passes on an empty set."""
    rng = np.random.default_rng(11)
    sizes = [(1, 1), (2, 2), (3, 1), (3, 3), (37, 29), (tile_w - 1, tile_h - 1), (tile_w, tile_h), (tile_w + 1, tile_h + 1),
             (2 * tile_w + 1, 2 * tile_h + 1), (130, 70),
             (17 * tile_w - 14, 16 * tile_h - 7),           # 272 tiles: more records than the finishing walk's 256 threads
             (33 * tile_w - 15, 63 * tile_h - 7)]           # 2079 tiles > max_blocks: a workgroup takes more than one tile
    assert 256 < 17 * 16 <= max_blocks < 33 * 63
    out = []
    for k, (W, H) in enumerate(sizes):
        cam = camera(W, H, 0.5 if W >= H else 0.5 * W / H)
        out.append(_case(f"wavy_{W}x{H}", W, H, wavy_depth(cam, rng), rng, mask=k % 2 == 0, rot=k % 3 == 0, want_grad=k % 4 != 3,
                         degenerate=W < 3 or H < 3))
    for W, H in ((37, 29), (130, 70)):
        cam = camera(W, H)
        out.append(_case(f"plane_{W}x{H}", W, H, plane_depth(cam)[0], rng, final_T=np.zeros((H, W), np.float32)))
        out.append(_case(f"holes_{W}x{H}", W, H, wavy_depth(cam, rng), rng, holes=border_holes(W, H, rng, tile_w, tile_h), mask=True, rot=True))
        out.append(_case(f"background_{W}x{H}", W, H, None, rng, degenerate=True, Dinv=np.zeros((H, W), np.float32), final_T=np.ones((H, W), np.float32)))
        out.append(_case(f"decades_{W}x{H}", W, H, None, rng, finite_only=True, Dinv=(10.0 ** rng.uniform(-3, 3, (H, W))).astype(np.float32)))
    for c in out:
        share = c["dec"]["valid"].sum() / max(1, (c["W"] - 2) * (c["H"] - 2))
        if c["degenerate"]:
            assert not c["dec"]["valid"].any(), c["name"]
        elif not c["finite_only"]:
            assert share >= 0.5, (c["name"], share)
    return out
