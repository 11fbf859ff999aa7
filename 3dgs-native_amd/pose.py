"""
Per-view pose corrections over the camera gradients of backward(camera_grad=True) (include/gsr_camera_grads.h).

Convention (one place for it).  A camera dict (cameras.py) holds `world_to_camera` V in the row-vector form the kernels take,
p_cam = [p, 1] @ V, i.e. V = M^T with the column-form pose M = [[R, t], [0, 1]], p_cam = R p + t.  A pose correction is a 6-vector
xi = (rho, phi): rho a translation and phi an axis-angle rotation (radians), both in the CAMERA frame, applied on the left of the
pose:
    p_cam' = exp(xi^) p_cam,   exp(xi^) = [[Exp(phi), J(phi) rho], [0, 1]]    (the SE(3) exponential; J its left Jacobian)
so M' = exp(xi^) M and V' = V exp(xi^)^T.  The intrinsics stay fixed: full_proj_matrix' = V' @ proj_matrix, and camera_center'
is the translation row of V'^-1.  xi = 0 is the identity, and apply_pose_delta(cam, 0) returns the camera bit for bit.

pose_gradient composes the three partials backward() returns -- dL/dviewmatrix, dL/dprojmatrix, dL/dcampos, each taken as
independent -- into dL/dxi through V(xi), V(xi) @ proj_matrix and the camera centre, by float64 autograd on that small graph.
It assumes the render was called with viewmatrix = world_to_camera, projmatrix = full_proj_matrix and campos = camera_center of
apply_pose_delta(cam, xi), as examples/train.py does.
"""
import numpy as np
import torch

from .cameras import _world_to_view

D = torch.float64


def _hat(w):
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def se3_exp(xi):
    """4x4 column-form exp(xi^) of xi = (rho, phi), float64 torch, differentiable at xi = 0 (series below 1e-8 rad^2)."""
    xi = torch.as_tensor(xi, dtype=D)
    rho, phi = xi[:3], xi[3:]
    th2 = (phi * phi).sum()
    small = th2 < 1e-8
    safe = torch.where(small, torch.ones_like(th2), th2)
    th = torch.sqrt(safe)
    a = torch.where(small, 1.0 - th2 / 6.0 + th2 * th2 / 120.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - th2 / 24.0 + th2 * th2 / 720.0, (1.0 - torch.cos(th)) / safe)
    c = torch.where(small, 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0, (th - torch.sin(th)) / (safe * th))
    K = _hat(phi)
    I = torch.eye(3, dtype=D)
    R = I + a * K + b * (K @ K)
    J = I + b * K + c * (K @ K)
    top = torch.cat([R, (J @ rho)[:, None]], 1)
    return torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=D)], 0)


def apply_pose_delta(cam, xi):
    """The camera dict with the pose correction xi applied (module docstring): `world_to_camera`, `full_proj_matrix`,
    `camera_center` and the pose-derived `R`, `T`, `view_matrix` recomputed with cameras.nerf_camera's own expressions and dtypes;
    every other key (intrinsics, size) is shared with `cam`."""
    xi = np.asarray(xi, np.float64).reshape(6)
    V = np.asarray(cam["world_to_camera"])
    E = se3_exp(torch.as_tensor(xi)).numpy()
    Vn = (V.astype(np.float64) @ E.T).astype(V.dtype)
    out = dict(cam)
    out["world_to_camera"] = Vn
    out["full_proj_matrix"] = Vn @ cam["proj_matrix"]
    out["camera_center"] = np.linalg.inv(Vn)[3, :3]
    w2c = Vn.T
    out["R"], out["T"] = w2c[:3, :3].copy(), w2c[:3, 3].copy()
    if "view_matrix" in cam:
        out["view_matrix"] = _world_to_view(out["R"], out["T"])
    return out


def _as64(x, shape):
    if torch.is_tensor(x):
        x = x.detach().to("cpu")
    return torch.as_tensor(np.asarray(x, np.float64) if not torch.is_tensor(x) else x.to(D)).reshape(shape)


def pose_gradient(cam, xi, dL_dview, dL_dproj, dL_dcampos):
    """dL/dxi (numpy float64, 6) from the camera partials of backward(camera_grad=True) at apply_pose_delta(cam, xi)."""
    xi_t = torch.as_tensor(np.asarray(xi, np.float64).reshape(6)).requires_grad_(True)
    V0 = torch.as_tensor(np.asarray(cam["world_to_camera"], np.float64))
    P = torch.as_tensor(np.asarray(cam["proj_matrix"], np.float64))
    V = V0 @ se3_exp(xi_t).T
    centre = torch.linalg.inv(V)[3, :3]
    L = (V * _as64(dL_dview, (4, 4))).sum() + ((V @ P) * _as64(dL_dproj, (4, 4))).sum() + (centre * _as64(dL_dcampos, (3,))).sum()
    return torch.autograd.grad(L, xi_t)[0].numpy()


def pose_error(cam, ref):
    """(rotation error in degrees, camera-centre distance in scene units) of camera dict `cam` against `ref`."""
    Ra = np.asarray(cam["world_to_camera"], np.float64)[:3, :3]
    Rb = np.asarray(ref["world_to_camera"], np.float64)[:3, :3]
    c = float(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(np.asarray(cam["camera_center"], np.float64) -
                                                                  np.asarray(ref["camera_center"], np.float64)))


def random_pose_delta(rng, rot_deg, trans):
    """A xi with a rotation of exactly rot_deg degrees about a random axis and a translation of length `trans` in a random
    direction (camera frame)."""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    return np.concatenate([d * float(trans), ax * np.radians(float(rot_deg))])
