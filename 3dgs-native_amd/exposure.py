"""
Per-view exposure compensation (include/gsr_exposure.h) over the MI355X library: a learned affine colour transform per training
image, applied to the render before the loss -- the photometric twin of pose refinement.  Auto-exposure and white balance differ
from photo to photo; without this stage 3DGS explains them with view-dependent floaters.

    E = (12,) float32, row-major (4, 3): rows 0-2 are A, row 3 is b;   c' = c @ A + b per pixel, no clamp;   identity: A = I, b = 0

    img1 = apply_exposure(img, E_v)                            # (H, W, 3)
    dpix, dE = exposure_backward(img, E_v, dpix1, out=dpix1)   # dL/dimg (here in place on dpix1) and dL/dE_v (12,)

The training step with a model = ExposureModel(num_views, device), for view v (examples/train.py --optimize-exposure):

    img, depth, buf = render_gaussians(...)
    img1 = apply_exposure(img, model.matrix(v))
    loss, dpix1 = l1_loss_and_gradients(img1, target_v)        # any loss of loss.py: it sees the corrected image
    dpix, dE = exposure_backward(img, model.matrix(v), dpix1, out=dpix1)
    grads = backward(dL_dpixels=dpix, ...)
    model.step(v, dE, lr)                                      # one Adam step on the 12 numbers of view v, on the device

Nothing here waits on the device, and render_gaussians / backward know nothing of it: it is an image-space stage beside loss.py.
Held-out views have no matrix: they are scored with the identity, i.e. not passed through this module at all.
"""
import numpy as np
import torch

from . import _args, _host, _lib

NE = _lib.EXPOSURE_FLOATS
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15       # 3DGS's exposure optimizer


def _check_E(E, name="E"):
    if not isinstance(E, (torch.Tensor, np.ndarray)):
        raise ValueError(f"{name} must be a torch tensor or a numpy array of {NE} float32 (got {type(E).__name__})")
    if int(np.prod(tuple(E.shape))) != NE:
        raise ValueError(f"{name} must have {NE} elements, row-major (4, 3): A then b (got shape {tuple(E.shape)})")
    if not _args.is_f32(E):
        raise ValueError(f"{name} must be float32 (got {E.dtype})")


def _row(E, dev):
    """E as the library takes it: 12 packed float32 on `dev`, 4-byte aligned -- a row of a (V, 12) tensor goes through as it is."""
    if isinstance(E, torch.Tensor) and E.is_cuda and E.device == dev and E.is_contiguous():
        return E
    return torch.as_tensor(np.ascontiguousarray(E.detach().cpu().numpy() if isinstance(E, torch.Tensor) else E, np.float32).reshape(NE)).to(dev)


def apply_exposure(image, E, out=None):
    """The corrected image c' = c @ A + b, (H, W, 3) float32 on the device (gsr_exposure_apply), as a new tensor or into `out`, which
    may be `image` itself.  With E = identity the result is the input bit for bit (-0 comes back +0)."""
    shape = _args.image_hw(image, "image", channels=3, f32=True) + (3,)
    _check_E(E)
    if out is not None:
        _args.check_out(out, shape, "out")
    _args.check_one_device(image, E, out)
    L = _lib.lib()
    dev = _host.device_of(image, E, out)
    r = _host.to_dev(image, torch.float32, dev, shape)
    e = _row(E, dev)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    with _host.on_device(dev):
        _lib.check(L.gsr_exposure_apply(_host.ptr(r), _host.ptr(e), _host.ptr(out), shape[1], shape[0], _host.raw_stream(dev)))
    _host.written_in_place(out)
    return out


def exposure_backward(image, E, dL_dout, out=None, want_image_grad=True, dE_out=None):
    """(dL_dimage, dL_dE) from dL_dout = dL/d(corrected image) (gsr_exposure_backward): dL_dimage (H, W, 3) is a new tensor, or
    `out` -- in place on dL_dout when `out is dL_dout` -- or None with want_image_grad=False; dL_dE is (12,) float32 in E's layout, a
    new tensor or `dE_out`.  `image` is the UNcorrected render.  The sums use no atomics: the same inputs give the same bits."""
    shape = _args.image_hw(image, "image", channels=3, f32=True) + (3,)
    _check_E(E)
    _args.image_hw(dL_dout, "dL_dout", shape[:2], 3, f32=True)
    if out is not None:
        if not want_image_grad:
            raise ValueError("out was given with want_image_grad=False")
        _args.check_out(out, shape, "out")
    _args.check_slot(dE_out, NE, "dE_out", contiguous=True)
    _args.check_one_device(image, E, dL_dout, out, dE_out)
    L = _lib.lib()
    dev = _host.device_of(image, E, dL_dout, out)
    r = _host.to_dev(image, torch.float32, dev, shape)
    e = _row(E, dev)
    g = _host.to_dev(dL_dout, torch.float32, dev, shape)
    if want_image_grad and out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    dE = torch.empty(NE, dtype=torch.float32, device=dev) if dE_out is None else dE_out
    stream = _host.raw_stream(dev)
    with _host.on_device(dev):
        ws = _host.workspace("exposure", L.gsr_exposure_workspace_bytes(shape[1], shape[0]), dev, stream)
        _lib.check(L.gsr_exposure_backward(_host.ptr(r), _host.ptr(e), _host.ptr(g), _host.ptr(out), _host.ptr(dE), shape[1], shape[0],
                                           _host.ptr(ws), ws.numel(), stream))
    _host.written_in_place(out, dE)
    return out, dE


class ExposureModel:
    """One E per training view with its Adam state: `E`, `m`, `v` are (V, 12) float32 device tensors (identity, zeros, zeros), `steps`
    the host-side step count of every view (a view's bias correction follows its own count: a step touches one view)."""

    def __init__(self, num_views, device):
        if int(num_views) < 1:
            raise ValueError(f"num_views must be >= 1 (got {num_views})")
        self.num_views, self.device = int(num_views), torch.device(device)
        self.E = torch.tensor(IDENTITY, dtype=torch.float32).repeat(self.num_views, 1).to(self.device)
        self.m, self.v = torch.zeros_like(self.E), torch.zeros_like(self.E)
        self.steps = [0] * self.num_views
        self._rows = [tuple(t.data_ptr() + 4 * NE * k for t in (self.E, self.m, self.v)) for k in range(self.num_views)]   # the step marshals no views

    def matrix(self, v):
        """Row v of E, (12,): a view, so a step is seen by the next call."""
        return self.E[v]

    def step(self, v, dL_dE, lr):
        """One Adam step (beta 0.9 / 0.999, eps 1e-15) on row v: one single-wave launch, no host wait."""
        _check_E(dL_dE, "dL_dE")
        lr = float(lr)
        if not (lr >= 0.0 and np.isfinite(lr)):
            raise ValueError(f"lr must be >= 0 and finite (got {lr})")
        L = _lib.lib()
        g = _row(dL_dE, self.device)
        with _host.on_device(self.device):
            e_ptr, m_ptr, v_ptr = self._rows[v]
            _lib.check(L.gsr_exposure_adam(e_ptr, _host.ptr(g), m_ptr, v_ptr, lr, BETA1, BETA2, EPS, self.steps[v] + 1, _host.raw_stream(self.device)))
        self.steps[v] += 1
        _host.written_in_place(self.E, self.m, self.v)

    def state_dict(self):
        """A JSON-able dict of lists (reads the three tensors back: for checkpoints, not for the step)."""
        return {"num_views": self.num_views, "layout": "row-major (4, 3): A rows 0-2, b row 3; c' = c @ A + b",
                "E": self.E.cpu().tolist(), "m": self.m.cpu().tolist(), "v": self.v.cpu().tolist(), "steps": list(self.steps)}

    def load_state_dict(self, state):
        rows = {k: np.asarray(state[k], np.float32) for k in ("E", "m", "v")}
        steps = [int(s) for s in state["steps"]]
        if any(a.shape != (self.num_views, NE) for a in rows.values()) or len(steps) != self.num_views or min(steps) < 0:
            raise ValueError(f"state is not that of {self.num_views} views: E, m, v must be ({self.num_views}, {NE}) and steps {self.num_views} counts >= 0")
        for k, a in rows.items():
            getattr(self, k).copy_(torch.from_numpy(a))
        self.steps = steps


# ---- experiments: exposure errors to recover from (examples/train.py --exposure-noise) ----
def random_exposures(num_views, S, seed, offdiag=0.0):
    """(V, 12) float64: per view A = diag(exp(u + w)), u ~ N(0, S^2) per channel, w ~ N(0, S^2) shared by the channels (a colour cast
    and a gain), b ~ N(0, (S / 4)^2) per channel.  Deterministic per seed; S = 0 is the identity exactly.  offdiag > 0 adds +-offdiag
    (signs drawn after everything else) to the six off-diagonal entries of A."""
    S = float(S)
    if not (S >= 0.0 and np.isfinite(S)):
        raise ValueError(f"S must be >= 0 and finite (got {S})")
    rng = np.random.default_rng(int(seed))
    u, w, b = rng.normal(0.0, S, (num_views, 3)), rng.normal(0.0, S, (num_views, 1)), rng.normal(0.0, S / 4.0, (num_views, 3))
    E = np.zeros((num_views, 4, 3))
    for j in range(3):
        E[:, j, j] = np.exp(u[:, j] + w[:, 0])
    E[:, 3, :] = b + 0.0
    if offdiag:
        sign = rng.choice([-1.0, 1.0], size=(num_views, 3, 3))
        E[:, :3, :] += offdiag * sign * (1.0 - np.eye(3))
    return E.reshape(num_views, NE)


def perturbed_target(target, E_row):
    """clamp(t @ A + b, 0, 1) of an (H, W, 3) device tensor: what a camera with that exposure error would have stored.  Once per
    image at load (torch ops: not on the training step)."""
    E = torch.as_tensor(np.asarray(E_row, np.float64).reshape(4, 3), dtype=torch.float32, device=target.device)
    return (target @ E[:3] + E[3]).clamp_(0.0, 1.0).contiguous()
