"""
Loss step between forward and backward: the reference's `l1_loss` and
`compute_image_gradients` (reference loss.py:148-176, :217-244) on the GPU, in one pass over the image.
As in the reference, `lambda_dssim` only scales the L1 gradient there; the SSIM gradient is a TODO in the
reference (loss.py:243), and those two functions keep the reference's behaviour.
The standard 3DGS loss (1 - lambda) L1 + lambda (1 - SSIM) with its full pixel gradient is
`l1_dssim_loss_and_gradients` (include/gsr_loss.h).
"""
import torch

from . import _host, _lib


def l1_loss_and_gradients(rendered, target, lambda_dssim=0.0, want_grad=True, loss_out=None):
    """One kernel: returns (loss_sum device tensor [1] = sum |rendered - target|, pixel_grad (H,W,3) or None).
    mean L1 = loss_sum / (H*W*3); pixel_grad = (1-lambda_dssim)/(H*W*3) * sign(rendered - target).
    `loss_out`: a 1-element float32 device tensor (e.g. a slot of a trainer's loss curve) to receive the sum instead of a fresh one."""
    L = _lib.lib()
    dev = _host.device_of(rendered, target)
    r = _host.to_dev(rendered, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W, 3)
    t = _host.to_dev(target, torch.float32, dev, (H, W, 3))   # alpha already dropped by the caller (train.py:323-334)
    grad = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if want_grad else None
    if loss_out is not None and not (isinstance(loss_out, torch.Tensor) and loss_out.is_cuda and loss_out.dtype == torch.float32 and loss_out.numel() == 1):
        raise ValueError("l1_loss_and_gradients: loss_out must be a 1-element float32 device tensor")
    loss_sum = torch.empty(1, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    l1_weight = (1.0 - float(lambda_dssim)) / (H * W * 3.0)
    with _host.on_device(dev):
        _lib.check(L.gsr_l1_loss_grad(_host.ptr(r), _host.ptr(t), _host.ptr(grad), _host.ptr(loss_sum), W, H, l1_weight,
                                      _host.stream_ptr(dev)))
    return loss_sum, grad


def l1_loss(rendered, target):
    """Mean absolute error as a Python float (reference loss.py:148-176; synchronises, as the reference does)."""
    r = rendered
    s, _ = l1_loss_and_gradients(rendered, target, want_grad=False)
    return float(s.item()) / (int(r.shape[0]) * int(r.shape[1]) * 3)


def compute_image_gradients(rendered, target, lambda_dssim=0.2):
    """dL/dpixels for backward() (reference loss.py:217-244)."""
    return l1_loss_and_gradients(rendered, target, lambda_dssim)[1]


_DSSIM_WS = {}   # (device, stream, W, H) -> workspace of gsr_l1_dssim_loss_grad (one per stream: views in flight on several streams)


def _slot(t, name):
    if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
        raise ValueError(f"l1_dssim_loss_and_gradients: {name} must be a 1-element float32 device tensor")
    return t


def l1_dssim_loss_and_gradients(rendered, target, lambda_dssim=0.2, window="gaussian", want_grad=True, loss_out=None, ssim_out=None):
    """L = (1 - lambda) L1 + lambda (1 - SSIM) in one call (include/gsr_loss.h), with no host sync.
    Returns (l1_sum, ssim_sum, pixel_grad): device tensors [1] with l1_sum = sum |rendered - target| (mean L1 = l1_sum / (3HW))
    and ssim_sum = sum over pixels of the channel-mean SSIM (SSIM = ssim_sum / (HW)), and pixel_grad = dL/drendered (H, W, 3),
    or None without want_grad.  window: "gaussian" (centred sigma = 1.5, standard 3DGS) or "reference" (gsr_ssim's weights),
    both clipped to the image and renormalised at the border.  `loss_out` / `ssim_out`: 1-element float32 device tensors (e.g.
    slots of a trainer's curves) that receive the sums instead of fresh ones."""
    if window not in _lib.SSIM_WINDOWS:
        raise ValueError(f"window must be one of {sorted(_lib.SSIM_WINDOWS)}, not {window!r}")
    lam = float(lambda_dssim)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1], not {lambda_dssim}")
    _slot(loss_out, "loss_out")
    _slot(ssim_out, "ssim_out")
    L = _lib.lib()
    dev = _host.device_of(rendered, target)
    r = _host.to_dev(rendered, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W, 3)
    t = _host.to_dev(target, torch.float32, dev, (H, W, 3))
    grad = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if want_grad else None
    l1_sum = torch.empty(1, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    ssim_sum = torch.empty(1, dtype=torch.float32, device=dev) if ssim_out is None else ssim_out
    with _host.on_device(dev):
        stream = _host.stream_ptr(dev)
        key = (dev, stream, W, H)
        ws = _DSSIM_WS.get(key)
        if ws is None:
            ws = _DSSIM_WS[key] = torch.empty(max(16, int(L.gsr_dssim_workspace_bytes(W, H))), dtype=torch.uint8, device=dev)
        _lib.check(L.gsr_l1_dssim_loss_grad(_host.ptr(r), _host.ptr(t), _host.ptr(grad), _host.ptr(l1_sum), _host.ptr(ssim_sum), W, H,
                                            lam, _lib.SSIM_WINDOWS[window], _host.ptr(ws), ws.numel(), stream))
    return l1_sum, ssim_sum, grad


def ssim(rendered, target, window="reference"):
    """Mean SSIM as a Python float (reference loss.py:178-215: 11x11 window, sigma 1.5, weights indexed by distance as the
    reference does -- see gsr.h).  An evaluation helper: the reference's training loop has its SSIM term commented out.
    window="gaussian": the centred sigma = 1.5 window standard 3DGS trains with (gsr_loss.h), through l1_dssim_loss_and_gradients."""
    if window != "reference":
        r = rendered
        _, s, _ = l1_dssim_loss_and_gradients(rendered, target, 0.0, window=window, want_grad=False)
        return float(s.item()) / (int(r.shape[0]) * int(r.shape[1]))
    L = _lib.lib()
    dev = _host.device_of(rendered, target)
    r = _host.to_dev(rendered, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W, 3)
    t = _host.to_dev(target, torch.float32, dev, (H, W, 3))
    acc = torch.empty(1, dtype=torch.float32, device=dev)
    with _host.on_device(dev):
        _lib.check(L.gsr_ssim(_host.ptr(r), _host.ptr(t), _host.ptr(acc), W, H, _host.stream_ptr(dev)))
    return float(acc.item()) / (W * H)


def depth_loss(rendered_depth, target_depth, depth_mask):
    """Masked mean L1 between inverse-depth images as a Python float (reference loss.py:271-303)."""
    L = _lib.lib()
    dev = _host.device_of(rendered_depth, target_depth, depth_mask)
    r = _host.to_dev(rendered_depth, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W)
    t = _host.to_dev(target_depth, torch.float32, dev, (H, W))
    m = _host.to_dev(depth_mask, torch.float32, dev, (H, W))
    acc = torch.empty(1, dtype=torch.float32, device=dev)
    with _host.on_device(dev):
        _lib.check(L.gsr_depth_loss(_host.ptr(r), _host.ptr(t), _host.ptr(m), _host.ptr(acc), W, H, _host.stream_ptr(dev)))
    return float(acc.item()) / (W * H)


def _aux_l1(entry, rendered, target, mask, weight, want_grad, loss_out):
    L = _lib.lib()
    dev = _host.device_of(rendered, target, mask)
    r = _host.to_dev(rendered, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W)
    t = _host.to_dev(target, torch.float32, dev, (H, W))
    m = _host.to_dev(mask, torch.float32, dev, (H, W)) if mask is not None else None
    _slot(loss_out, "loss_out")
    grad = torch.empty((H, W), dtype=torch.float32, device=dev) if want_grad else None
    loss_sum = torch.empty(1, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    with _host.on_device(dev):
        _lib.check(getattr(L, entry)(_host.ptr(r), _host.ptr(t), _host.ptr(m), _host.ptr(grad), _host.ptr(loss_sum), W, H,
                                     float(weight) / (W * H), _host.stream_ptr(dev)))
    return loss_sum, grad


def depth_loss_and_gradients(rendered, target, mask, weight=1.0, want_grad=True, loss_out=None):
    """Masked L1 between inverse-depth images and its gradient, one kernel, no host sync (include/gsr_aux_grads.h).
    Returns (loss_sum device tensor [1] = sum |rendered - target| * mask, grad (H, W) or None) with
    grad = weight / (W H) * mask * sign(rendered - target): the gradient of weight * loss_sum / (W H), the reference's depth_loss
    normalisation (loss.py:271-303).  mask may be None (all ones).  The gradient goes to backward(dL_ddepth_image=...)."""
    return _aux_l1("gsr_depth_loss_grad", rendered, target, mask, weight, want_grad, loss_out)


def alpha_loss_and_gradients(final_Ts, target_alpha, mask=None, weight=1.0, want_grad=True, loss_out=None):
    """Masked L1 between the alpha image 1 - final_Ts and target_alpha, and its gradient with respect to the alpha image, as
    depth_loss_and_gradients (normalised by W H).  final_Ts is the forward's img_buffer["final_Ts"]; the gradient goes to
    backward(dL_dalpha_image=...)."""
    return _aux_l1("gsr_alpha_loss_grad", final_Ts, target_alpha, mask, weight, want_grad, loss_out)
