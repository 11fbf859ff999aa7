"""
Loss step between forward and backward: the reference's `l1_loss` and
`compute_image_gradients` (reference loss.py:148-176, :217-244) on the GPU, in one pass over the image.
As in the reference, `lambda_dssim` only scales the L1 gradient there; the SSIM gradient is a TODO in the
reference (loss.py:243), and those two functions keep the reference's behaviour.
The standard 3DGS loss (1 - lambda) L1 + lambda (1 - SSIM) with its full pixel gradient is
`l1_dssim_loss_and_gradients` (include/gsr_loss.h).
"""
import numpy as np
import torch

from . import _args, _host, _lib
from . import normals as _normals


def _weight_total(w):
    """The device float M = sum of the (H, W) device tensor w (gsr_weight_total: fixed order, the same bits every call)."""
    L = _lib.lib()
    H, W = int(w.shape[0]), int(w.shape[1])
    total = torch.empty(1, dtype=torch.float32, device=w.device)
    with _host.on_device(w.device):
        stream = _host.stream_ptr(w.device)
        ws = _host.workspace("sum", L.gsr_weight_total_workspace_bytes(W, H), w.device, stream)
        _lib.check(L.gsr_weight_total(_host.ptr(w), W, H, _host.ptr(total), _host.ptr(ws), ws.numel(), stream))
    return total


class PixelWeights:
    """Per-pixel weights of the colour loss (include/gsr_weighted_loss.h): `.weights`, the (H, W) float32 device tensor, and
    `.total`, their sum M as a 1-element device tensor, computed once here so that a loss call adds no launch for it.
    Weights are >= 0 and finite (0 = the pixel does not count); nothing checks that.
    dilate=r first takes the minimum over each (2r+1) x (2r+1) neighbourhood (clipped to the image), which grows the ignored
    region by r pixels.  The SSIM term reaches 5 pixels, so a region is excluded bit for bit only by a mask grown by 5."""

    def __init__(self, weights, dilate=0):
        _args.image_hw(weights, "PixelWeights: weights", squeeze=False, f32=True)     # a weight image is exactly (H, W)
        if not (isinstance(dilate, int) and dilate >= 0):
            raise ValueError(f"PixelWeights: dilate must be an integer >= 0, not {dilate!r}")
        dev = _host.device_of(weights)
        w = _host.to_dev(weights, torch.float32, dev)
        if dilate:
            w = (-torch.nn.functional.max_pool2d(-w[None, None], 2 * dilate + 1, stride=1, padding=dilate))[0, 0].contiguous()
        self.weights, self.total = w, _weight_total(w)


def _checked_weights(weights, rendered, target, who):
    """The `weights` keyword before anything touches the GPU: a PixelWeights or a bare weight image whose shape is the images' and
    which lies on their device."""
    w = weights.weights if isinstance(weights, PixelWeights) else weights
    if w is weights:
        _args.image_hw(w, f"{who}: weights", squeeze=False, f32=True)
    hw = tuple(np.shape(rendered)[:2])
    if tuple(w.shape) != hw:
        raise ValueError(f"{who}: weights have shape {tuple(w.shape)} for a {hw} image")
    for img in (rendered, target):
        if isinstance(w, torch.Tensor) and w.is_cuda and isinstance(img, torch.Tensor) and img.is_cuda and img.device != w.device:
            raise ValueError(f"{who}: weights on {w.device}, image on {img.device}")
    return weights


def _device_weights(weights, dev):
    """(weight image, total) on `dev`; a bare image's total is computed here, in the call."""
    if isinstance(weights, PixelWeights):
        return weights.weights, weights.total
    w = _host.to_dev(weights, torch.float32, dev)
    return w, _weight_total(w)


def l1_loss_and_gradients(rendered, target, lambda_dssim=0.0, want_grad=True, loss_out=None, weights=None):
    """One kernel: returns (loss_sum device tensor [1] = sum |rendered - target|, pixel_grad (H,W,3) or None).
    mean L1 = loss_sum / (H*W*3); pixel_grad = (1-lambda_dssim)/(H*W*3) * sign(rendered - target).
    `loss_out`: a 1-element float32 device tensor (e.g. a slot of a trainer's loss curve) to receive the sum instead of a fresh one.
    `weights`: a PixelWeights, or a bare (H, W) float32 weight image m whose total M is computed in the call
    (include/gsr_weighted_loss.h).  Then loss_sum = sum m |rendered - target|, mean L1 = loss_sum / (3 M) and
    pixel_grad = (1-lambda_dssim)/(3 M) * m * sign(rendered - target); the sum is reduced in a fixed order."""
    if weights is not None:
        _checked_weights(weights, rendered, target, "l1_loss_and_gradients")
    L = _lib.lib()
    dev = _host.device_of(rendered, target)
    r = _host.to_dev(rendered, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W, 3)
    t = _host.to_dev(target, torch.float32, dev, (H, W, 3))   # alpha already dropped by the caller (train.py:323-334)
    grad = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if want_grad else None
    _args.check_slot(loss_out, 1, "l1_loss_and_gradients: loss_out")
    loss_sum = torch.empty(1, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    if weights is not None:
        m, total = _device_weights(weights, dev)
        with _host.on_device(dev):
            stream = _host.stream_ptr(dev)
            ws = _host.workspace("sum", L.gsr_weight_total_workspace_bytes(W, H), dev, stream)
            _lib.check(L.gsr_weighted_l1_loss_grad(_host.ptr(r), _host.ptr(t), _host.ptr(m), _host.ptr(total), _host.ptr(grad), _host.ptr(loss_sum),
                                                   W, H, 1.0 - float(lambda_dssim), _host.ptr(ws), ws.numel(), stream))
        return loss_sum, grad
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


def l1_dssim_loss_and_gradients(rendered, target, lambda_dssim=0.2, window="gaussian", want_grad=True, loss_out=None, ssim_out=None,
                                weights=None):
    """L = (1 - lambda) L1 + lambda (1 - SSIM) in one call (include/gsr_loss.h), with no host sync.
    Returns (l1_sum, ssim_sum, pixel_grad): device tensors [1] with l1_sum = sum |rendered - target| (mean L1 = l1_sum / (3HW))
    and ssim_sum = sum over pixels of the channel-mean SSIM (SSIM = ssim_sum / (HW)), and pixel_grad = dL/drendered (H, W, 3),
    or None without want_grad.  window: "gaussian" (centred sigma = 1.5, standard 3DGS) or "reference" (gsr_ssim's weights),
    both clipped to the image and renormalised at the border.  `loss_out` / `ssim_out`: 1-element float32 device tensors (e.g.
    slots of a trainer's curves) that receive the sums instead of fresh ones.
    `weights`: a PixelWeights, or a bare (H, W) float32 weight image m whose total M is computed in the call
    (include/gsr_weighted_loss.h).  The same tuple comes back, of the weighted loss: l1_sum = sum m |rendered - target| (mean L1 =
    l1_sum / (3 M)), ssim_sum = sum of m times the channel-mean SSIM (SSIM = ssim_sum / M)."""
    if window not in _lib.SSIM_WINDOWS:
        raise ValueError(f"window must be one of {sorted(_lib.SSIM_WINDOWS)}, not {window!r}")
    lam = float(lambda_dssim)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1], not {lambda_dssim}")
    _args.check_slot(loss_out, 1, "l1_dssim_loss_and_gradients: loss_out")
    _args.check_slot(ssim_out, 1, "l1_dssim_loss_and_gradients: ssim_out")
    if weights is not None:
        _checked_weights(weights, rendered, target, "l1_dssim_loss_and_gradients")
    L = _lib.lib()
    dev = _host.device_of(rendered, target)
    r = _host.to_dev(rendered, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W, 3)
    t = _host.to_dev(target, torch.float32, dev, (H, W, 3))
    grad = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if want_grad else None
    l1_sum = torch.empty(1, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    ssim_sum = torch.empty(1, dtype=torch.float32, device=dev) if ssim_out is None else ssim_out
    if weights is not None:
        m, total = _device_weights(weights, dev)
        with _host.on_device(dev):
            stream = _host.stream_ptr(dev)
            ws = _host.workspace("weighted_dssim", L.gsr_weighted_dssim_workspace_bytes(W, H), dev, stream)
            _lib.check(L.gsr_weighted_l1_dssim_loss_grad(_host.ptr(r), _host.ptr(t), _host.ptr(m), _host.ptr(total), _host.ptr(grad),
                                                         _host.ptr(l1_sum), _host.ptr(ssim_sum), W, H, lam, _lib.SSIM_WINDOWS[window],
                                                         _host.ptr(ws), ws.numel(), stream))
        return l1_sum, ssim_sum, grad
    with _host.on_device(dev):
        stream = _host.stream_ptr(dev)
        ws = _host.workspace("dssim", L.gsr_dssim_workspace_bytes(W, H), dev, stream)
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


def _aux_l1(entry, who, rendered, target, mask, weight, want_grad, loss_out):
    L = _lib.lib()
    dev = _host.device_of(rendered, target, mask)
    r = _host.to_dev(rendered, torch.float32, dev)
    H, W = int(r.shape[0]), int(r.shape[1])
    r = r.reshape(H, W)
    t = _host.to_dev(target, torch.float32, dev, (H, W))
    m = _host.to_dev(mask, torch.float32, dev, (H, W)) if mask is not None else None
    _args.check_slot(loss_out, 1, f"{who}: loss_out")
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
    return _aux_l1("gsr_depth_loss_grad", "depth_loss_and_gradients", rendered, target, mask, weight, want_grad, loss_out)


def alpha_loss_and_gradients(final_Ts, target_alpha, mask=None, weight=1.0, want_grad=True, loss_out=None):
    """Masked L1 between the alpha image 1 - final_Ts and target_alpha, and its gradient with respect to the alpha image, as
    depth_loss_and_gradients (normalised by W H).  final_Ts is the forward's img_buffer["final_Ts"]; the gradient goes to
    backward(dL_dalpha_image=...)."""
    return _aux_l1("gsr_alpha_loss_grad", "alpha_loss_and_gradients", final_Ts, target_alpha, mask, weight, want_grad, loss_out)


def distortion_loss_and_gradients(dist, mask=None, weight=1.0):
    """The depth-distortion term of distortion.render_distortion()'s image (include/gsr_distortion.h), normalised by W H:
    (loss, g) with loss = weight * sum(mask * dist) / (W H), a device tensor [1] for the log, and g = weight * mask / (W H), (H, W):
    the gradient with respect to `dist`, which goes to backward(dL_ddistortion=g, distortion_moments=...).  mask may be None (all
    ones).  Plain torch: two elementwise launches, no host sync."""
    if not (_args.is_dev(dist, torch.float32) and dist.dim() == 2 and dist.numel() > 0):
        raise ValueError("distortion_loss_and_gradients: dist must be a float32 device tensor of shape (H, W)")
    w = _args.finite(weight, "distortion_loss_and_gradients: weight")
    H, W = int(dist.shape[0]), int(dist.shape[1])
    if mask is None:
        g = torch.full((H, W), w / (W * H), dtype=torch.float32, device=dist.device)
    else:
        if not (isinstance(mask, (torch.Tensor, np.ndarray)) and tuple(np.shape(mask)) == (H, W)):
            raise ValueError(f"distortion_loss_and_gradients: mask must have shape {(H, W)} (the image's shape)")
        g = _host.to_dev(mask, torch.float32, dist.device, (H, W)) * (w / (W * H))
    return (g * dist).sum().reshape(1), g


def depth_corr_loss_and_gradients(rendered, target, mask=None, weight=1.0, want_grad=True, loss_out=None, fit_out=None):
    """1 - Pearson correlation between the rendered inverse depth and a relative depth target, with its exact gradient, three
    launches, no host sync (include/gsr_depth_corr.h).  A relative target is one known only up to t -> a t + b per image (a > 0), as
    a monocular depth network gives it: the loss and the gradient do not change under that map.
    Returns (loss, grad, fit): loss a device tensor [1] = 1 - rho, rho the correlation under the weights `mask` (None: all ones);
    grad (H, W) = weight * dloss/drendered, or None without want_grad; fit a device tensor [4] = (rho, s, b, M) with
    rendered ~ s * target + b in the least-squares sense and M the weight total.  A frame without variance (M = 0, a constant
    render or target) gives loss 1, a zero gradient and fit (0, 0, 0, M).  The loss is O(1) whatever the image size: there is no
    1 / (W H) in `weight`.  `loss_out`: a 1-element float32 device tensor that receives the loss instead of a fresh one; `fit_out`:
    the same for the 4 floats of the fit (a row of a (V, 4) tensor).  The gradient goes to backward(dL_ddepth_image=...)."""
    who = "depth_corr_loss_and_gradients"
    hw = _args.image_hw(rendered, f"{who}: rendered")
    _args.image_hw(target, f"{who}: target", hw)
    if mask is not None:
        _args.image_hw(mask, f"{who}: mask", hw)
    weight = _args.finite(weight, f"{who}: weight")
    _args.check_slot(loss_out, 1, f"{who}: loss_out")
    _args.check_slot(fit_out, _lib.DEPTH_CORR_FIT_FLOATS, f"{who}: fit_out", contiguous=True)
    L = _lib.lib()
    dev = _host.device_of(rendered, target, mask)
    H, W = hw
    r = _host.to_dev(rendered, torch.float32, dev, (H, W))
    t = _host.to_dev(target, torch.float32, dev, (H, W))
    m = _host.to_dev(mask, torch.float32, dev, (H, W)) if mask is not None else None
    grad = torch.empty((H, W), dtype=torch.float32, device=dev) if want_grad else None
    loss = torch.empty(1, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    fit = torch.empty(_lib.DEPTH_CORR_FIT_FLOATS, dtype=torch.float32, device=dev) if fit_out is None else fit_out
    with _host.on_device(dev):
        stream = _host.stream_ptr(dev)
        ws = _host.workspace("depth_corr", L.gsr_depth_corr_workspace_bytes(W, H), dev, stream)
        _lib.check(L.gsr_depth_corr_loss_grad(_host.ptr(r), _host.ptr(t), _host.ptr(m), _host.ptr(grad), _host.ptr(loss), _host.ptr(fit), W, H,
                                              weight, _host.ptr(ws), ws.numel(), stream))
    _host.written_in_place(loss_out, fit_out)
    return loss, grad, fit


def _rotation(target_rotation):
    """The `target_rotation` keyword as 9 host floats, row-major (None: identity, passed on as NULL)."""
    if target_rotation is None:
        return None
    if isinstance(target_rotation, torch.Tensor):
        target_rotation = target_rotation.detach().cpu().numpy()
    R = np.asarray(target_rotation, dtype=np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError(f"normal_loss_and_gradients: target_rotation must be a finite 3 x 3 matrix, not shape {R.shape}")
    return R.astype(np.float32).reshape(9)


def normal_loss_and_gradients(depth, final_Ts, target, camera, mask=None, weight=1.0, target_rotation=None, alpha_min=_lib.NORMALS_ALPHA_MIN,
                              want_grad=True, loss_out=None):
    """The cosine loss between the normals of the rendered depth and a normal prior, with its exact gradient, two launches, no host
    sync (include/gsr_normals.h).  `depth` is the forward's inverse-depth image, `final_Ts` its img_buffer["final_Ts"], `camera` a
    dict with tan_fovx, tan_fovy, width, height; `target` (H, W, 3), any length, in camera space after `target_rotation` (a 3 x 3
    matrix applied to every target vector: the view rotation camera["R"] for world-space normals, a flip for another axis
    convention; None: identity); `mask` (H, W) weights m >= 0 (None: all ones).  Normals face the camera: a fronto-parallel surface
    has (0, 0, -1).  A pixel counts where its depth normal is valid (normals.normals_from_depth) and its target is not zero.
    Returns (sums, dL_ddepth_image, dL_dalpha_image): sums a device tensor [2] = (sum m (1 - n . t^), sum m) over those pixels (the
    mean loss is sums[0] / sums[1]); the two (H, W) images are the gradient of weight / (W H) * sums[0] -- depth_loss_and_gradients'
    normalisation -- and go straight into backward(dL_ddepth_image=..., dL_dalpha_image=...); None without want_grad.
    `loss_out`: a 2-element contiguous float32 device tensor that receives the sums instead of a fresh one."""
    who = "normal_loss_and_gradients"
    tx, ty, W, H = _args.camera_params(camera, who)
    a = _args.finite(alpha_min, f"{who}: alpha_min")
    _args.image_hw(depth, f"{who}: depth", (H, W))
    _args.image_hw(final_Ts, f"{who}: final_Ts", (H, W))
    _args.image_hw(target, f"{who}: target", (H, W), 3)
    if mask is not None:
        _args.image_hw(mask, f"{who}: mask", (H, W))
    weight = _args.finite(weight, f"{who}: weight")
    R = _rotation(target_rotation)
    _args.check_slot(loss_out, _lib.NORMALS_SUMS_FLOATS, f"{who}: loss_out", contiguous=True)
    L = _lib.lib()
    dev = _host.device_of(depth, final_Ts, target, mask)
    d = _host.to_dev(depth, torch.float32, dev, (H, W))
    t = _host.to_dev(final_Ts, torch.float32, dev, (H, W))
    tg = _host.to_dev(target, torch.float32, dev, (H, W, 3))
    m = _host.to_dev(mask, torch.float32, dev, (H, W)) if mask is not None else None
    gD = torch.empty((H, W), dtype=torch.float32, device=dev) if want_grad else None
    gA = torch.empty((H, W), dtype=torch.float32, device=dev) if want_grad else None
    sums = torch.empty(_lib.NORMALS_SUMS_FLOATS, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    Rp = R.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)) if R is not None else None
    with _host.on_device(dev):
        stream = _host.stream_ptr(dev)
        ws = _host.workspace("normals", L.gsr_normals_workspace_bytes(W, H), dev, stream)
        _lib.check(L.gsr_normals_loss_grad(_host.ptr(d), _host.ptr(t), _host.ptr(tg), Rp, _host.ptr(m), tx, ty, W, H, a, weight / (W * H),
                                           _host.ptr(gD), _host.ptr(gA), _host.ptr(sums), _host.ptr(ws), ws.numel(), stream))
    _host.written_in_place(loss_out)
    return sums, gD, gA


def normal_consistency_loss_and_gradients(normal_image, depth, final_Ts, camera, mask=None, weight=1.0, alpha_min=_lib.NORMALS_ALPHA_MIN,
                                          loss_out=None):
    """The depth-normal consistency term of 2DGS, GOF, PGSR and RaDe-GS with the gradient on BOTH sides, three launches and the
    depth normals' two, no host sync (include/gsr_normal_render.h).  `normal_image` (H, W, 3) is normal_render.render_normals()'s
    image N of the Gaussians' own normals, `depth` the forward's inverse-depth image, `final_Ts` its img_buffer["final_Ts"],
    `camera` a dict with tan_fovx, tan_fovy, width, height; `mask` (H, W) weights m >= 0 (None: all ones).  A pixel counts where its
    depth normal n_d is valid (normals.normals_from_depth) and |N| >= 1e-3 (decided in float32); its term is m (1 - n_d . N / |N|).
    Returns (sums, gN, gD, gA): sums a device tensor [2] = (sum of the terms, sum m) over the counted pixels (the mean loss is
    sums[0] / sums[1]; arccos(1 - mean) the angle for m = 1), reduced in a fixed order; gN (H, W, 3), gD, gA (H, W) the gradient of
    weight / (W H) * sums[0] with respect to the normal image, the inverse-depth image and the alpha image: they go into
    backward(dL_dnormal_image=gN, dL_ddepth_image=gD, dL_dalpha_image=gA, ...).  `loss_out`: a 2-element contiguous float32 device
    tensor that receives the sums instead of a fresh one."""
    who = "normal_consistency_loss_and_gradients"
    tx, ty, W, H = _args.camera_params(camera, who)
    a = _args.finite(alpha_min, f"{who}: alpha_min")
    if not (_args.is_dev(normal_image, torch.float32) and tuple(normal_image.shape) == (H, W, 3) and normal_image.is_contiguous()):
        raise ValueError(f"{who}: normal_image must be a contiguous float32 device tensor of shape {(H, W, 3)}")
    _args.image_hw(depth, f"{who}: depth", (H, W))
    _args.image_hw(final_Ts, f"{who}: final_Ts", (H, W))
    if mask is not None:
        _args.image_hw(mask, f"{who}: mask", (H, W))
    weight = _args.finite(weight, f"{who}: weight")
    _args.check_slot(loss_out, 2, f"{who}: loss_out", contiguous=True)
    L = _lib.lib()
    dev = normal_image.device
    nimg = _host.to_dev(normal_image, torch.float32, dev)
    m = _host.to_dev(mask, torch.float32, dev, (H, W)) if mask is not None else None
    n_d, valid = _normals.normals_from_depth(depth, final_Ts, camera, a)
    gN = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    gnd = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    sums = torch.empty(2, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    with _host.on_device(dev):
        stream = _host.stream_ptr(dev)
        ws = _host.workspace("normals", L.gsr_normals_workspace_bytes(W, H), dev, stream)
        _lib.check(L.gsr_normal_consistency_loss(_host.ptr(nimg), _host.ptr(n_d), _host.ptr(valid), _host.ptr(m), W, H, weight, _host.ptr(gN),
                                                 _host.ptr(gnd), _host.ptr(sums), _host.ptr(ws), ws.numel(), stream))
    _host.written_in_place(loss_out)
    gD, gA = _normals.normals_from_depth_backward(gnd, depth, final_Ts, camera, a)
    return sums, gN, gD, gA
