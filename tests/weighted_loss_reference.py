"""The weighted colour loss of include/gsr_weighted_loss.h restated in float64 torch, on dssim_reference.ssim_terms.

m is an (H, W) image of weights >= 0 and M = sum m.  The window sums run over all pixels of the image whatever their weight: the
weight multiplies the loss map, not the images.
    l1_sum   = sum_p m_p sum_c |x - y|
    ssim_sum = sum_p m_p (1/3) sum_c S_c(p)
    L        = (1 - lambda) l1_sum / (3 M) + lambda (1 - ssim_sum / M)
    pixel_grad(q, c) = (1 - lambda) / (3 M) m_q sign(x - y) - lambda / (3 M) [(w*(m alpha))(q) + 2 x_q (w*(m beta))(q) + y_q (w*(m gamma))(q)]
With M = 0 both sums are 0 and pixel_grad is all zeros.
"""
import torch

import dssim_reference as R

F64 = R.F64
RAD = R.RAD


def l1_sum(x, y, m):
    return (m[..., None] * (x - y).abs()).sum()


def ssim_sum(x, y, m, window="gaussian"):
    return (m * R.ssim_terms(x, y, window)[0].mean(-1)).sum()


def loss(x, y, m, lam, window="gaussian"):
    """L for M > 0 (a torch scalar: differentiable in x)"""
    M = m.sum()
    return (1 - lam) * l1_sum(x, y, m) / (3 * M) + lam * (1 - ssim_sum(x, y, m, window) / M)


def pixel_grad(x, y, m, lam, window="gaussian"):
    """dL/dx by the closed form above, sign(0) = +1; all zeros when M = 0."""
    M = float(m.sum())
    if M == 0.0:
        return torch.zeros_like(x)
    H, W = x.shape[0], x.shape[1]
    S, (m1, m2, A, B, C, D, Wp) = R.ssim_terms(x, y, window)
    mm = m[..., None]
    alpha = mm * S * (2 * m2 / A - 2 * m2 / B - 2 * m1 / C + 2 * m1 / D) / Wp
    beta = mm * (-S / D / Wp)
    gamma = mm * (2 * S / B / Wp)
    Mx, My = R.band(W, window, x.device), R.band(H, window, x.device)
    adj = lambda a: R._conv(My.T, Mx.T, a)
    sign = torch.where(x - y < 0, -1.0, 1.0).to(F64)
    return (1 - lam) / (3 * M) * mm * sign - lam / (3 * M) * (adj(alpha) + 2 * x * adj(beta) + y * adj(gamma))


def autograd_grad(x, y, m, lam, window="gaussian"):
    """dL/dx by autograd (x != y everywhere: |.| is differentiated away from 0)"""
    xr = x.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(loss(xr, y, m, lam, window), xr)
    return g


def _pool(a, r, largest):
    """max (or min) of the (H, W) image a over each (2r+1) x (2r+1) neighbourhood, clipped to the image"""
    a = a if largest else -a
    p = torch.nn.functional.max_pool2d(a[None, None], 2 * r + 1, stride=1, padding=r)[0, 0]
    return p if largest else -p


def dilate_zeros(m, r):
    """the minimum over each (2r+1)^2 neighbourhood: the zero region of m grown by r pixels (PixelWeights(dilate=r))"""
    return _pool(m, r, largest=False) if r else m


def reach(m, r=RAD):
    """True where some pixel within r (the window radius) has weight > 0: the only pixels that may receive a gradient"""
    return _pool((m > 0).to(m.dtype), r, largest=True) > 0
