"""The L1 + D-SSIM loss of include/gsr_loss.h restated in float64 torch, as the yardstick for the kernels and the oracle.

For channel c at pixel p = (i, j) the 11 x 11 window is clipped to the image and renormalised by its own weight sum
(reference loss.py:76-100): tap q weighs w(|qx - i|) w(|qy - j|), Wp = Sx(i) Sy(j).  The window sums are products with two banded
matrices, Mx[i, qx] = w(|qx - i|) for |qx - i| <= 5, so border clipping is the band ending at the matrix edge.  Two windows:
"reference" w(d) = exp(-(d - 5)^2 / 4.5) (quirk Q21, what gsr_ssim applies) and "gaussian" w(d) = exp(-d^2 / 4.5).

For the power checks only, renorm=False divides every window sum by the full window's weight (the zero-padded convolution).
"""
import torch

RAD = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2
F64 = torch.float64


def weights(window):
    d = torch.arange(RAD + 1, dtype=F64)
    if window == "reference":
        return torch.exp(-(d - RAD) ** 2 / 4.5)
    if window == "gaussian":
        return torch.exp(-d ** 2 / 4.5)
    raise ValueError(window)


def band(n, window, device="cpu"):
    """M[i, q] = w(|q - i|) for |q - i| <= 5, else 0 (n x n)."""
    w = weights(window).to(device)
    i = torch.arange(n, device=device)
    d = (i[None, :] - i[:, None]).abs()
    return torch.where(d <= RAD, w[d.clamp(max=RAD)], torch.zeros((), dtype=F64, device=device))


def _conv(My, Mx, f):
    """(w * f)[j, i, c] = sum_{b, a} My[j, b] Mx[i, a] f[b, a, c]: rows, then columns"""
    H, W = f.shape[0], f.shape[1]
    t = (My @ f.reshape(H, W * 3)).reshape(H, W, 3)
    return torch.einsum("ia,jac->jic", Mx, t)


def ssim_terms(x, y, window="gaussian", renorm=True):
    """Per-pixel, per-channel S (H, W, 3) and the window quantities (m1, m2, A, B, C, D, Wp) of float64 images x, y (H, W, 3)."""
    H, W = x.shape[0], x.shape[1]
    Mx, My = band(W, window, x.device), band(H, window, x.device)
    if renorm:
        Wp = (My.sum(1)[:, None] * Mx.sum(1)[None, :])[..., None]
    else:
        full = weights(window).to(x.device)
        full = full[0] + 2 * full[1:].sum()
        Wp = torch.full((H, W, 1), float(full * full), dtype=F64, device=x.device)
    m1, m2 = _conv(My, Mx, x) / Wp, _conv(My, Mx, y) / Wp
    e11, e22, e12 = _conv(My, Mx, x * x) / Wp, _conv(My, Mx, y * y) / Wp, _conv(My, Mx, x * y) / Wp
    A = 2 * m1 * m2 + C1
    B = 2 * (e12 - m1 * m2) + C2
    C = m1 * m1 + m2 * m2 + C1
    D = (e11 - m1 * m1) + (e22 - m2 * m2) + C2
    return A * B / (C * D), (m1, m2, A, B, C, D, Wp)


def ssim_sum(x, y, window="gaussian", renorm=True):
    """sum over pixels of the channel mean of S: what gsr_ssim and gsr_l1_dssim_loss_grad write to ssim_sum"""
    return ssim_terms(x, y, window, renorm)[0].mean(-1).sum()


def l1_sum(x, y):
    return (x - y).abs().sum()


def loss(x, y, lam, window="gaussian"):
    n = x.numel()
    return (1 - lam) * l1_sum(x, y) / n + lam * (1 - ssim_sum(x, y, window) * 3 / n)


def pixel_grad(x, y, lam, window="gaussian"):
    """dL/dx with sign(0) = +1 in the L1 term (as gsr_l1_loss_grad); the SSIM part by autograd."""
    xr = x.detach().clone().requires_grad_(True)
    n = x.numel()
    (g,) = torch.autograd.grad(ssim_sum(xr, y, window) * 3 / n, xr)
    sign = torch.where(x - y < 0, -1.0, 1.0).to(F64)
    return (1 - lam) / n * sign - lam * g


def closed_form_grad(x, y, window="gaussian"):
    """dSSIM/dx from the alpha / beta / gamma maps of gsr_loss.h (the kernels' formula), SSIM = mean over pixels and channels."""
    H, W = x.shape[0], x.shape[1]
    S, (m1, m2, A, B, C, D, Wp) = ssim_terms(x, y, window)
    alpha = S * (2 * m2 / A - 2 * m2 / B - 2 * m1 / C + 2 * m1 / D) / Wp
    beta = -S / D / Wp
    gamma = 2 * S / B / Wp
    Mx, My = band(W, window, x.device), band(H, window, x.device)
    adj = lambda a: _conv(My.T, Mx.T, a)          # (w * a)(q) = sum_p w(|p - q|) a(p): the same band, transposed (it is symmetric)
    return (adj(alpha) + 2 * x * adj(beta) + y * adj(gamma)) / x.numel()
