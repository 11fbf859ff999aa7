"""The float64 yardstick of the Pearson-correlation depth loss (include/gsr_depth_corr.h): loss = 1 - rho(r, t) under weights m, its
gradient two ways (the closed form of the header and torch autograd, which must agree) and the fit (rho, s, b, M).  Plain numpy /
torch on the CPU; inputs are the float32 values the kernels get, widened.  Every moment is a centred (two-pass) sum, never a raw
moment: the yardstick does not share the cancellation it is there to catch."""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
MIN_REL_VAR = 1e-12        # GSR_DEPTH_CORR_MIN_REL_VAR


def _f64(r, t, m):
    r, t = np.asarray(r, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    m = np.ones_like(r) if m is None else np.asarray(m, np.float64).reshape(-1)
    return r, t, m


def moments(r, t, m=None):
    """{"M", "mu_r", "mu_t", "Vr", "Vt", "C", "degenerate"}: centred weighted moments in float64, and the header's degeneracy test."""
    r, t, m = _f64(r, t, m)
    M = float(m.sum())
    if not M > 0.0:
        return {"M": M, "degenerate": True}
    mu_r, mu_t = float((m * r).sum() / M), float((m * t).sum() / M)
    mu_r += float((m * (r - mu_r)).sum() / M)          # (one correction step: the mean to the last bit that matters)
    mu_t += float((m * (t - mu_t)).sum() / M)
    dr, dt = r - mu_r, t - mu_t
    Vr, Vt, C = float((m * dr * dr).sum() / M), float((m * dt * dt).sum() / M), float((m * dr * dt).sum() / M)
    deg = not (Vr > MIN_REL_VAR * float((m * r * r).sum() / M) and Vt > MIN_REL_VAR * float((m * t * t).sum() / M))
    return {"M": M, "mu_r": mu_r, "mu_t": mu_t, "Vr": Vr, "Vt": Vt, "C": C, "degenerate": deg}


def closed_form(r, t, m=None, weight=1.0):
    """(loss, grad (shape of r), fit (4,)) by the header's formulas in float64; a degenerate frame gives (1, zeros, (0, 0, 0, M))."""
    q = moments(r, t, m)
    shape = np.shape(r)
    if q["degenerate"]:
        return 1.0, np.zeros(shape), np.array([0.0, 0.0, 0.0, q["M"]])
    rr, tt, mm = _f64(r, t, m)
    sd = np.sqrt(q["Vr"] * q["Vt"])
    rho = q["C"] / sd
    grad = -float(weight) * mm / (q["M"] * sd) * ((tt - q["mu_t"]) - (q["C"] / q["Vr"]) * (rr - q["mu_r"]))
    s = q["C"] / q["Vt"]
    return 1.0 - rho, grad.reshape(shape), np.array([rho, s, q["mu_r"] - s * q["mu_t"], q["M"]])


def autograd(r, t, m=None, weight=1.0):
    """(loss, grad) by torch autograd through the centred definition in float64 (a non-degenerate frame)."""
    rr, tt, mm = (torch.tensor(x) for x in _f64(r, t, m))
    rr.requires_grad_(True)
    M = mm.sum()
    dr, dt = rr - (mm * rr).sum() / M, tt - (mm * tt).sum() / M
    rho = (mm * dr * dt).sum() / torch.sqrt((mm * dr * dr).sum() * (mm * dt * dt).sum())
    loss = 1.0 - rho
    (float(weight) * loss).backward()
    return float(loss.detach()), rr.grad.numpy().reshape(np.shape(r))


# ---- the two float32 shortcuts the adversarial case is there to catch ----
def raw_moment_variance_f32(r):
    """sum r^2 / M - mu^2 with every sum and product in float32 (sequential pairwise numpy sums): the one-pass shortcut."""
    r = np.asarray(r, np.float32).reshape(-1)
    n = np.float32(r.size)
    mu = np.sum(r, dtype=np.float32) / n
    return float(np.sum(r * r, dtype=np.float32) / n - mu * mu)


def centring_error_f32(r):
    """max |float32(r_i - float32(mu)) - (r_i - mu)| / std(r), in units of eps32: centring against a mean rounded to float32."""
    r64 = np.asarray(r, np.float64).reshape(-1)
    mu = r64.mean()
    got = (np.asarray(r, np.float32).reshape(-1) - np.float32(mu)).astype(np.float64)
    return float(np.abs(got - (r64 - mu)).max() / r64.std() / EPS32)


# ---- the case matrix shared by the CPU and the GPU tests ----
def case_sizes(block_pixels, max_blocks):
    """(W, H): fewer pixels than a lane's four (1x1, 3x1), odd (37x29), one workgroup's edge ((BP-1)x1, BPx1, (BP+1)x1), and the
    first size that needs a second round: one 1024-pixel row more than max_blocks workgroups take in one."""
    full = block_pixels * max_blocks
    last = (1024, full // 1024 + 1) if full % 1024 == 0 else (full + 3, 1)
    return [(1, 1), (3, 1), (37, 29), (block_pixels - 1, 1), (block_pixels, 1), (block_pixels + 1, 1), last]


def make_case(W, H, seed):
    """An inverse-depth render r in (0.05, 2), a target t = 0.6 r + 0.3 + noise (correlation about 0.9) and a mask with a fifth of its
    pixels zero, a fifth fractional and the rest one.  float32, as the kernels get them."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.05, 2.0, (H, W))
    t = 0.6 * r + 0.3 + rng.normal(0.0, 0.15, (H, W))
    u = rng.uniform(0.0, 1.0, (H, W))
    m = np.where(u < 0.2, 0.0, np.where(u < 0.4, rng.uniform(0.05, 1.0, (H, W)), 1.0))
    return {"name": f"{W}x{H}", "W": W, "H": H, "r": r.astype(np.float32), "t": t.astype(np.float32), "m": m.astype(np.float32)}


SPECIAL_W, SPECIAL_H = 37, 29


def special_cases(multi_round):
    """The named cases: {"name", "W", "H", "r", "t", "m" (or None)}.  `multi_round` = the (W, H) of the multi-round size, where the
    adversarial pair lives (r = 5 + 1e-3 noise, t = 2 r + 0.7 + 5e-4 noise: a spread of 2e-4 of the mean)."""
    base = make_case(SPECIAL_W, SPECIAL_H, 7)
    z = np.zeros_like(base["r"])
    out = [dict(base, name="mask_none", m=None),
           dict(base, name="mask_all_zero", m=z.copy()),
           dict(base, name="constant_target", t=np.full_like(base["t"], 0.75)),
           dict(base, name="render_all_zero", r=z.copy()),
           dict(base, name="negative_correlation", t=(-1.5 * base["t"] + 4.0).astype(np.float32))]
    W, H = multi_round
    rng = np.random.default_rng(11)
    r = (5.0 + 1e-3 * rng.normal(0.0, 1.0, (H, W))).astype(np.float32)
    t = (2.0 * r.astype(np.float64) + 0.7 + 5e-4 * rng.normal(0.0, 1.0, (H, W))).astype(np.float32)
    out.append({"name": "adversarial", "W": W, "H": H, "r": r, "t": t, "m": None})
    return out


DEGENERATE = ("1x1", "mask_all_zero", "constant_target", "render_all_zero")


def all_cases(block_pixels, max_blocks):
    sizes = case_sizes(block_pixels, max_blocks)
    return [make_case(W, H, 100 + k) for k, (W, H) in enumerate(sizes)] + special_cases(sizes[-1])
