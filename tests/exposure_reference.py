"""The float64 yardstick of per-view exposure compensation (include/gsr_exposure.h): c' = c @ A + b, its backward two ways (torch
autograd and the closed form, which must agree), the Adam step, and the frozen-scene recovery loop.  Plain numpy / torch on the
CPU; inputs are the float32 values the kernels get, widened.  E is 12 numbers, row-major (4, 3): A rows 0-2, b row 3."""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15


def split(E):
    E = np.asarray(E, np.float64).reshape(4, 3)
    return E[:3], E[3]


def apply_f64(image, E):
    """(c' (H, W, 3), mag (H, W, 3)): mag = sum_i |c_i A_ij| + |b_j|, what a float32 evaluation's error scales with."""
    A, b = split(E)
    c = np.asarray(image, np.float64)
    return c @ A + b, np.abs(c) @ np.abs(A) + np.abs(b)


def backward_closed(image, E, g):
    """(dL_dimage, dL_dE (12,), mag_image, mag_E (12,)) by the three formulas of the header; the mags are the sums of the terms'
    magnitudes."""
    A, _ = split(E)
    c, g = np.asarray(image, np.float64).reshape(-1, 3), np.asarray(g, np.float64).reshape(-1, 3)
    d_img = (g @ A.T).reshape(np.shape(image))
    mag_img = (np.abs(g) @ np.abs(A).T).reshape(np.shape(image))
    dE = np.concatenate([(c.T @ g).reshape(9), g.sum(0)])
    mag_E = np.concatenate([(np.abs(c).T @ np.abs(g)).reshape(9), np.abs(g).sum(0)])
    return d_img, dE, mag_img, mag_E


def backward_autograd(image, E, g):
    """(dL_dimage, dL_dE (12,)) by torch autograd through c @ A + b in float64."""
    c = torch.tensor(np.asarray(image, np.float64), requires_grad=True)
    Et = torch.tensor(np.asarray(E, np.float64).reshape(4, 3), requires_grad=True)
    out = c @ Et[:3] + Et[3]
    out.backward(torch.tensor(np.asarray(g, np.float64)))
    return c.grad.numpy(), Et.grad.numpy().reshape(12)


def adam_f64(E, g, m, v, lr, step, beta1=BETA1, beta2=BETA2, eps=EPS):
    """One step of gsr_exposure_adam in float64 (step >= 1): returns (E, m, v)."""
    E, g, m, v = (np.asarray(x, np.float64) for x in (E, g, m, v))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    return E - lr * ((m / (1.0 - beta1 ** step)) / (np.sqrt(v / (1.0 - beta2 ** step)) + eps)), m, v


def decayed_lr(lr0, lr1, i, T):
    """scheduler.decayed_lr."""
    return lr0 if T <= 1 else lr0 * ((lr1 / lr0) ** min(i / (T - 1), 1.0))


def l1_and_gradient(out, target):
    """Mean L1 and its gradient, sign(0) = +1 as gsr_l1_loss_grad."""
    d = out - target
    return float(np.abs(d).mean()), np.where(d < 0.0, -1.0, 1.0) / d.size


def recover_f64(image, E_star, steps, lr0, lr1):
    """The frozen-scene loop: target = image @ A* + b* (no clamp), E from the identity, `steps` Adam steps on the mean L1 alone with the
    learning rate decayed lr0 -> lr1.  Returns {"initial", "final" (the loss of the final E), "E", "max_err", "curve"}."""
    image = np.asarray(image, np.float64)
    target, _ = apply_f64(image, E_star)
    E, m, v = IDENTITY.copy(), np.zeros(12), np.zeros(12)
    curve = []
    for t in range(steps):
        out, _ = apply_f64(image, E)
        loss, g = l1_and_gradient(out, target)
        curve.append(loss)
        _, dE, _, _ = backward_closed(image, E, g)
        E, m, v = adam_f64(E, dE, m, v, decayed_lr(lr0, lr1, t, steps), t + 1)
    final = l1_and_gradient(apply_f64(image, E)[0], target)[0]
    return {"initial": curve[0], "final": final, "E": E, "max_err": float(np.abs(E - np.asarray(E_star, np.float64).reshape(12)).max()), "curve": curve}


# ---- the case matrix shared by the CPU and the GPU tests ----
def make_case(W, H, seed):
    """A Lego-like image: the first half of its pixels zero, colours in [0, 1) elsewhere, the blue channel scaled to +-1e4; E near the
    identity; g ~ N(0, 1) / (3 W H).  float32, as the kernels get them."""
    rng = np.random.default_rng(seed)
    P = W * H
    img = rng.uniform(0.0, 1.0, (P, 3))
    img[:P // 2] = 0.0
    img[:, 2] *= rng.choice([-1e4, 1e4], size=P)
    E = IDENTITY + rng.normal(0.0, 0.1, 12)
    g = rng.normal(0.0, 1.0, (P, 3)) / (3.0 * P)
    return {"W": W, "H": H, "image": img.reshape(H, W, 3).astype(np.float32), "E": E.astype(np.float32), "g": g.reshape(H, W, 3).astype(np.float32)}


def case_sizes(block_pixels, max_blocks, finish_threads=256):
    """(W, H): tail only (1x1, 3x1, 5x7: no full 4-pixel group in the first two, 35 = 8 groups + 3), exact groups (64x4), groups plus
    tail over several workgroups (67x33), one more partial record than the finishing workgroup has threads (its threads then add
    more than one), and one pixel-row more than max_blocks workgroups take in one round (the backward's second round)."""
    return [(1, 1), (3, 1), (5, 7), (64, 4), (67, 33), (finish_threads * block_pixels // 512 + 1, 512), (max_blocks * block_pixels // 1024 + 1, 1024)]


# ---- the recovery case: one view of a small synthetic scene at 48 x 40 ----
# 300 Gaussians inside (-0.5, 0.5)^3 over a black background (63 % of the pixels stay black), their SH DC colours three times
# synthetic_scene's: with the generator's pale colours the image's three channels are nearly collinear (condition number of c^T c 117
# against 28 here), two columns of A trade against each other, and 300 steps do not separate them in float64 either (max|E - E*|
# 0.09-0.17 on two seeds of three).  That is a property of the case, not of the arithmetic: the case has the colour spread of a photo.
RECOVERY = {"W": 48, "H": 40, "gaussians": 300, "scale": 0.05, "sigma": 0.5, "seed": 11, "extent": 0.5, "dc_gain": 3.0, "noise": 0.2,
            "offdiag": 0.02, "noise_seed": 3, "steps": 300, "lr0": 0.01, "lr1": 0.001, "loss_factor": 20.0, "max_err": 2e-3}


def recovery_case(scenes, cameras, random_exposures):
    """(scene, camera, render kwargs, E* (12,) float64) of the recovery test: A*, b* drawn as --exposure-noise 0.2 draws them, plus
    off-diagonals of +-0.02."""
    from conftest import lego_camera, render_kwargs
    q = RECOVERY
    sc = scenes.synthetic_scene(q["gaussians"], q["scale"], q["sigma"], q["seed"], extent=q["extent"])
    sc["shs"][:, 0] *= np.float32(q["dc_gain"])
    cam = lego_camera(cameras, 0, q["W"], q["H"])
    return sc, cam, render_kwargs(sc, cam), random_exposures(1, q["noise"], q["noise_seed"], offdiag=q["offdiag"])[0]


def adam_gradients(T, seed=5):
    """A fixed gradient sequence (T, 12) float32: N(0, 1e-3) with a drift, so m and v neither vanish nor settle."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 1e-3, (T, 12)) + 2e-4 * np.sin(np.arange(T)[:, None] / 50.0 + np.arange(12)[None, :])).astype(np.float32)


def adam_run_f64(grads, lr0=0.01, lr1=0.001):
    """E, m, v after every gradient of `grads`, from the identity; and the learning rates, as float32 values (what the kernel gets)."""
    T = len(grads)
    lrs = [float(np.float32(decayed_lr(lr0, lr1, t, T))) for t in range(T)]
    E, m, v = IDENTITY.copy(), np.zeros(12), np.zeros(12)
    for t in range(T):
        E, m, v = adam_f64(E, grads[t], m, v, lrs[t], t + 1, float(np.float32(BETA1)), float(np.float32(BETA2)), float(np.float32(EPS)))
    return E, m, v, lrs
