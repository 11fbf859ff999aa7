"""
An independent float64 statement of the update half of a training iteration: the reference's Adam step and the SH gradient
the trainer rebuilds from per-view colour gradients (numpy float64, element-wise).

Test helper like tests/f64_reference.py, not a test file.  It is written from the reference's Python (optimizer.py:7-139
for the step, utils/wp_utils.py for the vec3 helpers and their 1e-9, backward.py:84-255 for the SH basis and the
no-gradient rule at the camera centre), not from oracle/ or the kernels: oracle.adam_update restates the step in float32
with the kernels' expression tree, so a misreading shared by both passes every parity test.  Nothing under the product
package or oracle/ imports this module.

Inputs are the float32 arrays and scalars the kernel sees, widened: learning rates, betas and epsilon enter as their float32
values, and so do the literals the reference's kernel holds in float32 (0.001, 1e-9; 1.0 and 0.0 are exact).  The bias
corrections are the float64 1 - beta**(iteration + 1) of the float32 betas, so the error of the float32 powf is something
a comparison measures, not something built in.

Every convention of the step is a named switch in SWITCHES, defaulting to the reference's behaviour; flipping one
(tests/test_adam_reference.py::test_each_convention_is_load_bearing) must make the oracle comparison fail.
"""
import numpy as np

import f64_reference as F

GROUPS = ("positions", "scales", "rotations", "opacities", "shs")

# True = the reference's behaviour.
SWITCHES = {
    # optimizer.py:47-48: the bias corrections use iteration + 1 (the iteration count is 0-based).  False: iteration.
    "bias_iteration_plus_one": True,
    # wp_vec3_div_element adds 1e-9 to the denominator, so positions, scales and SH divide by sqrt(v_hat) + epsilon + 1e-9
    # (optimizer.py:59, :70, :139) while rotation and opacity, written out per component, divide by sqrt(v_hat) + epsilon
    # (:96-99, :125).  False: the other way round.
    "vec3_div_eps_1e9": True,
    # optimizer.py:71-75: each scale component is max(scale - update, 0.001).  False: no floor.
    "scale_floor": True,
    # optimizer.py:126: opacity = max(min(opacity - update, 1), 0).  False: no clamp.
    "opacity_clamp": True,
    # optimizer.py:104-115: the updated quaternion is divided by its length ...  False: left as updated.
    "quat_renormalise": True,
    # ... only if that length is > 0 (:109).  False: divided whatever the length.
    "quat_renormalise_guard": True,
    # optimizer.py:53 etc.: v accumulates the square of the raw gradient.  False: of the bias-corrected first moment.
    "second_moment_of_raw_gradient": True,
    # backward.py:84-86: a view contributes no SH gradient to a Gaussian within 1e-8 of its camera centre.  False: it
    # contributes with the direction 0 the forward evaluates there (the degree-0 term).
    "sh_skip_at_campos": True,
    # backward.py:95-119: coefficients at and above (degree + 1)^2 get no gradient.  False: all sixteen do.
    "sh_zero_above_degree": True,
}

FLOOR = float(np.float32(0.001))        # the literals as the reference's float32 kernel holds them
DIV_EPS = float(np.float32(1e-9))
CAMPOS_EPS = float(np.float32(1e-8))


def _sw(switches):
    s = dict(SWITCHES)
    if switches:
        unknown = set(switches) - set(SWITCHES)
        assert not unknown, f"unknown switches {unknown}"
        s.update(switches)
    return s


def _w(x):
    """float32 rounding (what the kernel sees), then float64."""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _f(x):
    return float(np.float32(x))


def bias_corrections(beta1, beta2, iteration, switches=None):
    t = iteration + 1 if _sw(switches)["bias_iteration_plus_one"] else iteration
    return 1.0 - _f(beta1) ** t, 1.0 - _f(beta2) ** t


def adam_step(params, grads, m, v, lrs, beta1=0.9, beta2=0.999, epsilon=1e-8, iteration=0, switches=None, widen=True):
    """One step over the five groups.  Returns (params, m, v): new float64 copies of all fifteen arrays, shaped as given.
    widen=False: parameters and moments are this function's own float64 results of the step before and are taken as they
    are (a trajectory in float64 throughout); the gradients are float32 values either way."""
    s = _sw(switches)
    own = _w if widen else (lambda x: np.asarray(x, np.float64))
    b1, b2, eps = _f(beta1), _f(beta2), _f(epsilon)
    bc1, bc2 = bias_corrections(beta1, beta2, iteration, switches)
    P, M, V = {}, {}, {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in GROUPS:
            p, g, lr = own(params[k]), _w(grads[k]), _f(lrs[k])
            M[k] = b1 * own(m[k]) + (1.0 - b1) * g
            m_hat = M[k] / bc1
            sq = g * g if s["second_moment_of_raw_gradient"] else m_hat * m_hat
            V[k] = b2 * own(v[k]) + (1.0 - b2) * sq
            denom = np.sqrt(V[k] / bc2) + eps
            if (k in ("positions", "scales", "shs")) == s["vec3_div_eps_1e9"]:
                denom = denom + DIV_EPS
            p = p - lr * (m_hat / denom)
            if k == "scales" and s["scale_floor"]:
                p = np.maximum(p, FLOOR)
            if k == "opacities" and s["opacity_clamp"]:
                p = np.maximum(np.minimum(p, 1.0), 0.0)
            if k == "rotations" and s["quat_renormalise"]:
                q = p.reshape(-1, 4)
                length = np.sqrt((q * q).sum(1, keepdims=True))
                p = (np.where(length > 0.0, q / np.where(length > 0.0, length, 1.0), q) if s["quat_renormalise_guard"]
                     else q / length).reshape(p.shape)
            P[k] = p
    return P, M, V


def sh_basis(dirs, degree):
    """(N, 16) basis values at the (N, 3) directions; columns at and above (degree + 1)^2 are zero.  The basis is
    f64_reference.sh_colour's, read off through its linearity: colour of the k-th unit coefficient vector, minus the 0.5."""
    import torch
    n = dirs.shape[0]
    d = torch.as_tensor(np.ascontiguousarray(dirs, dtype=np.float64))
    eye = torch.eye(16, dtype=torch.float64)
    out = np.zeros((n, 16))
    for k in range((degree + 1) ** 2):
        out[:, k] = (F.sh_colour(eye[k][None, :, None].expand(n, 16, 3), d, degree)[:, 0] - 0.5).numpy()
    return out


def view_directions(means, campos):
    """(unit directions (N, 3), zero where the length is zero; lengths (N,)) from one camera centre to the means."""
    d = _w(means).reshape(-1, 3) - _w(campos).reshape(1, 3)
    length = np.sqrt((d * d).sum(1))
    return np.where(length[:, None] > 0.0, d / np.where(length > 0.0, length, 1.0)[:, None], 0.0), length


def sh_gradient_from_views(means, payloads, degree, scale, switches=None):
    """The (N*16, 3) SH gradient scale * sum_v basis_k(dir_v) * dL_drgb_v.  `payloads`: V rows of 3N + 4 floats (the N
    colour-gradient rows of a view, its camera centre, one unused float).  `scale` enters as its float32 value."""
    s = _sw(switches)
    n = int(np.asarray(means).size // 3)
    out = np.zeros((n, 16, 3))
    for row in payloads:
        row = _w(row).reshape(-1)
        assert row.size == 3 * n + 4, row.size
        dirs, length = view_directions(means, row[3 * n:3 * n + 3])
        basis = sh_basis(dirs, degree if s["sh_zero_above_degree"] else 3)
        if s["sh_skip_at_campos"]:
            basis = basis * (length >= CAMPOS_EPS)[:, None]
        out += basis[:, :, None] * row[:3 * n].reshape(n, 1, 3)
    return (_f(scale) * out).reshape(n * 16, 3)
