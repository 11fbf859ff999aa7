"""
The float32 oracle's Adam step against the independent float64 statement of it (tests/adam_reference.py), and that
statement's SH-from-views gradient against a second route.  No GPU.

oracle.adam_update and the kernels share one float32 expression tree by construction, so every other Adam test would pass
a misreading common to both.  Here the oracle meets float64 arithmetic written from the reference's Python, with every
convention of the step a switch, on a matrix of sizes, iterations, hyperparameters, gradient families and clamp edges with
five pairwise distinct learning rates.  tests/test_gpu_adam_f64.py holds the kernels to the same statement.

Float32 error model (u = 2^-24, one rounding; TINY = 2^-149, one rounding in the subnormal range), element by element, with
every magnitude taken from the float64 side.  "carry" is the bound on the incoming array: zero for a single step from exact
float32 inputs, the bound of the step before in the trajectory:
  m'  = b1 m + (1-b1) g        two products and a sum: |dm| <= b1 carry + 3u (b1|m| + (1-b1)|g|) + 2 TINY;
  v'  = b2 v + (1-b2) g g      three products and a sum of positive terms: |dv| <= b2 carry + 4u v' + 4 TINY;
  bc  = 1 - powf(b, t)         powf within one unit of its last place (2^-24 below 1) and the subtraction:
                               |dbc| / bc <= u (1 + b^t / (1 - b^t)) -- 999 u for b2 = 0.999 at t = 1, 1 u from t ~ 10^4;
  s   = sqrt(v' / bc2)         |ds| <= min(dv / (2 bc2 s), sqrt(dv / bc2)) + s (dbc2 / 2 + 2u);
  den = s + eps (+ 1e-9)       |dden| <= ds + 2u den;
  r   = (m' / bc1) / den       |dr| <= dm / (bc1 den) + |r| (dbc1 + 4u + dden / den)   (two divisions, the product with lr);
  p'  = p - lr r               |dp| / lr <= carry + dr + u |p'| / lr;
  max(., 0.001), the [0, 1] clamp: 1-Lipschitz, the bound stands;
  q / |q|                      in the 2-norm per quaternion: |dq'| <= |dq| / |q| + 6u (four squares, three sums, the root, a division).
The issue's figures (max |x - x64| / max |x64| for moments, max |p - p64| / lr for parameters) are recorded beside the
largest error / bound ratio; the assertion is element-wise, error <= bound, which implies the bound on the maxima.
"""
import json
import os

import numpy as np
import pytest
import torch

import adam_reference as A
import f64_reference as F

GROUPS = A.GROUPS
U, TINY = 2.0 ** -24, 2.0 ** -149
# five learning rates, pairwise distinct, no two within 20 % of each other (the smallest ratio is 1.6)
LRS = {"positions": 1.0e-2, "scales": 6.1e-3, "rotations": 3.7e-3, "opacities": 2.3e-3, "shs": 1.4e-3}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_margins.json")


def shapes(n):
    return {"positions": (n, 3), "scales": (n, 3), "rotations": (n, 4), "opacities": (n,), "shs": (n * 16, 3)}


# ------------------------------------------------------------------------------------------------------------ case matrix
# moments: "zero" | "real" (|m| ~ 1e-3, v ~ m^2 and above) | "stale" ("real" with a third of the second moments exactly zero under
# first moments of 1e-9: a Gaussian unseen for thousands of steps; the denominator is then eps (+ 1e-9) alone, which is what
# makes the 1e-9 visible).  grads: "dense" | "sparse" (70 % exact zeros) | "zero" | "tiny" (|g| ~ 1e-25: g g underflows) |
# "large" (|g| up to 1e15: g g <= 1e30 stays finite in float32; beyond that the float32 reference itself overflows and
# the comparison would measure float32's range, not the step).  edges: the clamp rows of _edges() are written over rows 0..11.
CASES = [
    ("n1_it0", dict(n=1, it=0, seed=1, grads="dense", moments="zero")),
    ("n63_it1_sparse", dict(n=63, it=1, seed=2, grads="sparse", moments="real")),
    ("n64_it2_beta1", dict(n=64, it=2, seed=3, grads="dense", moments="real", beta1=0.8)),
    ("n65_it9_beta2", dict(n=65, it=9, seed=4, grads="sparse", moments="real", beta2=0.99)),
    ("n255_it999_eps", dict(n=255, it=999, seed=5, grads="dense", moments="real", eps=1e-6)),
    ("n257_it6999_zero_grads", dict(n=257, it=6999, seed=6, grads="zero", moments="stale")),
    ("n1025_it29999", dict(n=1025, it=29999, seed=7, grads="sparse", moments="stale")),
    ("n3001_it10000000", dict(n=3001, it=10_000_000, seed=8, grads="dense", moments="real")),
    ("n257_it0_all_zero", dict(n=257, it=0, seed=9, grads="zero", moments="zero")),
    ("n65_it0_tiny", dict(n=65, it=0, seed=10, grads="tiny", moments="zero")),
    ("n255_it2_large", dict(n=255, it=2, seed=11, grads="large", moments="zero")),
    ("n65_it0_edges", dict(n=65, it=0, seed=12, grads="dense", moments="zero", edges=True)),
    ("n3001_it9_edges", dict(n=3001, it=9, seed=13, grads="sparse", moments="real", edges=True)),
    ("n64_it1_all", dict(n=64, it=1, seed=14, grads="dense", moments="stale", beta1=0.8, beta2=0.99, eps=1e-6, edges=True)),
]
CASE_NAMES = [c[0] for c in CASES]
TRAJECTORY = dict(n=3001, seed=21, steps=200, check=(1, 10, 200))


def _grads(rng, n, family, scale=1e-3):
    out = {}
    for k, s in shapes(n).items():
        if family == "zero":
            g = np.zeros(s)
        elif family == "tiny":
            g = rng.choice([-1.0, 1.0], s) * rng.uniform(0.5e-25, 2e-25, s)
        elif family == "large":
            g = rng.choice([-1.0, 1.0], s) * 10.0 ** rng.uniform(9, 15, s)
        else:
            g = rng.normal(0, scale, s)
            if family == "sparse":
                g = g * (rng.uniform(0, 1, s) > 0.7)
        out[k] = g.astype(np.float32)
    return out


def _edges(P, G, M, V, lrs):
    """Clamp rows.  With zero moments at iteration 0 the step is lr sign(g) (|g| >> eps), so the side each row lands on is known."""
    f = np.float32
    one_step = f(lrs["scales"])
    # scales: at the floor and just above it, pushed down (lands on the floor) and up
    P["scales"][0] = [f(0.001), f(0.001), f(0.001) + f(1e-4)]
    G["scales"][0] = [2e-3, -2e-3, 2e-3]
    P["scales"][1] = [f(0.001) + f(1e-4), f(0.001) + f(0.5) * one_step, f(0.001) + f(2) * one_step]
    G["scales"][1] = [-2e-3, 2e-3, 2e-3]
    # opacities: at 0, at 1 and within one step of each, pushed out and in
    lo = f(lrs["opacities"])
    P["opacities"][0:8] = [0.0, 0.0, 1.0, 1.0, f(0.5) * lo, f(0.5) * lo, f(1) - f(0.5) * lo, f(1) - f(0.5) * lo]
    G["opacities"][0:8] = [2e-3, -2e-3, -2e-3, 2e-3, 2e-3, -2e-3, -2e-3, 2e-3]
    # a zero quaternion with a zero gradient (and zero moments): stays zero, no NaN; and one pushed off zero by its gradient
    P["rotations"][2] = 0.0
    G["rotations"][2] = 0.0
    M["rotations"][2] = 0.0
    V["rotations"][2] = 0.0
    P["rotations"][3] = 0.0
    # rows 0..11 step in the direction of their gradient whatever the case's moments are
    for k, rows in (("scales", slice(0, 2)), ("opacities", slice(0, 8))):
        M[k][rows] = 0.0
        V[k][rows] = 0.0


def build_case(spec):
    """float32 numpy inputs of one step: (P, G, M, V, hyper)."""
    n = spec["n"]
    rng = np.random.default_rng(spec["seed"])
    sh = shapes(n)
    P = {k: rng.normal(0, 1, s).astype(np.float32) for k, s in sh.items()}
    P["scales"] = (np.abs(P["scales"]) * 0.02 + 0.0015).astype(np.float32)
    P["rotations"] /= np.linalg.norm(P["rotations"], axis=1, keepdims=True)
    P["opacities"] = rng.uniform(0.02, 0.98, n).astype(np.float32)
    P["shs"] = (P["shs"] * 0.3).astype(np.float32)
    G = _grads(rng, n, spec["grads"])
    if spec["moments"] == "zero":
        M = {k: np.zeros(s, np.float32) for k, s in sh.items()}
        V = {k: np.zeros(s, np.float32) for k, s in sh.items()}
    else:
        M = {k: rng.normal(0, 1e-3, s).astype(np.float32) for k, s in sh.items()}
        V = {k: (M[k].astype(np.float64) ** 2 * rng.uniform(1.0, 4.0, s)).astype(np.float32) for k, s in sh.items()}
        if spec["moments"] == "stale":
            for k, s in sh.items():
                stale = rng.uniform(0, 1, s) < 1.0 / 3.0
                M[k][stale] = (rng.choice([-1.0, 1.0], s) * 1e-9)[stale]
                V[k][stale] = 0.0
    if spec.get("edges"):
        _edges(P, G, M, V, LRS)
    hyper = dict(beta1=spec.get("beta1", 0.9), beta2=spec.get("beta2", 0.999), epsilon=spec.get("eps", 1e-8), iteration=spec["it"])
    return P, G, M, V, hyper


# ------------------------------------------------------------------------------------------------------------ error model
def _bc_err(beta, t):
    bt = A._f(beta) ** t
    return U * (1.0 + bt / (1.0 - bt))


def model_bounds(P, G, M, V, lrs, hyper, carry=None, widen=True):
    """Per-element bounds of the float32 step's error against float64 (see the module docstring), from the float64 side.
    Returns ({group: bound on |dp| / lr}, {group: bound on |dm|}, {group: bound on |dv|}).  For rotations the parameter bound
    is per quaternion (2-norm), repeated over its four components.  `carry`: the three dicts of bounds of the step before."""
    b1, b2, eps = A._f(hyper["beta1"]), A._f(hyper["beta2"]), A._f(hyper["epsilon"])
    t = hyper["iteration"] + 1
    bc1, bc2 = A.bias_corrections(b1, b2, hyper["iteration"])
    d1, d2 = _bc_err(b1, t), _bc_err(b2, t)
    P64, M64, V64 = A.adam_step(P, G, M, V, lrs, **hyper, widen=widen)
    raw = A.adam_step(P, G, M, V, lrs, **hyper, widen=widen, switches={"scale_floor": False, "opacity_clamp": False, "quat_renormalise": False})[0]
    bp, bm, bv = {}, {}, {}
    for k in GROUPS:
        lr = A._f(lrs[k])
        g, m = A._w(G[k]), np.asarray(M[k], np.float64)
        cp, cm, cv = (carry[i][k] for i in range(3)) if carry is not None else (0.0, 0.0, 0.0)
        dm = b1 * cm + 3 * U * (b1 * np.abs(m) + (1 - b1) * np.abs(g)) + 2 * TINY
        dv = b2 * cv + 4 * U * V64[k] + 4 * TINY
        s = np.sqrt(V64[k] / bc2)
        den = s + eps + (A.DIV_EPS if k in ("positions", "scales", "shs") else 0.0)
        r = (M64[k] / bc1) / den
        with np.errstate(divide="ignore", invalid="ignore"):
            ds = np.minimum(np.where(s > 0, dv / (2 * bc2 * s), np.inf), np.sqrt(dv / bc2)) + s * (0.5 * d2 + 2 * U)
        dr = dm / (bc1 * den) + np.abs(r) * (d1 + 4 * U + (ds + 2 * U * den) / den)
        dp = dr + U * np.abs(raw[k]) / lr
        if k == "rotations":
            length = np.sqrt((raw[k].reshape(-1, 4) ** 2).sum(1))
            row = np.sqrt((dp.reshape(-1, 4) ** 2).sum(1)) + (cp.reshape(-1, 4)[:, 0] if carry is not None else 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                row = np.where(length > 0, row / length + 6 * U / lr, row)
            dp = np.repeat(row, 4).reshape(dp.shape)
        else:
            dp = dp + cp
        bp[k], bm[k], bv[k] = dp, dm, dv
    return bp, bm, bv, (P64, M64, V64)


def _rel(x, x64):
    """max |x - x64| / max |x64|; an all-zero statement demands exact zeros (inf otherwise)."""
    d = float(np.abs(x - x64).max()) if x64.size else 0.0
    top = float(np.abs(x64).max()) if x64.size else 0.0
    if not np.isfinite(d) or not np.all(np.isfinite(x)):
        return float("inf")
    return d / top if top > 0.0 else (0.0 if d == 0.0 else float("inf"))


def measure(got, ref64, bounds, lrs):
    """Rows (array, the issue's error figure, worst error / bound ratio) for the fifteen arrays of one step.  `got`: (P, M, V)
    float32 results; `ref64`: the statement's; `bounds`: model_bounds' (bp, bm, bv).  A NaN anywhere is an infinite error."""
    rows = []
    for name, x, x64, b, unit in [(f"{pre}{k}", got[i][k], ref64[i][k], bounds[i][k], A._f(lrs[k]) if i == 0 else None)
                                  for i, pre in enumerate(("", "m_", "v_")) for k in GROUPS]:
        x = np.asarray(x, np.float64)
        err = np.abs(x - x64)
        if unit is not None:
            err = err / unit
            if name == "rotations":
                err = np.repeat(np.sqrt((err.reshape(-1, 4) ** 2).sum(1)), 4).reshape(err.shape)
            figure = float(np.abs(x - x64).max() / unit) if np.all(np.isfinite(x)) and np.all(np.isfinite(x64)) else float("inf")
        else:
            figure = _rel(x, x64)
        finite = np.isfinite(err) & np.isfinite(b)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / b)
        worst = float("inf") if not finite.all() else (float(ratio.max()) if ratio.size else 0.0)
        rows.append((name, figure, worst))
    return rows


def criterion(rows):
    """The criterion of test_oracle_against_f64: every array's error inside its float32 model."""
    bad = [f"{name}: error {fig:.3e}, {worst:.3g} x the float32 model" for name, fig, worst in rows if not worst <= 1.0]
    assert not bad, "; ".join(bad)


def run_oracle(oracle, inputs, lrs=LRS):
    P, G, M, V, hyper = inputs
    c = lambda d: {k: np.ascontiguousarray(v.copy()) for k, v in d.items()}
    p, m, v = c(P), c(M), c(V)
    oracle.adam_update(p, c(G), m, v, lrs, **hyper)
    return p, m, v


_CACHE = {}


def oracle_case(oracle, name):
    """Inputs, the oracle's step, the statement's and the model's bounds of one case (computed once per session, never changed)."""
    if name not in _CACHE:
        inputs = build_case(dict(CASES)[name])
        *bounds, ref64 = model_bounds(*inputs[:4], LRS, inputs[4])
        got = run_oracle(oracle, inputs)
        _CACHE[name] = dict(inputs=inputs, got=got, ref64=ref64, bounds=bounds, rows=measure(got, ref64, bounds, LRS))
    return _CACHE[name]


def record_margins(key, table):
    """Merge {case: {array: [error, second figure]}} into `key` of tests/golden/adam_margins.json, leaving everything else."""
    data = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            data = json.load(f)
    data.setdefault(key, {}).update({c: {name: [float(f"{fig:.4g}"), float(f"{worst:.4g}")] for name, fig, worst in rows} for c, rows in table.items()})
    try:
        with open(GOLDEN, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:                                              # a read-only checkout: the figures are printed anyway
        pass


def trajectory(step_fn, spec=TRAJECTORY):
    """Run `steps` consecutive steps from zero moments on the 70 %-zeros family.  step_fn(P, G, M, V, hyper) -> (P, M, V) float32
    numpy.  Yields (step count, float32 state, float64 state, bounds) at the steps in spec["check"].  The gradients do not
    depend on the parameters, so both sides see the same sequence."""
    n = spec["n"]
    P, _, M, V, _ = build_case(dict(n=n, it=0, seed=spec["seed"], grads="zero", moments="zero"))
    rng = np.random.default_rng(spec["seed"] + 1)
    s64 = ({k: A._w(x) for k, x in P.items()}, {k: A._w(x) for k, x in M.items()}, {k: A._w(x) for k, x in V.items()})
    s32, carry = (P, M, V), None
    for it in range(spec["steps"]):
        G = _grads(rng, n, "sparse")
        hyper = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, iteration=it)
        # the float64 side continues from its own float64 state: nothing is rounded to float32 between steps
        bp, bm, bv, s64 = model_bounds(*s64[:1], G, *s64[1:], LRS, hyper, carry=carry, widen=False)
        s32 = step_fn(s32[0], G, s32[1], s32[2], hyper)
        carry = (bp, bm, bv)
        if it + 1 in spec["check"]:
            yield it + 1, s32, s64, (bp, bm, bv)


# ------------------------------------------------------------------------------------------------------------ SH from views
# (name, V, degree, N, scale).  V = 17 and 20 exceed GSR_MAX_VIEWS = 16 and are rebuilt in chunks; 0.37 is no 1/V.
SH_CASES = [
    ("v1_deg0_n1", 1, 0, 1, 1.0),
    ("v2_deg1_n64", 2, 1, 64, 1.0),
    ("v3_deg2_n65", 3, 2, 65, 0.37),
    ("v16_deg3_n130", 16, 3, 130, 1.0 / 16),
    ("v17_deg3_n1000", 17, 3, 1000, 1.0 / 17),
    ("v20_deg2_n65", 20, 2, 65, 1.0),
    ("v3_deg3_n1000", 3, 3, 1000, 1.0 / 3),
    ("v2_deg0_n130", 2, 0, 130, 0.37),
]
SH_NAMES = [c[0] for c in SH_CASES]
MAX_VIEWS = 16


def build_sh_case(name):
    """(means (N,3) float32, payloads (V, 3N+4) float32, degree, scale, index of the Gaussian at view 0's camera or None)."""
    _, V, degree, n, scale = next(c for c in SH_CASES if c[0] == name)
    rng = np.random.default_rng(1000 + 31 * V + 7 * degree + n)
    means = rng.normal(0, 1, (n, 3)).astype(np.float32)
    cams = rng.normal(0, 3, (V, 3)).astype(np.float32)
    at = None
    if n > 1:
        at = n // 2
        means[at] = cams[0]
    pay = np.zeros((V, 3 * n + 4), np.float32)
    pay[:, :3 * n] = (rng.normal(0, 1e-3, (V, 3 * n)) * (rng.uniform(0, 1, (V, 3 * n)) > 0.2)).astype(np.float32)
    if at is not None:
        pay[0, 3 * at:3 * at + 3] = [1e-3, -2e-3, 3e-3]            # a gradient the skip must drop
    pay[:, 3 * n:3 * n + 3] = cams
    # the skip is a discontinuity: nothing else may sit near it
    dist = np.linalg.norm(means[:, None, :].astype(np.float64) - cams[None].astype(np.float64), axis=2)
    dist[at if at is not None else slice(0, 0), 0 if at is not None else slice(0, 0)] = 1.0
    assert dist.min() >= 1e-3, dist.min()
    return means, pay, degree, scale, at


def sh_gradient_by_autograd(means, payloads, degree, scale):
    """The second route: d/d(shs) of scale * sum_v sum(colour_v * dL_drgb_v), colour_v = f64_reference.sh_colour at view v's
    directions, with the views' gradient rows zeroed where the Gaussian is within 1e-8 of the camera."""
    n = means.shape[0]
    shs = torch.zeros(n, 16, 3, dtype=torch.float64, requires_grad=True)
    total = 0.0
    for row in payloads:
        dirs, length = A.view_directions(means, row[3 * n:3 * n + 3])
        w = A._w(row[:3 * n]).reshape(n, 3) * (length >= 1e-8)[:, None]
        total = total + (F.sh_colour(shs, torch.as_tensor(dirs), degree) * torch.as_tensor(w)).sum()
    (g,) = torch.autograd.grad(A._f(scale) * total, shs)
    return g.numpy().reshape(n * 16, 3)


# ------------------------------------------------------------------------------------------------------------ tests
def test_oracle_against_f64(oracle):
    table = {}
    for name in CASE_NAMES:
        c = oracle_case(oracle, name)
        table[name] = c["rows"]
    step = lambda P, G, M, V, hyper: run_oracle(oracle, (P, G, M, V, hyper))
    for n_steps, s32, s64, bounds in trajectory(step):
        table[f"trajectory_step{n_steps}"] = measure(s32, s64, bounds, LRS)
    print("\n  case / array                error vs f64   error / float32 model    (oracle)")
    for name, rows in table.items():
        for arr, fig, worst in rows:
            print(f"  {name:24s} {arr:12s} {fig:.3e}      {worst:.3f}")
    record_margins("oracle_vs_f64", table)
    for name, rows in table.items():
        try:
            criterion(rows)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
    # the SH statement against the autograd route: float64 rounding
    for name in SH_NAMES:
        means, pay, degree, scale, at = build_sh_case(name)
        g = A.sh_gradient_from_views(means, pay, degree, scale)
        g2 = sh_gradient_by_autograd(means, pay, degree, scale)
        assert g.shape == (means.shape[0] * 16, 3)
        assert np.abs(g - g2).max() <= 1e-13 * max(np.abs(g2).max(), 1e-300), f"{name}: {np.abs(g - g2).max():.3e}"


def _sh_agrees(name, switches):
    means, pay, degree, scale, at = build_sh_case(name)
    g = A.sh_gradient_from_views(means, pay, degree, scale, switches)
    g2 = sh_gradient_by_autograd(means, pay, degree, scale)
    assert np.abs(g - g2).max() <= 1e-13 * max(np.abs(g2).max(), 1e-300), f"SH gradient differs by {np.abs(g - g2).max():.3e}"


@pytest.mark.parametrize("switch", list(A.SWITCHES))
def test_each_convention_is_load_bearing(oracle, switch):
    """Flip one convention away from the reference: the oracle must then FAIL the criterion on at least one case.  A switch
    no case detects would mean the matrix lacks the case that exercises it, and that a kernel wrong there would pass."""
    flip = {switch: not A.SWITCHES[switch]}
    if switch.startswith("sh_"):
        for name in SH_NAMES:
            try:
                _sh_agrees(name, flip)
            except AssertionError as err:
                print(f"\n{switch}: detected on {name}: {str(err)[:140]}")
                return
        pytest.fail(f"flipping {switch} is not detected by any SH case")
    for name in CASE_NAMES:
        c = oracle_case(oracle, name)
        P, G, M, V, hyper = c["inputs"]
        ref = A.adam_step(P, G, M, V, LRS, **hyper, switches=flip)
        try:
            criterion(measure(c["got"], ref, c["bounds"], LRS))
        except AssertionError as err:
            print(f"\n{switch}: detected on {name}: {str(err)[:140]}")
            return
    pytest.fail(f"flipping {switch} is not detected by any case")


@pytest.mark.parametrize("pair", [(a, b) for i, a in enumerate(GROUPS) for b in GROUPS[i + 1:]], ids=lambda p: f"{p[0]}-{p[1]}")
def test_learning_rates_are_told_apart(oracle, pair):
    """The statement with two groups' learning rates swapped must fail the criterion against the oracle, on EVERY case whose
    gradients or moments move the parameters: a swap in the kernel's argument wiring then fails the GPU test too."""
    a, b = pair
    swapped = dict(LRS, **{a: LRS[b], b: LRS[a]})
    detected = []
    for name in CASE_NAMES:
        c = oracle_case(oracle, name)
        P, G, M, V, hyper = c["inputs"]
        ref = A.adam_step(P, G, M, V, swapped, **hyper)
        try:
            criterion(measure(c["got"], ref, c["bounds"], LRS))
        except AssertionError:
            detected.append(name)
    still = [n for n in CASE_NAMES if n not in detected]
    print(f"\n{a} <-> {b}: detected on {len(detected)} of {len(CASE_NAMES)} cases; not on {still}")
    assert "n1_it0" in detected and "n3001_it10000000" in detected, detected
    # undetected only where nothing moves (all-zero) or the step is below float32's resolution of the parameter (tiny)
    assert set(still) <= {"n257_it0_all_zero", "n65_it0_tiny"}, still


def test_case_matrix_reaches_the_edges(oracle):
    """The edges the tests above rely on are really in the matrix, counted on the oracle's run."""
    seen = dict(scale_on_floor=0, opacity_clamped_at_0=0, opacity_clamped_at_1=0, second_moment_exactly_zero=0,
                second_moment_zero_under_gradient=0, zero_length_quaternion=0, skipped_at_camera=0, chunked_views=0,
                powf_underflowed=0, n_not_multiple_of_4=0)
    for name in CASE_NAMES:
        c = oracle_case(oracle, name)
        P, G, M, V, hyper = c["inputs"]
        p, m, v = c["got"]
        free = A.adam_step(P, G, M, V, LRS, **hyper, switches={"scale_floor": False, "opacity_clamp": False})[0]
        seen["scale_on_floor"] += int(((p["scales"] == np.float32(0.001)) & (free["scales"] < A.FLOOR - 1e-5)).sum())
        seen["opacity_clamped_at_0"] += int(((p["opacities"] == 0.0) & (free["opacities"] < -1e-5)).sum())
        seen["opacity_clamped_at_1"] += int(((p["opacities"] == 1.0) & (free["opacities"] > 1.0 + 1e-5)).sum())
        seen["second_moment_exactly_zero"] += int(sum((v[k] == 0.0).sum() for k in GROUPS))
        seen["second_moment_zero_under_gradient"] += int(sum(((v[k] == 0.0) & (G[k] != 0.0)).sum() for k in GROUPS))
        seen["zero_length_quaternion"] += int((np.abs(p["rotations"]).max(1) == 0.0).sum())
        seen["powf_underflowed"] += int(np.float32(hyper["beta2"]) ** np.float32(hyper["iteration"] + 1) == 0.0)
        seen["n_not_multiple_of_4"] += int(P["positions"].shape[0] % 4 != 0)
        assert all(np.isfinite(x[k]).all() for x in (p, m, v) for k in GROUPS), name
    zero = oracle_case(oracle, "n257_it0_all_zero")
    for k in GROUPS:                                                  # zero gradients on zero moments: exactly no update
        moved = np.abs(zero["got"][0][k] - zero["inputs"][0][k]).max()
        assert moved <= (2.0 ** -23 if k == "rotations" else 0.0), (k, moved)   # (the renormalisation may round a unit quaternion)
        assert not zero["got"][1][k].any() and not zero["got"][2][k].any(), k
    for name in SH_NAMES:
        means, pay, degree, scale, at = build_sh_case(name)
        n = means.shape[0]
        if at is not None:
            length = A.view_directions(means, pay[0, 3 * n:3 * n + 3])[1]
            seen["skipped_at_camera"] += int((length < 1e-8).sum())
            assert pay[0, 3 * at:3 * at + 3].any()
        seen["chunked_views"] += int(pay.shape[0] > MAX_VIEWS)
    print("\nedges in the Adam case matrix:", seen)
    assert all(x > 0 for x in seen.values()), seen
    assert float(10_000_000 + 1) == float(np.float32(10_000_000 + 1)), "float(iteration + 1) must still be exact"
    assert {dict(CASES)[c]["n"] for c in CASE_NAMES} >= {1, 63, 64, 65, 255, 257, 1025, 3001}
    assert {dict(CASES)[c]["it"] for c in CASE_NAMES} >= {0, 1, 2, 9, 999, 6999, 29999, 10_000_000}
    rates = sorted(LRS.values())
    assert all(hi / lo > 1.2 for lo, hi in zip(rates, rates[1:])), rates
