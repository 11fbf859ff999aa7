"""
The HIP kernels against the independent float64 statement of the reference (tests/f64_reference.py), on the case matrix
of tests/test_f64_reference.py plus two larger cases.  The kernels must meet the same criteria as the oracle does there,
from both backward inputs _fwd_bwd uses (the oracle's forward buffers, and the product's own forward -> backward chain,
which covers the GPU-only paths: the Sigma3D recompute, the SH direction hand-over, record views and block masks), and one
case through the capacity-mode forward with K = D.

Tripwire: per gradient array, the kernel's maximum error against float64 (relative to max|g|) may be at most
3 x max(the oracle's error against float64 on the same case, the kernel's own run-to-run spread) + TRIP_FLOOR.  The
kernel must be no further from the exact answer than the float32 reference-order restatement is.  TRIP_FLOOR = 2e-5 of
max|g|, a fifth of the contract's tight band: the oracle's own errors on the matrix are 1e-7 .. 3e-6 of max|g|.
"""
import numpy as np
import pytest

from conftest import backward_kwargs, pkg, sub
import f64_reference as F
import parity
import test_f64_reference as R

pytestmark = pytest.mark.gpu
TRIP_FLOOR = 2e-5

LARGE = {
    "256x256_n20000": dict(W=256, H=256, n=20000, degree=3, train=True, bg=(0.2, 0.3, 0.4), sm=1.0, seed=31, bright=0.1,
                           opaque=0.1, faint=0.1, scale=0.02),
    "odd_grid_271x83_n2500": dict(W=271, H=83, n=2500, degree=2, train=False, bg=(0.0, 0.0, 0.0), sm=1.3, seed=32, opaque=0.2),
}


def _case(oracle, cameras, name):
    if name in LARGE and name not in R._CACHE:
        R.CASES.append((name, LARGE[name]))          # build_case looks cases up by name
    return R.oracle_case(oracle, cameras, name)


def _np_buf(buf):
    return {k: parity.to_np(v) for k, v in buf.items()}


def _kernel_side(c, fwd, g):
    """A case dict like the oracle's, with the kernel's forward outputs and gradients."""
    img, dep, buf = fwd
    buf = _np_buf(buf)
    d = dict(c, img=parity.to_np(img), dep=parity.to_np(dep), buf=buf, g={k: parity.to_np(v) for k, v in g.items()})
    d["f64"] = R.blend_on_buffers(c["pre"], buf)
    return d


def _check(oracle, cameras, name, capacity=False):
    gsr = pkg()
    c = _case(oracle, cameras, name)
    sc, cam, kw = c["sc"], c["cam"], c["kw"]
    extra = {}
    if capacity:
        D = int(c["buf"]["point_list"].shape[0])
        extra = dict(capacity=D, capacity_hint=D)
    fwd = sub("forward").render_gaussians(**kw, **extra) if capacity else gsr.render_gaussians(**kw)
    for k in ("radii", "point_list", "ranges"):                              # the list order the float64 side was given
        parity.assert_exact(k, fwd[2][k], c["buf"][k])
    f64 = F.backward_f64(sc, kw, c["buf"]["point_list"], c["buf"]["ranges"], c["dpix"], pre=c["pre"])
    g_o = gsr.backward(**backward_kwargs(sc, cam, kw, c["buf"], c["dpix"]))    # from the oracle's forward buffers
    g_o2 = gsr.backward(**backward_kwargs(sc, cam, kw, c["buf"], c["dpix"]))   # again: run-to-run spread
    g_c = gsr.backward(**backward_kwargs(sc, cam, kw, fwd[2], c["dpix"]))      # the product's own chain
    k_side = _kernel_side(c, fwd, g_c)
    rep = R.check_forward(k_side)
    rows = []
    for label, g in (("oracle buffers", g_o), ("own chain", g_c)):
        ks = dict(k_side, g={k: parity.to_np(v) for k, v in g.items()}, buf=c["buf"] if label == "oracle buffers" else k_side["buf"])
        for k in parity.GRAD_KEYS:
            parity.assert_grad(k, ks["g"][k], f64[k])
        assert not np.any(ks["g"]["dL_dcov3D"])
        m = R.geometry_margins(sc, kw, ks["buf"], ks["g"])
        for k, v in m.items():
            assert v <= 1.0, f"{label}: geometry stage {k}: error {v:.2f} x the float32 error model"
    for k in parity.GRAD_KEYS[:-1]:
        e_o = parity.grad_margin(c["g"][k], f64[k])[1]
        e_k = max(parity.grad_margin(g_o[k], f64[k])[1], parity.grad_margin(g_c[k], f64[k])[1])
        spread = parity.grad_margin(g_o2[k], parity.to_np(g_o[k]))[1]
        rows.append((k, e_o, e_k, spread))
    print(f"\n{name}{' (capacity mode, K = D)' if capacity else ''}: forward " + ", ".join(
        f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in rep.items() if not isinstance(v, tuple)))
    print("  array          oracle vs f64   kernel vs f64   kernel spread   (max err / max|g|)")
    for r in rows:
        print("  %-14s %.3e       %.3e       %.3e" % r)
    for k, e_o, e_k, spread in rows:
        assert e_k <= 3.0 * max(e_o, spread) + TRIP_FLOOR, f"{k}: kernel {e_k:.3e} vs float64; oracle {e_o:.3e}, spread {spread:.3e}"


@pytest.mark.parametrize("name", R.CASE_NAMES + list(LARGE))
def test_kernels_against_f64(oracle, cameras, name):
    _check(oracle, cameras, name)


def test_capacity_mode_against_f64(oracle, cameras):
    _check(oracle, cameras, "200x136_n3000", capacity=True)
