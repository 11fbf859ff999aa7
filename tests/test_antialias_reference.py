"""CPU-side checks of the float64 yardstick of the antialiased mode (tests/antialias_reference.py): rho's range and limits, its
closed-form derivative against autograd, the two-stage backward against autograd of one float64 loss through the whole
antialiased forward, the antialiased image as the classic image of the scene with opacity * rho, and the case matrix the GPU tests
run (tests/test_gpu_antialias.py): enough sub-pixel Gaussians to show the mode, few enough on the kink of the floor."""
import numpy as np
import pytest
import torch

import antialias_reference as AA
import f64_reference as F
import test_f64_reference as R

D = torch.float64

# The GPU case matrix: test_f64_reference.make_case arguments (SH degrees 0-3, both matrix conventions, scale modifier != 1,
# anisotropy up to 20, opaque / faint / bright / off-screen / behind-camera shares) with scales that put a good share of the
# visible Gaussians below a pixel.  SUBPIXEL_SHARE: the least share of visible Gaussians with rho < 0.5 a case must have;
# KINK_SHARE: the most that may sit within a relative 1e-3 of the floor r = 0.000025 (left out of gradient comparisons).
AA_CASES = [
    ("aa_37x29_n63", dict(W=37, H=29, n=63, degree=2, train=True, bg=(0.5, 0.1, 0.9), sm=1.0, seed=103, bright=0.3, scale=0.02)),
    ("aa_64x48_n64", dict(W=64, H=48, n=64, degree=3, train=False, bg=(0, 0, 0), sm=1.3, seed=104, bright=0.5, scale=0.02)),
    ("aa_64x48_n65", dict(W=64, H=48, n=65, degree=3, train=True, bg=(0.3, 0.3, 0.3), sm=1.0, seed=105, opaque=0.4, faint=0.3, scale=0.02)),
    ("aa_37x29_n257", dict(W=37, H=29, n=257, degree=1, train=True, bg=(0, 0, 0), sm=1.3, seed=106, opaque=0.2, faint=0.2, scale=0.03)),
    ("aa_200x136_n700", dict(W=200, H=136, n=700, degree=3, train=False, bg=(0.1, 0.7, 0.2), sm=1.0, seed=107, bright=0.2, opaque=0.1,
                             scale=0.01)),
    ("aa_200x136_n3000", dict(W=200, H=136, n=3000, degree=3, train=True, bg=(0.9, 0.8, 0.7), sm=1.3, seed=108, bright=0.1, opaque=0.1,
                              faint=0.1, scale=0.008)),
    ("aa_64x48_n700_deg0", dict(W=64, H=48, n=700, degree=0, train=False, bg=(0.2, 0.2, 0.2), sm=1.3, seed=109, opaque=0.3, scale=0.02)),
    ("aa_needles", dict(W=64, H=48, n=300, degree=2, train=True, bg=(0, 0, 0), sm=1.0, seed=110, scale=0.02, aniso=200.0, outside=0)),
]
AA_CASE_NAMES = [c[0] for c in AA_CASES]
SUBPIXEL_SHARE, KINK_SHARE = 0.25, 0.01


def aa_case(cameras, name):
    return R.make_case(cameras, **dict(AA_CASES)[name])


def test_rho_range_limits_and_closed_form_derivative():
    rng = np.random.default_rng(0)
    # covariances from 1e-4 px^2 to 1e4 px^2, any anisotropy and orientation
    l1, l2 = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), (2, 4000)))
    th = rng.uniform(0, np.pi, 4000)
    c, s = np.cos(th), np.sin(th)
    a0 = torch.tensor(l1 * c * c + l2 * s * s, requires_grad=True)
    b = torch.tensor((l1 - l2) * c * s, requires_grad=True)
    c0 = torch.tensor(l1 * s * s + l2 * c * c, requires_grad=True)
    rho, r = AA.rho_of(a0, b, c0)
    assert bool((rho > 0).all()) and bool((rho <= 1).all())
    t64 = lambda v: torch.tensor([v], dtype=D)
    big = t64(900.0), t64(100.0), t64(400.0)          # a splat of tens of pixels
    assert abs(float(AA.rho_of(*big)[0]) - 1.0) < 1e-3
    flat = t64(4.0), t64(2.0), t64(1.0)               # degenerate: det0 = 0
    assert float(AA.rho_of(*flat)[0]) == float(np.sqrt(AA.FLOOR))
    tiny = t64(1e-9), t64(0.0), t64(1e-9)
    assert float(AA.rho_of(*tiny)[0]) == float(np.sqrt(AA.FLOOR))
    # the closed forms (derivative with respect to the blurred a, b, c = with respect to a0, b, c0) against autograd
    ga, gb, gc = torch.autograd.grad(rho.sum(), (a0, b, c0))
    ca, cb, cc = AA.rho_grad_closed(a0.detach(), b.detach(), c0.detach())
    off = (r.detach() - AA.FLOOR).abs() > 1e-9
    assert int((r.detach() <= AA.FLOOR).sum()) > 0 and int((r.detach() > AA.FLOOR).sum()) > 3000
    for g, cf in ((ga, ca), (gb, cb), (gc, cc)):
        err = ((g - cf).abs() / (g.abs() + 1e-300))[off & (g != 0)]
        assert float(err.max()) < 1e-9, float(err.max())
        assert bool((cf[r.detach() <= AA.FLOOR] == 0).all())


TRUE_GRADIENT = {"denom_eps": False, "q1_textbook_backward": False, "q2_cov3d_literal": False, "q16_bwd_scale_modifier_one": False,
                 "q3_view_column_term": False, "frustum_clamp_grad": False, "sh_skip_at_campos": False, "alpha_cap_passes_grad": False,
                 "dnormvdv_floor": False}


def test_backward_is_autograd_of_the_whole_antialiased_forward(oracle, cameras):
    """Every quirk switch set to the true gradient: the two-stage backward with its two additions must equal autograd of one float64
    loss through preprocess + rho + blend, for means, scales, rotations, opacities and SH, to 1e-6 of each array's maximum."""
    sc, cam, kw = R.make_case(cameras, W=40, H=32, n=60, degree=3, train=True, bg=(0.3, 0.1, 0.2), sm=1.3, seed=121, outside=0.1,
                              behind=0.05, opaque=0.2, scale=0.02)
    buf = oracle.render_gaussians(**kw)[2]           # the lists: the classic forward's (radii, rectangles and order do not change)
    dpix = R.pixel_grad(32, 40, seed=5)
    r = AA.backward_aa_f64(sc, kw, buf["point_list"], buf["ranges"], dpix, TRUE_GRADIENT)
    N = sc["means"].shape[0]
    leaves = {"means": F._t(sc["means"], (N, 3)).requires_grad_(True), "shs": F._t(sc["shs"], (N, 16, 3)).requires_grad_(True),
              "opacities": F._t(sc["opacities"], (N,)).requires_grad_(True), "scales": F._t(sc["scales"], (N, 3)).requires_grad_(True),
              "rotations": F._t(sc["rotations"], (N, 4)).requires_grad_(True)}
    pre = AA.preprocess_aa_f64(dict(sc, **leaves), kw, 3, 1.3)
    vis = ~pre["culled"]
    assert int(vis.sum()) >= 30 and int((pre["rho"].detach().numpy()[vis] < 0.5).sum()) >= 8
    assert not AA.near_floor(pre).any()
    img = AA.blend_f64(pre["xy"], pre["conic"], pre["opacity"], pre["colour"], pre["depth"], buf["point_list"], buf["ranges"],
                      pre["cam"].bg, 40, 32, alpha_cap_grad=False)[0]
    (img * torch.as_tensor(dpix, dtype=D)).sum().backward()
    got = {"dL_dmean3D": leaves["means"].grad, "dL_dshs": leaves["shs"].grad.reshape(N * 16, 3), "dL_dopacity": leaves["opacities"].grad,
           "dL_dscale": leaves["scales"].grad, "dL_drot": leaves["rotations"].grad}
    for k, v in got.items():
        m = np.abs(r[k]).max()
        assert m > 0, k
        assert np.abs(v.numpy() - r[k]).max() <= 1e-6 * m, (k, np.abs(v.numpy() - r[k]).max() / m)
    # and the additions matter: without the rho term the scale gradient is another one
    classic = F.backward_f64(dict(sc, opacities=pre["opacity"].detach()), kw, buf["point_list"], buf["ranges"], dpix, TRUE_GRADIENT)
    assert np.abs(classic["dL_dscale"] - r["dL_dscale"]).max() > 1e-2 * np.abs(r["dL_dscale"]).max()


def test_antialiased_image_is_the_classic_image_with_the_effective_opacity(oracle, cameras):
    sc, cam, kw = aa_case(cameras, "aa_64x48_n65")
    buf = oracle.render_gaussians(**kw)[2]
    pre = AA.preprocess_aa_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    got = AA.render_aa_f64(sc, kw, buf["point_list"], buf["ranges"], pre=pre)
    eff = (F._t(sc["opacities"], (pre["N"],)) * AA.rho_of(*AA._forward_cov2d(pre, sc, kw, float(kw["scale_modifier"])))[0]).detach()
    pre_c = F.preprocess_f64(dict(sc, opacities=eff), kw, int(kw["degree"]), float(kw["scale_modifier"]))
    with torch.no_grad():
        ref = AA.blend_f64(pre_c["xy"], pre_c["conic"], pre_c["opacity"], pre_c["colour"], pre_c["depth"], buf["point_list"], buf["ranges"],
                          pre_c["cam"].bg, pre_c["cam"].W, pre_c["cam"].H)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r.numpy())
    classic = R.blend_on_buffers(F.preprocess_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"])), buf)[0]
    assert np.abs(classic - got[0]).max() > 1e-2          # and it is another image than the classic one


@pytest.mark.parametrize("name", AA_CASE_NAMES)
def test_case_matrix_has_subpixel_gaussians_and_stays_off_the_kink(cameras, name):
    sc, cam, kw = aa_case(cameras, name)
    pre = AA.preprocess_aa_f64(sc, kw, int(kw["degree"]), float(kw["scale_modifier"]))
    vis = ~pre["culled"]
    rho = pre["rho"].numpy()[vis]
    sub, kink = float((rho < 0.5).mean()), float(AA.near_floor(pre).sum() / max(1, vis.sum()))
    print(f"\n{name}: {int(vis.sum())} visible, rho < 0.5 on {sub:.3f}, on the floor {float((pre['rho_r'][vis] <= AA.FLOOR).mean()):.3f}, "
          f"within 1e-3 of it {kink:.4f}, rho min {rho.min():.4f} max {rho.max():.4f}")
    assert int(vis.sum()) >= min(20, pre["N"] // 2)
    assert sub >= SUBPIXEL_SHARE
    assert kink <= KINK_SHARE
