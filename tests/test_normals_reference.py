"""The float64 yardstick of the normals stage (tests/normals_reference.py) against what is known in closed form, on the CPU: a plane
gives its own normal, autograd agrees with finite differences and with the header's gather written out, the loss has the
invariances the header states, and a float32 restatement of the formulas stays inside the error model eps32 x kappa that
tests/test_gpu_normals.py states its bounds in."""
import numpy as np
import pytest

import normals_reference as R

TILE_W, TILE_H, MAX_BLOCKS = 32, 8, 2048      # include/gsr_normals.h (tests/test_normals_abi.py holds them to the header)
# What a float32 restatement may reach, in units of eps32 kappa: a difference of two points of size |P| carries at most 2 x eps32 / 2
# of |P| from the points' own roundings and eps32 / 2 of itself, and a normal depends on two such differences: 2 x 1.5 = 3; the
# products behind them (z r) add one more rounding each.  4 bounds the sum; measured on the CPU: 1.2-1.5 (normals), 0.7-0.8 (gradients).
MODEL_BOUND = 4.0


@pytest.fixture(scope="module")
def cases():
    return [c for c in R.all_cases(TILE_W, TILE_H, MAX_BLOCKS)]


def test_a_tilted_plane_gives_its_normal_and_a_fronto_parallel_one_faces_the_camera():
    for W, H in ((37, 29), (100, 100)):
        cam = R.camera(W, H)
        z, n0 = R.plane_depth(cam)
        n = R.normals_from_z(z, cam)
        err = np.abs(n[1:-1, 1:-1] - n0).max()
        print(f"plane {W}x{H}: max |n - n0| = {err:.2e}")
        assert err <= 1e-12
        assert np.isnan(n[0]).all() and np.isnan(n[:, 0]).all()              # no normal on the image border
        flat = R.normals_from_z(np.full((H, W), 2.5), cam)
        assert np.abs(flat[1:-1, 1:-1] - np.array([0.0, 0.0, -1.0])).max() <= 1e-12


def _small_case(seed=3, **kw):
    rng = np.random.default_rng(seed)
    W, H = 9, 7
    return R._case("small", W, H, R.wavy_depth(R.camera(W, H), rng), rng, **kw)


def test_autograd_agrees_with_finite_differences():
    c = _small_case(mask=True, rot=True)
    ref = R.reference(c)
    assert c["dec"]["valid"].sum() >= 20
    D0, T0 = c["Dinv"].astype(np.float64), c["final_T"].astype(np.float64)
    h = 1e-6
    worst = 0.0
    for (y, x) in [(yy, xx) for yy in range(c["H"]) for xx in range(c["W"])]:
        e = np.zeros_like(D0)
        e[y, x] = h
        fd_D = (_loss64(c, D0 + e, T0) - _loss64(c, D0 - e, T0)) / (2 * h)
        fd_A = -(_loss64(c, D0, T0 + e) - _loss64(c, D0, T0 - e)) / (2 * h)
        worst = max(worst, abs(fd_D - ref["gD"][y, x]) / np.abs(ref["gD"]).max(), abs(fd_A - ref["gA"][y, x]) / np.abs(ref["gA"]).max())
    print(f"autograd against central differences (h = {h}): worst {worst:.2e} of max|g|")
    assert worst <= 1e-6


def _loss64(c, D, T):
    """weight32 x loss_sum in float64 for float64 images, under the case's float32 validity pattern."""
    import torch
    th, t_ok = R.target_unit(c["target"], c["R"])
    ok = c["dec"]["valid"] & t_ok
    m = np.ones(ok.shape) if c["mask"] is None else c["mask"].astype(np.float64)
    n = R.torch_normals(torch.as_tensor(D), torch.as_tensor(1.0 - T), c["dec"], c["cam"]).numpy()
    return float((np.where(ok, m, 0.0) * (1.0 - (n * th).sum(-1))).sum()) * c["weight32"]


def test_closed_form_gather_agrees_with_autograd(cases):
    rng = np.random.default_rng(5)
    for c in cases:
        if c["degenerate"] or c["finite_only"] or c["W"] * c["H"] > 1 << 16:
            continue
        ref, cf = R.reference(c), R.closed_form(c)
        assert np.array_equal(ref["valid"], cf["valid"])
        assert np.abs(ref["normals"] - cf["normals"]).max() <= 1e-12
        for k in ("gD", "gA"):
            assert np.abs(ref[k] - cf[k]).max() <= 1e-10 * np.abs(ref[k]).max(), (c["name"], k)
        assert abs(ref["sums"][0] - cf["sums"][0]) <= 1e-10 * abs(ref["sums"][0]) and ref["sums"][1] == pytest.approx(cf["sums"][1], rel=1e-14)
        g = rng.normal(0, 1, (c["H"], c["W"], 3))
        _, aD, aA = R.autograd_vjp(c, g)
        cD, cA = R.closed_form_vjp(c, g)
        assert np.abs(aD - cD).max() <= 1e-10 * np.abs(aD).max() and np.abs(aA - cA).max() <= 1e-10 * np.abs(aA).max(), c["name"]


def test_loss_is_blind_to_the_scale_of_depth_and_of_the_target():
    c = _small_case(mask=True)
    ref = R.reference(c)
    scaled = dict(c, Dinv=(np.float32(4) * c["Dinv"]))                        # exact in float32: the same decisions
    scaled["dec"] = R.decide(scaled["Dinv"], c["final_T"], c["cam"])
    assert np.array_equal(scaled["dec"]["valid"], c["dec"]["valid"])
    r2 = R.reference(scaled)
    assert abs(r2["sums"][0] - ref["sums"][0]) <= 1e-12 * abs(ref["sums"][0])
    euler = (ref["gD"] * c["Dinv"].astype(np.float64)).sum()
    print(f"sum gD Dinv = {euler:.2e} against sum |gD Dinv| = {np.abs(ref['gD'] * c['Dinv']).sum():.2e}")
    assert abs(euler) <= 1e-12 * np.abs(ref["gD"] * c["Dinv"]).sum()
    r3 = R.reference(dict(c, target=np.float32(4) * c["target"]))
    assert abs(r3["sums"][0] - ref["sums"][0]) <= 1e-12 * abs(ref["sums"][0])
    assert np.abs(r3["gD"] - ref["gD"]).max() <= 1e-12 * np.abs(ref["gD"]).max()


def test_rotating_the_target_equals_rotating_it_beforehand():
    c = _small_case(rot=True)
    ref = R.reference(c)
    t = c["target"].astype(np.float64) @ c["R"].astype(np.float64).T           # R t, stored as float32: eps32 / 2 per component
    pre = R.reference(dict(c, target=t.astype(np.float32), R=None))
    assert abs(pre["sums"][0] - ref["sums"][0]) <= 8 * R.EPS32 * ref["sums"][1]
    assert np.abs(pre["gD"] - ref["gD"]).max() <= 8 * R.EPS32 * np.abs(ref["gD"]).max()


def test_a_float32_restatement_stays_inside_the_error_model(cases):
    print()
    seen = 0
    for c in cases:
        if c["degenerate"] or c["finite_only"] or c["W"] * c["H"] > 1 << 16:
            continue
        ref, f32 = R.closed_form(c), R.restatement32(c)
        kap = R.kappa(c)
        e = R.error_ratios(f32, ref, kap)
        print(f"{c['name']:22s} kappa {kap:8.1f}  float32 restatement, units of eps32 kappa: normals {e['normals']:.3f} gD {e['gD']:.3f} gA {e['gA']:.3f}; "
              f"sums {e['sums']:.3f} eps32")
        assert np.array_equal(f32["valid"], ref["valid"])
        assert 0 < e["normals"] <= MODEL_BOUND and e["gD"] <= MODEL_BOUND and e["gA"] <= MODEL_BOUND, c["name"]
        seen += 1
    assert seen >= 10


def test_the_case_matrix_covers_what_it_says(cases):
    names = {c["name"] for c in cases}
    assert {f"wavy_{w}x{h}" for w, h in ((1, 1), (2, 2), (3, 1), (3, 3), (37, 29), (31, 7), (32, 8), (33, 9), (65, 17), (130, 70))} <= names
    assert sum(c["degenerate"] for c in cases) >= 5 and sum(c["finite_only"] for c in cases) == 2
    one = [c for c in cases if c["name"] == "wavy_3x3"][0]
    assert one["dec"]["valid"].sum() == 1
    for c in cases:
        if c["name"].startswith("holes"):
            share = (~c["dec"]["defined"]).mean()
            assert 0.03 <= share <= 0.08, share
    assert any(c["mask"] is None for c in cases) and any(c["mask"] is not None for c in cases)
    assert any(c["R"] is None for c in cases) and any(c["R"] is not None for c in cases)
    assert any(not c["want_grad"] for c in cases)
