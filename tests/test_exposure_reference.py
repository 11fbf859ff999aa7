"""The exposure yardstick checked against itself on the CPU (tests/exposure_reference.py): autograd = closed form on the GPU tests' case
matrix, the recovery loop inside the GPU test's bound on the very case that test uses (rendered here by the CPU oracle), the Adam
statement against a hand-written first step, and the trainer's noise generator."""
import numpy as np
import pytest

from conftest import sub
import exposure_reference as R


def _sizes():
    _lib = sub("_lib")
    return R.case_sizes(_lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS)


def test_case_sizes_cover_the_kernels_paths():
    _lib = sub("_lib")
    bp, mb = _lib.EXPOSURE_BLOCK_PIXELS, _lib.EXPOSURE_MAX_BLOCKS
    px = [w * h for w, h in _sizes()]
    assert px[0] < 4 and px[1] < 4 and px[2] % 4 and px[3] % 4 == 0 and px[4] % 4 and px[4] > bp      # tails, exact groups, several workgroups
    assert 256 < -(-px[5] // bp) <= mb                                                                 # the finish's threads add two records
    assert -(-px[6] // bp) > mb                                                                        # the backward's second round


@pytest.mark.parametrize("k", range(6))
def test_autograd_equals_the_closed_form(k):
    W, H = _sizes()[k]
    c = R.make_case(W, H, 100 + k)
    d_img, dE, mag_img, mag_E = R.backward_closed(c["image"], c["E"], c["g"])
    a_img, a_E = R.backward_autograd(c["image"], c["E"], c["g"])
    eps64 = np.finfo(np.float64).eps
    assert (np.abs(d_img - a_img) <= 8 * eps64 * mag_img).all()
    assert (np.abs(dE - a_E) <= 64 * eps64 * mag_E).all()        # two float64 summation orders of up to 2^18 terms
    assert (c["image"].reshape(-1, 3)[:W * H // 2] == 0).all() and (np.abs(c["image"][..., 2]).max() > 100 or W * H < 4)
    out, mag = R.apply_f64(c["image"], R.IDENTITY)
    assert (out == c["image"]).all() and (mag == np.abs(c["image"])).all()


def test_adam_statement_first_steps_by_hand():
    g = np.linspace(-1e-3, 2e-3, 12)
    E, m, v = R.adam_f64(R.IDENTITY, g, np.zeros(12), np.zeros(12), 0.01, 1)
    nz = g != 0
    assert np.allclose(m, 0.1 * g, rtol=1e-15) and np.allclose(v, 0.001 * g * g, rtol=1e-15)
    assert np.allclose((R.IDENTITY - E)[nz], 0.01 * np.sign(g[nz]), rtol=1e-9)      # the first Adam step is lr * sign(g)
    E2, m2, v2 = R.adam_f64(E, g, m, v, 0.01, 2)
    assert np.allclose(m2, 0.19 * g, rtol=1e-14) and np.allclose((E - E2)[nz], 0.01 * np.sign(g[nz]), rtol=1e-9)
    assert R.decayed_lr(0.01, 0.001, 0, 300) == 0.01 and abs(R.decayed_lr(0.01, 0.001, 299, 300) - 0.001) < 1e-15
    assert R.decayed_lr(0.01, 0.001, 5, 300) == sub("scheduler").decayed_lr(0.01, 0.001, 5, 300)


def test_the_yardstick_recovers_the_exposure_on_the_gpu_tests_case(oracle, scenes, cameras):
    q = R.RECOVERY
    _, _, kw, E_star = R.recovery_case(scenes, cameras, sub("exposure").random_exposures)
    img = np.asarray(oracle.render_gaussians(**kw)[0], np.float32).reshape(q["H"], q["W"], 3)
    assert (img.reshape(-1, 3).max(1) == 0).mean() > 0.2 and (img > 0.05).mean() > 0.2      # Lego-like: black background, a lit object
    A = E_star.reshape(4, 3)
    off = A[:3][~np.eye(3, dtype=bool)]
    assert np.allclose(np.abs(off), q["offdiag"]) and (np.abs(np.log(np.diag(A[:3]))) > 1e-3).all()
    r = R.recover_f64(img, E_star, q["steps"], q["lr0"], q["lr1"])
    print(f"\nfloat64 recovery: L1 {r['initial']:.3e} -> {r['final']:.3e} (x{r['initial'] / r['final']:.1f}), max|E - E*| = {r['max_err']:.3e}")
    assert r["final"] <= r["initial"] / q["loss_factor"]
    assert r["max_err"] <= q["max_err"]


def test_noise_generator_is_deterministic_and_the_identity_at_zero():
    X = sub("exposure")
    a, b = X.random_exposures(8, 0.2, 4), X.random_exposures(8, 0.2, 4)
    assert a.shape == (8, 12) and a.dtype == np.float64 and np.array_equal(a, b)
    assert not np.array_equal(a, X.random_exposures(8, 0.2, 5))
    z = X.random_exposures(8, 0.0, 4)
    assert np.array_equal(z, np.tile(R.IDENTITY, (8, 1))) and not np.signbit(z).any()
    A = a.reshape(8, 4, 3)
    assert (A[:, :3][:, ~np.eye(3, dtype=bool)] == 0).all() and (A[:, [0, 1, 2], [0, 1, 2]] > 0).all()
    # the statistics of the statement: log-gains N(0, 2 S^2) (channel + shared), offsets N(0, (S/4)^2)
    big = X.random_exposures(4000, 0.2, 1).reshape(4000, 4, 3)
    lg = np.log(big[:, [0, 1, 2], [0, 1, 2]])
    assert abs(lg.std() - 0.2 * np.sqrt(2)) < 0.01 and abs(big[:, 3].std() - 0.05) < 0.003 and abs(lg.mean()) < 0.01
    assert abs(np.corrcoef(lg[:, 0], lg[:, 1])[0, 1] - 0.5) < 0.05                           # the shared gain
    with pytest.raises(ValueError):
        X.random_exposures(2, -1.0, 0)
    # the off-diagonals of the recovery case leave the diagonal and b draws alone
    c = X.random_exposures(8, 0.2, 4, offdiag=0.02).reshape(8, 4, 3)
    assert np.array_equal(c[:, 3], A[:, 3]) and np.array_equal(c[:, [0, 1, 2], [0, 1, 2]], A[:, [0, 1, 2], [0, 1, 2]])
