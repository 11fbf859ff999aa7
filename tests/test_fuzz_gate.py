"""CPU tests of the fuzz sweep's re-judging gate (tests/test_gpu_fuzz.py::rejudge_allowed) on fabricated arrays: the sweep
may hand a failing gradient array to the needle criterion only when every out-of-band element belongs to a measurably
ill-conditioned Gaussian (seed 15099's kind), never for a well-conditioned one or a uniformly wrong gradient."""
import numpy as np

from test_gpu_fuzz import REJUDGE_KAPPA, REJUDGE_RADIUS, conic_condition, rejudge_allowed


def _fabricated(n=300, seed=0):
    rng = np.random.default_rng(seed)
    ref = rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    conic = np.zeros((n, 4), np.float32)
    conic[:, 0], conic[:, 2], conic[:, 3] = 0.5, 0.4, 0.6        # round splats: condition number 1.25
    radii = np.full(n, 12, np.int32)
    # Gaussian 7 as seed 15099's: radius 325 px, condition number ~2.7e3 (conic eigenvalues 1/11736 and 1/4.3)
    lam_big, lam_small = 1.0 / 4.3, 1.0 / 11736.0
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s], [s, c]])
    M = R @ np.diag([lam_big, lam_small]) @ R.T
    conic[7, :3] = M[0, 0], M[0, 1], M[1, 1]
    radii[7] = 325
    return ref, conic, radii


def test_condition_number_of_the_15099_like_splat():
    _, conic, radii = _fabricated()
    k = conic_condition(conic)
    assert abs(k[0] - 1.25) < 1e-5
    assert 2.5e3 < k[7] < 2.9e3 and k[7] >= REJUDGE_KAPPA and radii[7] >= REJUDGE_RADIUS


def test_15099_like_pattern_is_rejudged():
    ref, conic, radii = _fabricated()
    got = ref.copy()
    got[7] += 0.05 * np.abs(ref).max()                           # only the ill-conditioned splat is out of band
    assert rejudge_allowed(got, ref, conic, radii)


def test_out_of_band_on_a_well_conditioned_gaussian_is_not_rejudged():
    ref, conic, radii = _fabricated()
    got = ref.copy()
    got[7] += 0.05 * np.abs(ref).max()
    got[100, 1] += 1e-3 * np.abs(ref).max()                     # one element of a round splat out of band as well
    assert not rejudge_allowed(got, ref, conic, radii)


def test_small_radius_or_mild_anisotropy_is_not_rejudged():
    ref, conic, radii = _fabricated()
    got = ref.copy()
    got[7] += 0.05 * np.abs(ref).max()
    assert not rejudge_allowed(got, ref, conic, np.where(np.arange(len(radii)) == 7, 40, radii))
    mild = conic.copy()
    mild[7, :3] = 0.5, 0.0, 0.01                                # condition number 50
    assert not rejudge_allowed(got, ref, mild, radii)


def test_gradient_scaled_by_1_01_is_not_rejudged():
    ref, conic, radii = _fabricated()
    assert not rejudge_allowed(ref * np.float32(1.01), ref, conic, radii)


def test_nothing_out_of_band_is_not_rejudged():
    ref, conic, radii = _fabricated()
    assert not rejudge_allowed(ref.copy(), ref, conic, radii)
