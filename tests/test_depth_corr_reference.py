"""The float64 yardstick of the Pearson-correlation depth loss (tests/depth_corr_reference.py) held to itself on the CPU: the closed
form of include/gsr_depth_corr.h equals torch autograd, the loss has the invariances it is chosen for, degenerate frames give exactly
(1, zeros, (0, 0, 0, M)), and the adversarial case does catch the two float32 shortcuts it is in the matrix for."""
import numpy as np
import pytest

import depth_corr_reference as R

BP, MB = 1024, 1024         # GSR_DEPTH_CORR_BLOCK_PIXELS / _MAX_BLOCKS (tests/test_depth_corr_abi.py holds them to the header)
CHEAP = 1 << 17             # pixels up to which the autograd twin runs


@pytest.fixture(scope="module")
def cases():
    return R.all_cases(BP, MB)


def _live(cases):
    return [c for c in cases if not R.moments(c["r"], c["t"], c["m"])["degenerate"]]


def test_case_matrix_is_the_stated_one(cases):
    sizes = R.case_sizes(BP, MB)
    assert sizes[:6] == [(1, 1), (3, 1), (37, 29), (BP - 1, 1), (BP, 1), (BP + 1, 1)]
    W, H = sizes[6]
    assert W * H > BP * MB and W * H - BP * MB <= 1024                # the first size with a second round
    names = [c["name"] for c in cases]
    assert names[7:] == ["mask_none", "mask_all_zero", "constant_target", "render_all_zero", "negative_correlation", "adversarial"]
    adv = cases[-1]
    assert (adv["W"], adv["H"]) == (W, H) and adv["m"] is None
    for c in cases:
        assert c["r"].dtype == c["t"].dtype == np.float32 and c["r"].shape == c["t"].shape == (c["H"], c["W"])
        if c["m"] is not None:
            assert c["m"].dtype == np.float32 and c["m"].min() >= 0.0
    m = cases[2]["m"]
    assert (m == 0).any() and ((m > 0) & (m < 1)).any() and (m == 1).any()   # zeros and fractional weights
    assert {c["name"] for c in cases if R.moments(c["r"], c["t"], c["m"])["degenerate"]} >= set(R.DEGENERATE)
    assert len(_live(cases)) >= 8


def test_closed_form_equals_autograd(cases):
    done = 0
    for c in _live(cases):
        if c["W"] * c["H"] > CHEAP:
            continue
        for weight in (1.0, 0.37):
            loss, grad, fit = R.closed_form(c["r"], c["t"], c["m"], weight)
            a_loss, a_grad = R.autograd(c["r"], c["t"], c["m"], weight)
            assert abs(loss - a_loss) <= 1e-10, c["name"]
            assert np.abs(grad - a_grad).max() <= 1e-10 * np.abs(a_grad).max(), c["name"]
            assert abs(fit[0] - (1.0 - loss)) <= 1e-15 and fit[3] == (c["m"].astype(np.float64).sum() if c["m"] is not None else c["r"].size)
        done += 1
    assert done >= 7


def test_fit_is_the_least_squares_map_of_the_target_onto_the_render(cases):
    c = cases[2]
    _, _, (rho, s, b, M) = R.closed_form(c["r"], c["t"], c["m"])
    r, t, m = (x.astype(np.float64).reshape(-1) for x in (c["r"], c["t"], c["m"]))
    A = np.stack([t, np.ones_like(t)], 1) * np.sqrt(m)[:, None]
    sol = np.linalg.lstsq(A, r * np.sqrt(m), rcond=None)[0]
    assert np.allclose([s, b], sol, rtol=1e-9, atol=1e-12) and 0.5 < rho < 1.0 and M == m.sum()


def test_invariances_in_float64(cases):
    """Unchanged under t -> a t + b (a > 0); loss -> 2 - loss under a < 0; sum grad = 0 and sum grad r = 0.  The affine maps are
    applied in float64 (the yardstick widens whatever it gets), to 1e-8."""
    for c in _live(cases):
        if c["W"] * c["H"] > CHEAP and c["name"] != "adversarial":
            continue
        loss, grad, _ = R.closed_form(c["r"], c["t"], c["m"])
        gmax = np.abs(grad).max()
        t64 = c["t"].astype(np.float64)
        for a, b in ((3.0, 1.0), (0.25, -2.0)):
            l2, g2, _ = R.closed_form(c["r"], a * t64 + b, c["m"])
            assert abs(l2 - loss) <= 1e-8 and np.abs(g2 - grad).max() <= 1e-8 * gmax, (c["name"], a, b)
        l3, g3, _ = R.closed_form(c["r"], -3.0 * t64 + 1.0, c["m"])
        assert abs(l3 - (2.0 - loss)) <= 1e-8 and np.abs(g3 + grad).max() <= 1e-8 * gmax, c["name"]
        r64 = c["r"].astype(np.float64)
        assert abs(grad.sum()) <= 1e-8 * np.abs(grad).sum(), c["name"]
        assert abs((grad * r64).sum()) <= 1e-8 * np.abs(grad * r64).sum(), c["name"]
    neg = [c for c in cases if c["name"] == "negative_correlation"][0]
    assert R.closed_form(neg["r"], neg["t"], neg["m"])[0] > 1.5


def test_degenerate_frames_give_exactly_one_zeros_and_the_weight_total(cases):
    seen = set()
    for c in cases:
        if not R.moments(c["r"], c["t"], c["m"])["degenerate"]:
            continue
        loss, grad, fit = R.closed_form(c["r"], c["t"], c["m"], 0.7)
        M = float(c["m"].astype(np.float64).sum()) if c["m"] is not None else float(c["r"].size)
        assert loss == 1.0 and grad.shape == c["r"].shape and not grad.any() and fit.tolist() == [0.0, 0.0, 0.0, M], c["name"]
        seen.add(c["name"])
    assert seen >= set(R.DEGENERATE)


def test_the_adversarial_case_rejects_the_two_float32_shortcuts(cases):
    adv = cases[-1]
    assert adv["name"] == "adversarial"
    q = R.moments(adv["r"], adv["t"], None)
    raw = R.raw_moment_variance_f32(adv["r"])
    centring = R.centring_error_f32(adv["r"])
    print(f"\nadversarial: Vr = {q['Vr']:.4e}, one-pass float32 variance {raw:.4e} (off by {abs(raw - q['Vr']) / q['Vr']:.2f}); "
          f"float32 centring off by {centring:.0f} eps32 of the spread; rho = {q['C'] / np.sqrt(q['Vr'] * q['Vt']):.6f}")
    assert 0.9e-6 < q["Vr"] < 1.1e-6
    assert abs(raw - q["Vr"]) > 0.1 * q["Vr"]
    assert centring > 100.0
