"""CPU checks of the float64 yardstick of the 3D smoothing filter (tests/filter3d_reference.py): its own identities, the header's
closed-form transpose against autograd, Mip-Splatting's compute_3D_filter transcribed literally, and the case matrix's exclusion cap."""
import numpy as np
import pytest
import torch

import filter3d_reference as R


@pytest.fixture(scope="module")
def cases(scenes, cameras):
    out = {}
    for name in R.CASE_NAMES:
        c = R.make_case(scenes, cameras, name)
        c["sampling"] = R.sampling_f64(c["scene"]["means"], c["cams"])
        out[name] = c
    return out


def test_identities_of_the_map(cases):
    for c in cases.values():
        s, o, f = c["scene"]["scales"], c["scene"]["opacities"], c["sampling"]["filter_3d"].copy()
        f[::7] = 0.0
        sp, op = (t.numpy() for t in R.apply_f64(s, o, f))
        s64, o64 = s.astype(np.float64), o.reshape(-1).astype(np.float64)
        on = f != 0
        np.testing.assert_allclose(sp ** 2, s64 ** 2 + (f ** 2)[:, None], rtol=1e-13)           # a convolution: variances add
        assert (sp[on] >= np.abs(s64[on])).all() and (sp[on] > 0).all() and (op[on] < o64[on]).all() and (op[on] > 0).all()
        np.testing.assert_array_equal(sp[~on], s64[~on])                                        # f == 0: a pass-through
        np.testing.assert_array_equal(op[~on], o64[~on])
        # the integral opacity * prod s'_k is that of the raw Gaussian, opacity * prod |s_k|
        np.testing.assert_allclose(op * np.abs(sp).prod(1), o64 * np.abs(s64).prod(1), rtol=1e-12)
        sp_neg, op_neg = (t.numpy() for t in R.apply_f64(-s, o, f))                             # a negative scale: its magnitude's s'
        np.testing.assert_array_equal(np.abs(sp_neg), np.abs(sp))
        np.testing.assert_array_equal(op_neg, op)


def test_identities_of_the_sampling_rate(cases, cameras):
    for c in cases.values():
        sm = c["sampling"]
        N = sm["nu"].shape[0]
        seen_any = sm["seen"].any(0)
        np.testing.assert_array_equal(seen_any, sm["any_seen"])
        if seen_any.any():
            f = sm["filter_3d"]
            assert (f > 0).all() and f[~seen_any].tolist() == [f[seen_any].max()] * int((~seen_any).sum())
            np.testing.assert_allclose(f[seen_any] * sm["nu"][seen_any], np.sqrt(np.float64(np.float32(0.2))), rtol=1e-14)
        assert (sm["z_cond"][sm["seen"]] >= 1.0 - 1e-12).all()
        # adding a view can only raise nu; no view, or none that sees anything: zeros
        if len(c["cams"]) > 1:
            fewer = R.sampling_f64(c["scene"]["means"], c["cams"][:-1])
            assert (fewer["nu"] <= sm["nu"]).all()
        assert not R.sampling_f64(c["scene"]["means"], [])["filter_3d"].any()
        far = R.sampling_f64(c["scene"]["means"] * 0 + np.float32(1e4), c["cams"])
        assert not far["filter_3d"].any() and N == far["nu"].shape[0]


def test_the_case_matrix_has_its_edges_and_stays_inside_the_exclusion_cap(cases):
    for name, c in cases.items():
        sm = c["sampling"]
        N = sm["nu"].shape[0]
        excluded = R.near_threshold(sm).any(0)
        assert excluded.sum() <= R.MAX_EXCLUDED * N, (name, int(excluded.sum()))
        if N >= 63:
            m = sm["margins"]
            V = sm["seen"].shape[0]
            z_behind = np.stack([(R.sampling_f64(c["scene"]["means"], [k])["nu_view"][0] < 0) for k in c["cams"]])
            assert z_behind.any(), name                                             # behind a camera
            assert (~sm["seen"] & ~z_behind).any(), name                            # in front, outside the margin
            assert (~sm["any_seen"]).any() and sm["any_seen"].any(), name           # seen by none, and by some
            if V > 1:
                assert (sm["seen"].sum(0) == 1).any(), name                         # seen by one view only
            assert m.shape == (V, N, 3)
    sc = cases["negative"]["scene"]["scales"]
    assert (sc < 0).any() and sc.min() >= -1.0 and 1e-4 <= np.abs(sc).min() and np.abs(sc).max() <= 1.0
    focals = {r[1] for r in R.view_records(cases["mixed"]["cams"])}
    assert len(focals) == 3 and all(k["width"] <= 64 and k["height"] <= 48 for k in cases["mixed"]["cams"])


def test_closed_form_transpose_equals_autograd(cases):
    for name, c in cases.items():
        s, o, f = c["scene"]["scales"], c["scene"]["opacities"], c["sampling"]["filter_3d"].copy()
        f[::5] = 0.0
        rng = np.random.default_rng(len(name))
        g_s, g_o = rng.normal(0, 1, s.shape), rng.normal(0, 1, s.shape[0])
        ds_a, do_a = R.transpose_autograd(s, o, f, g_s, g_o)
        ds_c, do_c, mag = R.transpose_closed(s, o, f, g_s, g_o)
        assert (np.abs(ds_a - ds_c) <= 1e-12 * mag).all(), name
        assert (np.abs(do_a - do_c) <= 1e-12 * np.abs(do_a)).all(), name
        np.testing.assert_array_equal(ds_c[::5], g_s[::5])
        np.testing.assert_array_equal(do_c[::5], g_o[::5])


def test_one_focal_length_is_mip_splattings_compute_3d_filter(cases):
    """Statement for statement, with the screen test at |x - W/2| <= 1.15 W/2 (screen_margin = 0.075) the yardstick IS
    compute_3D_filter.  Mip-Splatting's literal bounds, -0.15 W <= x <= 1.15 W about the image corner, are |x - W/2| <= 1.3 W/2: the
    two differ on the Gaussians that project between 1.15 and 1.3 half-images from the centre, and only there -- with those left
    out of the scene, the literal transcription gives the same filter."""
    for name, c in cases.items():
        if name == "mixed":
            continue
        means, sm = c["scene"]["means"], c["sampling"]
        np.testing.assert_allclose(R.mip_splatting_compute_3d_filter(means, c["cams"], 0.075), sm["filter_3d"], rtol=1e-13, err_msg=name)
        # pairs inside the band: in front, inside the literal screen, outside the header's
        per_view_differs = np.zeros_like(sm["seen"])
        for v, k in enumerate(c["cams"]):
            a = R.sampling_f64(means, [k])
            per_view_differs[v] = a["seen"][0] != _seen_literal(means, k, 0.15)
        keep = ~per_view_differs.any(0)
        if keep.any():
            sub = means[keep]
            np.testing.assert_allclose(R.mip_splatting_compute_3d_filter(sub, c["cams"], 0.15), R.sampling_f64(sub, c["cams"])["filter_3d"],
                                       rtol=1e-13, err_msg=name)


def _seen_literal(means, cam, margin):
    M, focal, W, H = R.view_records([cam])[0]
    p = torch.as_tensor(np.asarray(means, np.float32).astype(np.float64)) @ M[:3, :3] + M[3, :3][None, :]
    z = torch.clamp(p[:, 2], min=0.001)
    x, y = p[:, 0] / z * focal + W / 2.0, p[:, 1] / z * focal + H / 2.0
    return ((p[:, 2] > 0.2) & (x >= -margin * W) & (x <= (1 + margin) * W) & (y >= -margin * H) & (y <= (1 + margin) * H)).numpy()
