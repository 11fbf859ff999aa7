"""
The camera gradient of the distortion term and of the consistency term's normal image, each ALONE, on the MI355X.

tests/test_gpu_train_step.py S7 and S9 see these gradients only next to the colour term's.  Here, on the two frames of
tests/test_gpu_distortion.py / tests/test_gpu_normal_render.py whose lists pass 512 entries and whose tiles are partial (n2000_64x48,
classic and antialiased: the smallest on file), the 35 floats of

    backward(dL_dpixels=None, dL_ddistortion=g, distortion_moments=..., camera_grad=True)
    backward(dL_dpixels=None, dL_dnormal_image=G, gaussian_normals=..., normal_image=..., camera_grad=True)

are held to step_reference.camera_gradient_f64 by tests/test_gpu_camera_grads.py's criterion, per float:
|kernel - f64| <= TRIP x sum |f64 term|.  g and G are distortion_reference.draw_g and normal_render_reference.draw_G, zero at the
pixels those yardsticks mask.  The normals are constants of the camera on both sides: the library's contract
(include/gsr_normal_render.h (b)); tests/test_step_reference.py measures what that leaves out.  The run-to-run spread of two calls
is printed beside the error, in the same units, and must itself stay inside TRIP (it does by three orders: no wider form of the
bound is needed).  Measured on the MI355X, |kernel - f64| / sum|term| and the spread of two calls: distortion 2.9e-7 / 1.0e-7
(n2000_64x48) and 4.0e-7 / 6.4e-8 (antialiased); normal image 3.5e-7 / 1.7e-8 and 2.7e-7 / 2.3e-8; TRIP is 8.9e-4.
"""
import numpy as np
import pytest

from conftest import sub
import parity
import step_reference as S
import test_gpu_distortion as TD
import test_gpu_normal_render as TN
from test_gpu_camera_grads import TRIP, _cam36

pytestmark = pytest.mark.gpu


def _hold(name, term, calls, ref, scale):
    a, b = calls
    assert np.isfinite(a).all() and np.abs(ref[:35]).max() > 0
    zero = scale == 0
    assert not np.any(a[zero]), np.where(zero & (a != 0))[0]
    err = float((np.abs(a - ref)[~zero] / scale[~zero]).max())
    spread = float((np.abs(a - b)[~zero] / scale[~zero]).max())
    print(f"\n{name} {term}: |kernel - f64| / sum|term| {err:.2e} (TRIP {TRIP:.2e}), two calls differ by {spread:.2e}")
    assert spread <= TRIP, (spread, "the run-to-run spread alone passes the bound")
    assert err <= TRIP, (err, a, ref)


@pytest.mark.parametrize("name", ["n2000_64x48", "n2000_antialiased"])
def test_distortion_term_alone_camera_gradient_against_float64(name):
    f = TD.frame(name)
    H, W = f["H"], f["W"]
    _, mom = sub("distortion").render_distortion(f["buf"], H, W)
    calls = [_cam36(TD._backward(f, None, f["gd"], mom, camera_grad=True)) for _ in range(2)]
    lists = {k: parity.to_np(f["buf"][k]) for k in ("radii", "point_list", "ranges")}
    ref, scale = S.camera_gradient_f64(f["sc"], f["kw"], lists["radii"], lists["point_list"], lists["ranges"],
                                       antialiased=name == "n2000_antialiased", g_dist=f["g"])
    _hold(name, "distortion", calls, ref, scale)


@pytest.mark.parametrize("name", ["n2000_64x48", "n2000_antialiased"])
def test_normal_image_term_alone_camera_gradient_against_float64(name):
    f = TN.frame(name)
    H, W = f["H"], f["W"]
    nimg = sub("normal_render").render_normals(f["n"], f["buf"], H, W)
    calls = [_cam36(TN._backward(f, None, f["Gd"], nimg, camera_grad=True)) for _ in range(2)]
    lists = {k: parity.to_np(f["buf"][k]) for k in ("radii", "point_list", "ranges")}
    ref, scale = S.camera_gradient_f64(f["sc"], f["kw"], lists["radii"], lists["point_list"], lists["ranges"],
                                       antialiased=name == "n2000_antialiased", gN=f["G"], normals=f["n32"])
    _hold(name, "normal image", calls, ref, scale)
