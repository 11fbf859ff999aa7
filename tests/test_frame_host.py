"""CPU-side checks of the host frame record (_frame.py, the host counterpart of csrc/frame_walk.h) and of backward()'s stage table:
both constructors fill the same struct fields for the same arrays, the table lists the stages in the order they run under keywords
backward() takes, and the three "needs geom_buffer['depths']" refusals come out of the table word for word."""
import inspect

import pytest
import torch

from abi_helpers import OnDevice
from conftest import pkg, sub

N, H, W, D = 8, 20, 33, 50
TILES = 3 * 2


def _fields(s):
    return {k: getattr(s, k) for k, _ in s._fields_}


@pytest.fixture()
def frame(monkeypatch):
    """A forward's own buffers, as forward.py tags them (records behind the column views, block masks behind the list), and the arrays
    backward() would hand to the second constructor."""
    _lib, _host = sub("_lib"), sub("_host")

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    dev = lambda t: t.as_subclass(OnDevice)
    i32 = torch.int32
    rec = dev(torch.zeros(N, 16))
    xy, co, rgb = rec[:, 0:2], rec[:, 2:6], rec[:, 6:9]
    pl, rg, nc = dev(torch.zeros(D, dtype=i32)), dev(torch.zeros(TILES, 2, dtype=i32)), dev(torch.zeros(H, W, dtype=i32))
    masks = dev(torch.zeros(D, dtype=torch.uint8))
    xy._gsr_records = (rec, {"means2D": _host.stamp(xy), "conic_opacity": _host.stamp(co), "rgb": _host.stamp(rgb)})
    pl._gsr_block_masks = (masks, {"ranges": _host.stamp(rg), "n_contrib": _host.stamp(nc), "means2D": _host.stamp(xy),
                                   "conic_opacity": _host.stamp(co)}, None)
    buffers = {"points_xy_image": xy, "conic_opacity": co, "colors": rgb, "point_list": pl, "ranges": rg, "n_contrib": nc}
    return buffers, rec, pl, rg, nc, masks


def test_both_constructors_fill_the_same_struct(frame):
    _lib, Frame = sub("_lib"), sub("_frame").Frame
    buffers, rec, pl, rg, nc, masks = frame
    for use_masks in (True, False):
        for inv_depth in (True, False):
            a = Frame.from_buffers(buffers, H, W, use_masks, inv_depth=inv_depth)
            b = Frame.from_records(rec, pl, rg, nc, masks if use_masks else None)
            sa, sb = a.struct(), b.struct(inv_depth=inv_depth)
            kind = _lib.GsrDistortionFrame if inv_depth else _lib.GsrFeaturesFrame
            assert type(sa) is kind and type(sb) is kind                  # 1 / depth asked for: the distortion's frame, else the features'
            fa = _fields(sa)
            assert fa == _fields(sb)
            assert (fa["W"], fa["H"], fa["N"], fa["D"]) == (W, H, N, D)
            assert (fa["xy"], fa["xy_stride"]) == (rec.data_ptr(), 16)
            assert (fa["conic_opacity"], fa["conic_opacity_stride"]) == (rec.data_ptr() + 8, 16)
            assert (fa["point_list"], fa["ranges"], fa["n_contrib"]) == (pl.data_ptr(), rg.data_ptr(), nc.data_ptr())
            assert fa["block_masks"] == (masks.data_ptr() if use_masks else None)
            if inv_depth:
                assert (fa["inv_depth"], fa["inv_depth_stride"]) == (rec.data_ptr() + 36, 16)
            assert (a.N, a.D, a.W, a.H, a.device) == (b.N, b.D, b.W, b.H, b.device)
    assert type(Frame.from_records(rec, pl, rg, nc, None).struct()) is _lib.GsrDistortionFrame    # the records always carry 1 / depth


def test_packed_arrays_and_foreign_buffers(frame):
    _lib, Frame = sub("_lib"), sub("_frame").Frame
    buffers, rec, pl, rg, nc, masks = frame
    dev = lambda t: t.as_subclass(OnDevice)
    xy, co, depths = dev(torch.zeros(N, 2)), dev(torch.zeros(N, 4)), dev(torch.tensor([0.0, -1.0, 2.0, 4.0, 1.0, 1.0, 1.0, 1.0]))
    packed = dict(buffers, points_xy_image=xy, conic_opacity=co, depths=depths)       # clones: no records tag, and the masks' stamps do not hold
    fr = Frame.from_buffers(packed, H, W, True, inv_depth=True)
    s = fr.struct()
    assert type(s) is _lib.GsrDistortionFrame
    assert (s.xy, s.xy_stride, s.conic_opacity, s.conic_opacity_stride) == (xy.data_ptr(), 2, co.data_ptr(), 4)
    assert s.block_masks is None and (s.inv_depth, s.inv_depth_stride) == (fr.inv_depth.data_ptr(), 1)
    assert fr.inv_depth.tolist() == [0.0, 0.0, 0.5, 0.25, 1.0, 1.0, 1.0, 1.0]         # 1 / depth, 0 where the depth is not positive
    assert type(Frame.from_buffers(packed, H, W).struct()) is _lib.GsrFeaturesFrame
    with pytest.raises(ValueError, match=r"buffers\['depths'\] must be a float32 device tensor of shape \(N,\)"):
        Frame.from_buffers(dict(packed, depths=None), H, W, inv_depth=True)
    empty = dict(packed, points_xy_image=dev(torch.zeros(0, 2)), conic_opacity=dev(torch.zeros(0, 4)), depths=None)
    assert Frame.from_buffers(empty, H, W, inv_depth=True).inv_depth is None            # a frame with no Gaussians never needs depths


def test_stage_table_order_and_keywords():
    bw, nr, _lib = sub("backward"), sub("normal_render"), sub("_lib")
    assert [s.name for s in bw.STAGES] == ["distortion", "normal", "plane", "median"]
    params = inspect.signature(pkg().backward).parameters
    dev = lambda t: t.as_subclass(OnDevice)
    hw, hw3, n3 = dev(torch.zeros(H, W)), dev(torch.zeros(H, W, 3)), dev(torch.zeros(N, 3))
    values = {"dL_ddistortion": hw, "distortion_moments": dev(torch.zeros(H, W, 4)), "dL_dnormal_image": hw3, "gaussian_normals": n3,
              "normal_image": hw3, "dL_dplane_depth": hw, "plane_slopes": dev(torch.zeros(N, 2)), "plane_depth_image": hw,
              "dL_dmedian_depth": hw, "median_contributor": dev(torch.zeros(H, W, dtype=torch.int32))}
    for s in bw.STAGES:
        for k in s.keywords + (() if s.param_grad is None else (s.param_grad,)):
            assert k in nr.STAGE_KEYWORDS or params[k].kind is inspect.Parameter.KEYWORD_ONLY, (s.name, k)
        # the stage's inputs function takes the keywords' values by their names, in the order its check does
        assert tuple(inspect.signature(s.inputs).parameters)[5:] == s.keywords == tuple(inspect.signature(s.check).parameters)
        assert (s.follow_up is None) == (s.param_grad is None) and (s.follow_up is None or s.result is not None)
        tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS")]
        argtypes = next(t[s.entry] for t in tables if s.entry in t)[1]                     # an entry point _lib binds, called with
        arrays = s.inputs(torch.device("cpu"), N, H, W, values["gaussian_normals"], *(values[k] for k in s.keywords))
        assert len(argtypes) == 1 + len(arrays) + 1 + (s.result is not None) + 1            # frame, inputs, accumulators[, result], stream
        assert all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in arrays)
    assert {s.name for s in bw.STAGES if s.follow_up is not None} == set(bw.FOLLOW_UP_ORDER) and bw.FOLLOW_UP_ORDER == ("plane", "normal")
    assert [s.name for s in bw.STAGES if s.depths_reason is None] == ["normal"]


def test_needs_depths_messages_come_from_the_table_word_for_word():
    bw = sub("backward")
    parent = {
        "distortion": "backward(dL_ddistortion=...) on a frame that does not carry the forward's records needs "
                      "geom_buffer['depths']: the distortion is a function of the Gaussians' inverse depths",
        "plane": "backward(dL_dplane_depth=...) on a frame that does not carry the forward's records needs "
                 "geom_buffer['depths']: the plane depth is a function of the Gaussians' inverse depths",
        "median": "backward(dL_dmedian_depth=...) on a frame that does not carry the forward's records needs "
                  "geom_buffer['depths']: the per-Gaussian half carries dL/d(1/depth) on through the re-packed records",
    }
    made = {s.name: bw._needs_depths(s) for s in bw.STAGES if s.depths_reason is not None}
    assert set(made) == set(parent)
    for name, e in made.items():
        assert isinstance(e, ValueError) and str(e) == parent[name]
