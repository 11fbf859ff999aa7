"""What backward() decides about the state render_gaussians() left on its frame, row by row: which of the forward's records, block
masks, d(colour)/d(direction) sums, Sigma3D recompute and pre-cleared workspace one call may use, and which frames it refuses.

Written against the public call surface and the five `backward.last_call_*` flags only.  It asserts decisions, not values: the
blend backward sums with float atomics, so gradients are not bitwise repeatable, and the value tests of this suite hold them.

The shape is the smallest at which every branch is live: 300 Gaussians (not a multiple of 4: the arena's padding branch; more than
one workgroup), 40 x 24 pixels (partial tiles in a 3 x 2 grid), SH degree 3, device tensors used in place.  One forward and
backward run first, so the forward's pre-clear of the backward workspace is armed."""
import numpy as np
import pytest
import torch

from conftest import backward_kwargs, lego_camera, pkg, render_kwargs, sub

pytestmark = pytest.mark.gpu
N, W, H = 300, 40, 24
NAMES = ("used_forward_records", "used_forward_masks", "used_forward_sh_dir", "recomputed_sigma3d", "skipped_the_clear")
ALL = "TTTTT"       # (records, masks, sh_dir, sigma recompute, skipped clear)


def flags():
    bwd = sub("backward").backward
    return "".join("T" if getattr(bwd, "last_call_" + n) else "F" for n in NAMES)


def expect(row):
    """`row` where the pre-clear is on (the default); without it no call skips its clear."""
    return row if sub("forward").PRECLEAR_BACKWARD else row[:4] + "F"


class Frame:
    """One fresh forward: `dev` the scene as device tensors (numpy arrays with host=True), `buf` the forward's dict, `bkw` the
    keyword arguments that hand it all back to backward()."""

    def __init__(self, scenes, cameras, host=False, host_opacity=False, **options):
        gsr = pkg()
        sc = scenes.synthetic_scene(N, 0.05, 0.6, 7)
        self.cam = cam = lego_camera(cameras, frame=3, width=W, height=H)
        kw = render_kwargs(sc, cam, width=W, height=H)
        up = (lambda a: np.ascontiguousarray(a)) if host else (lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda())
        self.dev = dev = {k: up(sc[k]) for k in ("means", "opacities", "scales", "rotations")}
        dev["shs"] = up(sc["shs"].reshape(-1, 3))
        if host_opacity:
            dev["opacities"] = np.ascontiguousarray(sc["opacities"])
        kw.update(means3D=dev["means"], opacity=dev["opacities"], scales=dev["scales"], rotations=dev["rotations"], sh=dev["shs"])
        self.kw = kw
        self.out = gsr.render_gaussians(**kw, **options)
        self.buf = self.out[2]
        dpix = torch.full((H, W, 3), 1.0 / (H * W * 3), device="cuda")
        self.bkw = backward_kwargs(dev, cam, kw, self.buf, dpix)

    def backward(self, **changes):
        """backward() on this frame with `changes` to its keywords; a key of one of the three buffer dicts replaces that entry too."""
        bkw = dict(self.bkw)
        for k, v in changes.items():
            inside = [d for d in ("geom_buffer", "binning_buffer", "img_buffer") if k in bkw[d]]
            for d in inside:
                bkw[d] = dict(bkw[d], **{k: v})
            if k in bkw or not inside:
                bkw[k] = v
        return pkg().backward(**bkw)


@pytest.fixture(scope="module", autouse=True)
def armed(scenes, cameras):
    """One forward and backward before the first row: from then on this process's forwards pre-clear the backward workspace."""
    Frame(scenes, cameras).backward()
    torch.cuda.synchronize()


def _shs_written(f):
    f.dev["shs"].mul_(1)


def _means_written_by_the_library(f):
    sub("_host").written_in_place(f.dev["means"])


def _n_contrib_written(f):
    f.buf["n_contrib"].add_(0)


def _scales_written(f):
    f.dev["scales"].add_(0)


ROWS = [
    # (row, what happens between the forward and the backward, changed keywords of backward(), expected flags)
    ("own_dict", None, lambda f: {}, ALL),
    ("means2D_clone", None, lambda f: {"means2D": f.buf["points_xy_image"].clone()}, "FFTTT"),
    ("ranges_clone", None, lambda f: {"ranges": f.buf["ranges"].clone()}, "TFTTT"),
    ("n_contrib_written", _n_contrib_written, lambda f: {}, "TFTTT"),
    ("shs_written", _shs_written, lambda f: {}, "TTFTT"),
    ("means3D_written_by_the_library", _means_written_by_the_library, lambda f: {}, "TTFTT"),
    ("another_campos", None, lambda f: {"campos": np.asarray(f.cam["camera_center"], np.float32) + np.float32(0.25)}, "TTFTT"),
    ("another_degree", None, lambda f: {"degree": 2}, "TTFTT"),
    ("another_scale_modifier", None, lambda f: {"scale_modifier": 1.5}, "TTTFT"),
    ("cov3Ds_clone", None, lambda f: {"cov3Ds": f.buf["cov3Ds"].clone()}, "TTTFT"),
    ("scales_written", _scales_written, lambda f: {}, "TTTFT"),
]


@pytest.mark.parametrize("row,between,changes,expected", ROWS, ids=[r[0] for r in ROWS])
def test_what_one_change_costs(scenes, cameras, row, between, changes, expected):
    f = Frame(scenes, cameras)
    if between is not None:
        between(f)
    out = f.backward(**changes(f))
    assert flags() == expect(expected), row
    assert out["dL_dmean3D"].shape == (N, 3)


def test_a_second_backward_clears_for_itself(scenes, cameras):
    f = Frame(scenes, cameras)
    f.backward()
    assert flags() == expect(ALL)
    f.backward()
    assert flags() == "TTTTF"


def test_host_arrays_keep_the_records_only(scenes, cameras):
    """Every input a numpy array: nothing to recognise again, so no direction sums and no Sigma3D recompute; the frame's own
    buffers still are device tensors."""
    f = Frame(scenes, cameras, host=True)
    f.backward()
    assert flags() == expect("TTFFT")


def test_a_capacity_frame_hands_over_like_a_sized_one(scenes, cameras):
    gsr = pkg()
    sized = Frame(scenes, cameras)
    D = int(sized.buf["point_list"].shape[0])
    assert D > 0
    f = Frame(scenes, cameras, capacity=4 * D + 64)
    assert gsr.forward.rendered_count(f.buf) == (D, False)
    f.backward()
    assert flags() == expect(ALL)


@pytest.mark.parametrize("host_opacity", [False, True], ids=["device_opacity", "numpy_opacity"])
def test_an_antialiased_frame_is_recognised(scenes, cameras, host_opacity):
    f = Frame(scenes, cameras, host_opacity=host_opacity, rasterize_mode="antialiased")
    out = f.backward(rasterize_mode="antialiased")
    assert flags() == expect(ALL)
    assert out["dL_dopacity"].shape == (N,)


def test_an_antialiased_frame_is_refused_when_stale_or_mixed_up(scenes, cameras):
    aa = Frame(scenes, cameras, rasterize_mode="antialiased")
    classic = Frame(scenes, cameras)
    with pytest.raises(ValueError, match="not a copy of it and not a classic frame"):
        classic.backward(rasterize_mode="antialiased")
    with pytest.raises(ValueError, match="pass the same mode"):
        aa.backward()
    aa.dev["opacities"].mul_(1)
    with pytest.raises(ValueError, match="written in place since"):
        aa.backward(rasterize_mode="antialiased")


def test_a_filtered_frame_is_recognised_or_refused(scenes, cameras):
    filt = torch.full((N,), 0.01, device="cuda")
    f = Frame(scenes, cameras, filter_3d=filt)
    out = f.backward(filter_3d=filt)                 # the raw scales and opacity again
    assert flags() == expect(ALL)
    assert out["dL_dscale"].shape == (N, 3)
    with pytest.raises(ValueError, match="pass the same tensor"):
        f.backward()
    with pytest.raises(ValueError, match="another filter tensor"):
        f.backward(filter_3d=filt.clone())
    filt.add_(0)
    with pytest.raises(ValueError, match="filter_3d was written in place"):
        f.backward(filter_3d=filt)
