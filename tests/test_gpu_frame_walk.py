"""The contracts of the shared frame-list walk (csrc/frame_walk.h), stated once for the three stages built on it and for both
directions: nothing here is compared against the code under test, only the code against itself and against exact zeros.
Frames come from tests/frame_walk_frames.py; the backwards run only where no destination receives more than two addends, so
that their float atomics give the same bits every call."""
import numpy as np
import pytest
import torch

import frame_walk_frames as FW

pytestmark = pytest.mark.gpu

SHAPES = dict(FW.BACKWARD_SHAPES, **{"50x37": dict(W=50, H=37)})   # the last one: forwards only (several tiles, partial ones)


def frame(tag, **kw):
    shape = SHAPES[tag]
    if tag in FW.BACKWARD_SHAPES:
        return FW.build_frame(11, lens=(640,), once_per_tile=True, **shape, **kw)
    return FW.build_frame(12, **shape, **kw)


CHANNELS = {"features C=3": 3, "features C=33": 33}   # features_kernel<1, *> and <2, *>


def run(fr, stage, direction, seeded):
    d = FW.DeviceFrame(fr)
    stage, Cn = stage.split()[0], CHANNELS.get(stage, 3)
    out = d.forward(stage, Cn) if direction == "forward" else d.backward(stage, Cn, seeded)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def same_bits(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


CASES = [(tag, stage, direction) for tag in SHAPES for stage in (*CHANNELS, *FW.STAGES[1:]) for direction in ("forward", "backward")
         if direction == "forward" or tag in FW.BACKWARD_SHAPES]


@pytest.mark.parametrize("tag,stage,direction", CASES)
def test_walk_contracts(tag, stage, direction):
    seeded = tag == "8x8"   # one wave adds: a seeded accumulator takes one addend per destination
    fr = frame(tag, masks=None)
    ref = run(fr, stage, direction, seeded)
    assert all(np.isfinite(x).all() for x in ref)
    assert any(np.any(x != 0) for x in ref), "the frame must exercise the walk"
    assert same_bits(ref, run(fr, stage, direction, seeded)), "a second call gives the same bits"
    assert same_bits(ref, run(frame(tag, masks="ff"), stage, direction, seeded)), "masks all 0xFF give the bits of masks NULL"
    assert fr["bad"].sum() >= 2
    assert same_bits(ref, run(FW.other_bad_ids(fr, 5), stage, direction, seeded)), "an out-of-range id is skipped whatever its value"
    if direction == "forward":
        none = fr["n_contrib"] == 0
        assert none.any() and not none.all()
        for x in ref:
            assert np.all(x[none].view(np.uint32) == 0), "a pixel with n_contrib = 0 is written as exactly 0"
    else:
        past = FW.past_every_pixel(fr)
        assert past.sum() >= FW.PAST // 2
        start = fr["acc_seed"] if seeded else np.zeros_like(fr["acc_seed"])
        for x in ref:
            before = start if x.shape[1] == 16 else np.zeros_like(x)   # the accumulator records; dL_dF and dL_dnormals start cleared
            assert x[past].tobytes() == before[past].tobytes(), "a Gaussian past every pixel's n_contrib receives exactly 0"
            assert np.any(x[~past] != before[~past])
