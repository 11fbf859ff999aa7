#!/usr/bin/env python3
"""The bits of every stage that walks a finished frame's tile lists (csrc/frame_walk.h: features.hip, distortion.hip,
normal_render.hip, plane_depth.hip and the two depth models of median_depth.hip), for comparing two builds of the library: their
kernels through the C ABI only on frames built on the host from a seed (tests/frame_walk_frames.py: STAGES and DEPTH_STAGES), and one
JSON line of name -> sha256 of each output buffer.
    GSR_LIB=ab/lib_parent.so python tools/frame_walk_bits.py > parent.json;  python tools/frame_walk_bits.py > new.json;  cmp parent.json new.json
Forwards: masks NULL / all 0xFF / seeded random, 50 x 37 and 64 x 48 (partial tiles), lists of 0, 1, 255, 256, 257 and 640 entries,
n_contrib anywhere within the list (multiples of 32, 4, 3 and not), ids < 0 and >= N, D = 0, features at C = 1, 3, 32, 33, 64, packed
arrays and the 16-float record view.  Backwards: they end in float atomics, so they are hashed where no destination receives more
than two addends (frame_walk_frames.BACKWARD_SHAPES): one tile, a 640-entry list with every Gaussian listed once, one wave with
pixels on seeded accumulators, two waves on zeroed ones."""
import hashlib
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
gsr = importlib.import_module("3dgs-native_amd")
import frame_walk_frames as FW               # noqa: E402  (the frames live with the tests)

OUT = {}
CHANNELS = (1, 3, 32, 33, 64)


def put(name, tensors):
    for k, t in enumerate(tensors):
        OUT[f"{name}[{k}]"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def stage_calls(tag, dev_frame, backward, seeded=False):
    for stage in FW.STAGES + FW.DEPTH_STAGES:
        for Cn in CHANNELS if stage == "features" else (3,):
            name = f"{stage}{' C=%d' % Cn if stage == 'features' else ''} {tag}"
            put(name + " forward", dev_frame.forward(stage, Cn))
            if backward:
                put(name + " backward", dev_frame.backward(stage, Cn, seeded))


def main():
    assert torch.cuda.is_available(), "frame_walk_bits needs the GPU"
    torch.cuda.set_device(0)
    seed = 0
    for W, H in ((50, 37), (64, 48)):
        for masks in (None, "ff", "random"):
            for record_view in (False, True):
                seed += 1
                stage_calls(f"{W}x{H} masks={masks} record_view={record_view}", FW.DeviceFrame(FW.build_frame(seed, W, H, masks=masks, record_view=record_view)), False)
    stage_calls("50x37 D=0", FW.DeviceFrame(FW.build_frame(90, 50, 37, lens=(0,), masks=None)), True)   # nothing walked: zeros, accumulators untouched
    for tag, shape in FW.BACKWARD_SHAPES.items():
        for masks in (None, "random"):
            seed += 1
            fr = FW.build_frame(seed, lens=(640,), masks=masks, once_per_tile=True, **shape)
            stage_calls(f"{tag} masks={masks}", FW.DeviceFrame(fr), True, seeded=tag == "8x8")
    torch.cuda.synchronize()
    print(json.dumps(dict(sorted(OUT.items()))), flush=True)


if __name__ == "__main__":
    main()
