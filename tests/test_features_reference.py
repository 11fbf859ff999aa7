"""
The yardstick of N-channel feature rendering (tests/features_reference.py) checked on the CPU oracle's buffers.  No GPU.

  1. the helper's dL_dF is torch autograd of its own dense forward;
  2. with F = [colours, 1, 1 / depth] the five channels reproduce the oracle's image (background 0), 1 - final_Ts and the
     inverse-depth image on the unmasked pixels: measured on the four scenes at most 4.4e-7, 4.6e-7 and 2.0e-7; 2e-6 is asserted,
     four times the worst (the oracle's float32 error against the float64 weights is all that separates them);
  3. at most 1 % of a scene's pixels are masked, and the scenes are what the GPU test needs of them (list lengths, n_contrib);
  4. with the float32 restatement as the checked side, the backward criterion E <= 3 max(E_f32, E_spread) + floor rejects a dropped
     list entry at positions 63, 64, 255 and 256 and a dropped 8x4 block, and accepts the intact restatement; the floor on file
     (tests/golden/features_margins.json) is the smallest E_f32 of this matrix.
"""
import numpy as np
import pytest
import torch

import features_reference as FR

C_CPU = 3
_CASES = {}


def oracle_case(oracle, scenes, cameras, name):
    """{sc, kw, W, H, image, inv_depth, buf (the oracle's forward, background 0), F, G, r}, once per session."""
    if name not in _CASES:
        sc, cam, kw = FR.scene(scenes, cameras, name)
        H, W = kw["image_height"], kw["image_width"]
        image, inv_depth, buf = oracle.render_gaussians(**kw)
        N = sc["means"].shape[0]
        F, G = FR.draw(N, C_CPU, H, W)
        _CASES[name] = dict(sc=sc, kw=kw, W=W, H=H, image=np.asarray(image), inv_depth=np.asarray(inv_depth), buf=buf, F=F, G=G,
                            r=FR.render(buf, W, H, F, G))
    return _CASES[name]


@pytest.mark.parametrize("name", list(FR.SCENES))
def test_dL_dF_is_autograd_of_the_dense_forward(oracle, scenes, cameras, name):
    c = oracle_case(oracle, scenes, cameras, name)
    r = c["r"]
    F = torch.tensor(c["F"].astype(np.float64), requires_grad=True)
    G = torch.as_tensor(c["G"].astype(np.float64))
    loss = torch.zeros((), dtype=torch.float64)
    out = np.zeros_like(r["out64"])
    for _, xs, ys, idx, w, masked in r["tiles"]:
        o = torch.as_tensor(w) @ F[torch.as_tensor(idx)]
        out[ys, xs] = o.detach().numpy()
        g = torch.where(torch.as_tensor(masked)[:, None], torch.zeros((), dtype=torch.float64), G[ys, xs])
        loss = loss + (o * g).sum()
    (dF,) = torch.autograd.grad(loss, F)
    assert np.abs(out - r["out64"]).max() <= 1e-13                # (two float64 matrix products: the order inside is the library's)
    e = FR.backward_error(dF.numpy(), r)
    assert e <= 1e-12, e                                    # float64 sums in two orders, in units of the terms' magnitude
    assert np.abs(r["dF64"]).max() > 0 and np.all(np.abs(r["dF64"]) <= r["mag"] * (1 + 1e-12))
    unused = np.asarray(c["buf"]["radii"]).reshape(-1) == 0
    assert not r["dF64"][unused].any() and not r["mag"][unused].any()      # a culled Gaussian gets exactly nothing


@pytest.mark.parametrize("name", list(FR.SCENES))
def test_colour_alpha_and_depth_channels_reproduce_the_oracle(oracle, scenes, cameras, name):
    c = oracle_case(oracle, scenes, cameras, name)
    buf, W, H = c["buf"], c["W"], c["H"]
    depths = np.asarray(buf["depths"], np.float64).reshape(-1)
    inv = np.where(depths > 0, 1.0 / np.where(depths > 0, depths, 1.0), 0.0)
    F5 = np.concatenate([np.asarray(buf["colors"], np.float64).reshape(-1, 3), np.ones((len(inv), 1)), inv[:, None]], 1)
    out = np.zeros((H, W, 5))
    for _, xs, ys, idx, w, _ in c["r"]["tiles"]:
        out[ys, xs] = w @ F5[idx]
    keep = ~c["r"]["mask"]
    e_img = np.abs(out[..., :3] - c["image"].reshape(H, W, 3))[keep].max()
    e_alpha = np.abs(out[..., 3] - (1.0 - np.asarray(buf["final_Ts"], np.float64).reshape(H, W)))[keep].max()
    e_depth = np.abs(out[..., 4] - c["inv_depth"].reshape(H, W))[keep].max()
    print(f"\n{name}: image {e_img:.2e}, 1 - final_Ts {e_alpha:.2e}, inverse depth {e_depth:.2e}")
    assert max(e_img, e_alpha, e_depth) <= 2e-6


def test_the_four_scenes_are_what_the_gpu_test_needs(oracle, scenes, cameras):
    seen = {}
    for name in FR.SCENES:
        c = oracle_case(oracle, scenes, cameras, name)
        r, nc = c["r"], np.asarray(c["buf"]["n_contrib"])
        masked = int(r["mask"].sum())
        seen[name] = (r["D"], r["longest"], int(nc.max()), masked)
        print(f"\n{name}: D {r['D']}, longest list {r['longest']}, largest n_contrib {int(nc.max())}, masked {masked} of {r['mask'].size}")
        assert masked <= FR.MAX_MASKED * r["mask"].size
        assert np.array_equal(r["n_contrib64"][~r["mask"]], nc.reshape(c["H"], c["W"])[~r["mask"]])
    assert seen["n300_50x37"][1] > 64
    assert seen["n900_faint_48x32"][1] > 512 and seen["n900_faint_48x32"][2] > 512        # past two 256-entry batches, unsaturated
    assert seen["n1500_opaque_48x48"][1] > 2 * seen["n1500_opaque_48x48"][2]              # early saturation


def _e_f32(c):
    return FR.backward_error(c["r"]["dF32"], c["r"])


def test_floor_on_file_is_the_smallest_f32_margin(oracle, scenes, cameras):
    E = {n: _e_f32(oracle_case(oracle, scenes, cameras, n)) for n in FR.SCENES}
    Ef = {n: FR.forward_error(oracle_case(oracle, scenes, cameras, n)["r"]["out32"], oracle_case(oracle, scenes, cameras, n)["r"],
                              oracle_case(oracle, scenes, cameras, n)["F"]) for n in FR.SCENES}
    floor = FR.golden()["floor"]
    print("\nE_f32 backward " + ", ".join(f"{n} {v:.3e}" for n, v in E.items()) + f"; floor on file {floor:.3e}")
    print("E_f32 forward " + ", ".join(f"{n} {v:.3e}" for n, v in Ef.items()))
    assert all(np.isfinite(v) and v > 0 for v in E.values())
    assert floor <= 2.0 * min(E.values())                 # (the libm's expf may differ from the one it was recorded with)
    assert all(FR.forward_criterion(v, v) for v in Ef.values())


@pytest.mark.parametrize("what", [63, 64, 255, 256, "block"])
def test_the_criterion_sees_a_dropped_term(oracle, scenes, cameras, what):
    """The term is dropped where it is a whole share of its Gaussian's row: the tile whose entry at that list position carries the
    most weight at unmasked pixels."""
    name = "n900_faint_48x32"
    c = oracle_case(oracle, scenes, cameras, name)
    r, floor = c["r"], FR.golden()["floor"]
    ranges = np.asarray(c["buf"]["ranges"]).reshape(-1, 2)
    pos = 100 if what == "block" else what
    best = None
    for tile, xs, ys, idx, w, masked in r["tiles"]:
        if w.shape[1] <= pos:
            continue
        blk = ((ys % 16) // 4) * 2 + (xs % 16) // 8
        per_block = np.array([w[blk == b, pos].sum() for b in range(8)])
        score = per_block.max() if what == "block" else per_block.sum()
        if best is None or score > best[0]:
            best = (score, int(ranges[tile, 0]) + pos, int(per_block.argmax()))
    assert best is not None and best[0] > 0
    drop = ("block", best[1], best[2]) if what == "block" else ("entry", best[1])
    dropped = FR.render(c["buf"], c["W"], c["H"], c["F"], c["G"], drops=(drop,))
    assert np.array_equal(dropped["dF32"], r["dF32"])
    E_f32, E = _e_f32(c), FR.backward_error(dropped["dF32_dropped"][0], r)
    print(f"\n{drop}: E = {E:.3e} against E_f32 {E_f32:.3e}, floor {floor:.3e}")
    assert FR.backward_criterion(E_f32, E_f32, 0.0, floor)                # the intact restatement passes
    assert not FR.backward_criterion(E, E_f32, 0.0, floor)
    assert E > 100 * (3.0 * E_f32 + floor)
