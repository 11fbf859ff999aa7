"""The shared argument validators (_args.py), called directly: each accepts the valid forms and refuses each invalid one with a
ValueError that names the argument.  Device tensors are abi_helpers.OnDevice stand-ins: nothing here touches the library or a GPU."""
import numpy as np
import pytest
import torch

from abi_helpers import OnDevice
from conftest import sub

NAN, INF = float("nan"), float("inf")


def dev(t, index=None):
    if index is None:
        return t.as_subclass(OnDevice)
    return t.as_subclass(type("T", (OnDevice,), {"device": torch.device("cuda", index)}))


def refused(call, *args, **kw):
    """The call raises a ValueError that names the argument "x"."""
    with pytest.raises(ValueError, match=r"\bx\b"):
        call(*args, **kw)


def test_predicates():
    A = sub("_args")
    f32, i32 = torch.float32, torch.int32
    assert A.is_dev(dev(torch.zeros(3)), f32) and A.is_dev(dev(torch.zeros(3, dtype=i32)), i32)
    for bad in (torch.zeros(3), dev(torch.zeros(3, dtype=torch.float64)), np.zeros(3, np.float32), None, [0.0]):
        assert not A.is_dev(bad, f32)
    assert A.is_f32(torch.zeros(2)) and A.is_f32(np.zeros(2, np.float32)) and A.is_f32(dev(torch.zeros(2)))
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float16), np.zeros(2), np.zeros(2, np.int32)):
        assert not A.is_f32(bad)
    base = dev(torch.zeros(4, 12))
    assert A.is_packed(base) and A.is_packed(base, 48) and A.is_packed(base[1], 12) and A.is_packed(dev(torch.zeros(16))[1:13], 12)
    for bad in (torch.zeros(12), dev(torch.zeros(12, dtype=torch.float64)), dev(torch.zeros(24))[::2], dev(torch.zeros(11)), dev(torch.zeros(13)),
                np.zeros(12, np.float32), None):
        assert not A.is_packed(bad, 12)
    assert not A.is_packed(dev(torch.zeros(6, 4)).t())


def test_check_out():
    A = sub("_args")
    A.check_out(dev(torch.zeros(5, 3)), (5, 3), "x")
    A.check_out(dev(torch.zeros(24, 3))[4:9], [5, 3], "x")                              # an offset view, 48 bytes in: aligned
    A.check_out(dev(torch.zeros(5, 3, dtype=torch.int32)), (5, 3), "x", torch.int32)
    A.check_out(dev(torch.zeros(5), 1), (5,), "x", dev=torch.device("cuda", 1))
    for bad in (dev(torch.zeros(5, 3, dtype=torch.float64)), dev(torch.zeros(5, 3, dtype=torch.int32)), torch.zeros(5, 3), np.zeros((5, 3), np.float32),
                None, dev(torch.zeros(5, 6))[:, ::2], dev(torch.zeros(3, 5)).t(), dev(torch.zeros(24, 3))[1:6], dev(torch.zeros(4, 3)), dev(torch.zeros(15)),
                dev(torch.zeros(5, 3, 1))):
        refused(A.check_out, bad, (5, 3), "x")
    refused(A.check_out, dev(torch.zeros(16))[1:6], (5,), "x")                          # misaligned by 4 bytes
    refused(A.check_out, dev(torch.zeros(5, 3)), (5, 3), "x", torch.int32)
    refused(A.check_out, dev(torch.zeros(5), 0), (5,), "x", dev=torch.device("cuda", 1))
    with pytest.raises(ValueError, match="aligned float32 device tensor of shape .5, 3. on cuda:1"):
        A.check_out(None, (5, 3), "x", dev=torch.device("cuda", 1))


def test_check_slot():
    A = sub("_args")
    rows = dev(torch.zeros(3, 4))
    A.check_slot(None, 1, "x")                                                          # no slot given: the call makes its own
    A.check_slot(dev(torch.zeros(1)), 1, "x")
    A.check_slot(dev(torch.zeros(7))[3:4], 1, "x")                                      # an element of a loss curve: 4-byte aligned is enough
    A.check_slot(rows[1], 4, "x", contiguous=True)                                      # a row of a 2-D tensor
    A.check_slot(rows[:, 1:2], 3, "x")                                                  # (strided: fine where no packing is asked for)
    for bad, n in ((torch.zeros(1), 1), (np.zeros(1, np.float32), 1), ([0.0], 1), (dev(torch.zeros(1, dtype=torch.float64)), 1), (dev(torch.zeros(2)), 1),
                   (dev(torch.zeros(0)), 1), (dev(torch.zeros(3)), 4), (dev(torch.zeros(5)), 4)):
        refused(A.check_slot, bad, n, "x")
        refused(A.check_slot, bad, n, "x", contiguous=True)
    refused(A.check_slot, dev(torch.zeros(8))[::2], 4, "x", contiguous=True)
    refused(A.check_slot, rows[:, 1], 3, "x", contiguous=True)
    with pytest.raises(ValueError, match="who: x must be a contiguous 4-element float32 device tensor"):
        A.check_slot(torch.zeros(4), 4, "who: x", contiguous=True)
    with pytest.raises(ValueError, match="who: x must be a 1-element float32 device tensor"):
        A.check_slot(torch.zeros(1), 1, "who: x")


def test_check_one_device():
    A = sub("_args")
    a0, b0, c1 = dev(torch.zeros(2), 0), dev(torch.zeros(3), 0), dev(torch.zeros(2), 1)
    A.check_one_device()
    A.check_one_device(a0, b0, None, np.zeros(2), torch.zeros(2), [1.0])                # host arrays are uploaded: they have no say
    A.check_one_device(c1)
    for bad in ((a0, c1), (a0, None, b0, c1), (c1, torch.zeros(2), a0)):
        with pytest.raises(ValueError, match=r"one device .*cuda:0.*cuda:1"):
            A.check_one_device(*bad)


def test_image_hw():
    A = sub("_args")
    img, img1, rgb = np.zeros((5, 7), np.float32), torch.zeros(5, 7, 1), np.zeros((5, 7, 3), np.float32)
    for ok in (img, img1, dev(torch.zeros(5, 7)), np.zeros((5, 7)), [[0.0] * 7] * 5, dev(torch.zeros(5, 14))[:, ::2]):
        assert A.image_hw(ok, "x") == (5, 7)                                            # the size discovered ...
        assert A.image_hw(ok, "x", (5, 7)) == (5, 7)                                    # ... or known
    assert A.image_hw(rgb, "x", channels=3) == A.image_hw(rgb, "x", (5, 7), 3) == A.image_hw(rgb, "x", (5, 7), 3, f32=True) == (5, 7)
    assert A.image_hw(img, "x", squeeze=False, f32=True) == A.image_hw(torch.zeros(5, 7), "x", f32=True) == (5, 7)
    assert A.image_hw(np.zeros((1, 1, 1), np.float32), "x") == (1, 1)
    for bad in (np.zeros(35, np.float32), rgb, np.zeros((5, 7, 1, 1), np.float32), np.zeros((0, 7), np.float32), np.zeros((5, 0, 1), np.float32),
                np.float32(1.0), None):
        refused(A.image_hw, bad, "x")
    for bad in (np.zeros((7, 5), np.float32), np.zeros((5, 8), np.float32), np.zeros((7, 5, 1), np.float32), np.zeros(35, np.float32), rgb):
        refused(A.image_hw, bad, "x", (5, 7))
    for bad in (img, img1, np.zeros((5, 7, 4), np.float32), np.zeros((5, 7, 3, 1), np.float32), np.zeros((0, 7, 3), np.float32)):
        refused(A.image_hw, bad, "x", channels=3)
    for bad in (img, np.zeros((7, 5, 3), np.float32), np.zeros((5, 7, 4), np.float32)):
        refused(A.image_hw, bad, "x", (5, 7), 3)
    refused(A.image_hw, img1, "x", squeeze=False)                                       # exactly (H, W) where no trailing 1 is taken
    refused(A.image_hw, img1, "x", (5, 7), squeeze=False)
    for bad, what in ((np.zeros((5, 7)), "float32"), (torch.zeros(5, 7, dtype=torch.float16), "float32"), (np.zeros((5, 7), np.int32), "float32"),
                      ([[0.0] * 7] * 5, "tensor or a numpy"), (None, "tensor or a numpy"), (np.zeros(35, np.float32), "shape")):
        with pytest.raises(ValueError, match=r"\bx\b.*" + what):
            A.image_hw(bad, "x", f32=True)
    with pytest.raises(ValueError, match=r"who: x must have shape \(H, W\), not \(35,\)"):
        A.image_hw(np.zeros(35), "who: x")
    with pytest.raises(ValueError, match=r"who: x must have shape \(H, W, 3\), not \(5, 7\)"):
        A.image_hw(img, "who: x", channels=3)
    with pytest.raises(ValueError, match=r"who: x must have shape \(5, 7, 3\) .*, not \(7, 5, 3\)"):
        A.image_hw(np.zeros((7, 5, 3)), "who: x", (5, 7), 3)


def test_scalars():
    A = sub("_args")
    assert A.finite(0, "x") == 0.0 and A.finite(-2.5, "x") == -2.5 and A.finite(np.float32(0.5), "x") == 0.5 and A.finite(torch.tensor(3.0), "x") == 3.0
    assert isinstance(A.finite(1, "x"), float) and isinstance(A.positive(np.float64(1), "x"), float)
    assert A.positive(1e-30, "x") == 1e-30 and A.positive(2, "x") == 2.0 and A.positive(INF, "x", allow_inf=True) == INF
    for bad in (NAN, INF, -INF, "abc", None, [1.0, 2.0]):
        refused(A.finite, bad, "x")
    for bad in (0.0, -0.0, -1.0, NAN, INF, -INF, "abc", None):
        refused(A.positive, bad, "x")
    for bad in (0.0, -1.0, NAN, -INF, "abc", None):
        refused(A.positive, bad, "x", allow_inf=True)
    with pytest.raises(ValueError, match="who: x must be finite, not nan"):
        A.finite(NAN, "who: x")
    with pytest.raises(ValueError, match="who: x must be positive and finite, not 0.0"):
        A.positive(0.0, "who: x")
    with pytest.raises(ValueError, match="who: x must be positive, not -1"):
        A.positive(-1, "who: x", allow_inf=True)


def test_camera_params():
    A = sub("_args")
    cam = {"tan_fovx": 0.5, "tan_fovy": np.float32(0.25), "width": 7, "height": np.int64(5), "world_to_camera": None}
    assert A.camera_params(cam, "x") == (0.5, 0.25, 7, 5)
    assert A.camera_params(dict(cam, width=7.0, height=1 << 25), "x") == (0.5, 0.25, 7, 1 << 25)
    assert [type(v) for v in A.camera_params(cam, "x")] == [float, float, int, int]
    for bad in (None, {}, [0.5, 0.25, 7, 5], {"tan_fovx": 0.5}, dict(cam, tan_fovx=0.0), dict(cam, tan_fovx=-0.5), dict(cam, tan_fovy=NAN),
                dict(cam, tan_fovy=INF), dict(cam, width=0), dict(cam, height=-1), dict(cam, height=2.5), dict(cam, width=1 << 14, height=(1 << 14) + 1)):
        refused(A.camera_params, bad, "x")


def test_the_module_needs_neither_the_library_nor_a_gpu(monkeypatch):
    _lib, A = sub("_lib"), sub("_args")

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    monkeypatch.setattr(torch.cuda, "is_available", no_lib)
    A.check_out(dev(torch.zeros(4)), (4,), "x")
    A.check_slot(dev(torch.zeros(1)), 1, "x")
    A.image_hw(np.zeros((2, 3), np.float32), "x", f32=True)
    A.camera_params({"tan_fovx": 1.0, "tan_fovy": 1.0, "width": 2, "height": 2}, "x")
    assert not hasattr(A, "_lib") and not hasattr(A, "_host")
