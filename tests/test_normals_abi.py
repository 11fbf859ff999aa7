"""CPU-side checks of the normals stage's C ABI and Python surface (include/gsr_normals.h): the header is plain C99, the library
exports what it declares and _lib binds it in a table of its own, every argument is refused in the documented order before anything
is enqueued, the Python validators raise before the library is touched, and the trainer parses its flags and refuses --lambda-normal
with a dataset that has no normal targets."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import A, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_normals.h")
NAMES = {"gsr_normals_workspace_bytes", "gsr_normals_from_depth", "gsr_normals_from_depth_backward", "gsr_normals_loss_grad"}


def test_normals_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_normals.h"\n'
                                'typedef char record[GSR_NORMALS_RECORD_BYTES == 8 * GSR_NORMALS_SUMS_FLOATS && GSR_NORMALS_RECORD_BYTES % 16 == 0 ? 1 : -1];\n'
                                'typedef char tile[GSR_NORMALS_TILE_W * GSR_NORMALS_TILE_H == 256 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  size_t (*w)(int32_t, int32_t) = gsr_normals_workspace_bytes;\n'
                                '  int (*f)(const float *, const float *, float, float, int32_t, int32_t, float, float *, float *, void *) = gsr_normals_from_depth;\n'
                                '  int (*b)(const float *, const float *, float, float, int32_t, int32_t, float, const float *, float *, float *, void *, size_t,\n'
                                '           void *) = gsr_normals_from_depth_backward;\n'
                                '  int (*l)(const float *, const float *, const float *, const float *, const float *, float, float, int32_t, int32_t, float,\n'
                                '           float, float *, float *, float *, void *, size_t, void *) = gsr_normals_loss_grad;\n'
                                '  float v = GSR_NORMALS_MIN_NORM2 + GSR_NORMALS_ALPHA_MIN;\n'
                                '  int n = GSR_NORMALS_MAX_BLOCKS;\n'
                                '  (void)w; (void)f; (void)b; (void)l; (void)v; (void)n; return 0; }\n')


def test_normals_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.NORMALS_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "NORMALS_EXPORTS"]
    assert len(tables) >= 14                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_normals.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "normals" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_normals" in ln} == declared      # exactly the declared names
    hdr = open(HDR).read()
    for macro, value in (("GSR_NORMALS_TILE_W", _lib.NORMALS_TILE_W), ("GSR_NORMALS_TILE_H", _lib.NORMALS_TILE_H),
                         ("GSR_NORMALS_MAX_BLOCKS", _lib.NORMALS_MAX_BLOCKS), ("GSR_NORMALS_RECORD_BYTES", _lib.NORMALS_RECORD_BYTES),
                         ("GSR_NORMALS_SUMS_FLOATS", _lib.NORMALS_SUMS_FLOATS), ("GSR_NORMALS_MIN_NORM2", f"{_lib.NORMALS_MIN_NORM2}f"),
                         ("GSR_NORMALS_ALPHA_MIN", f"{_lib.NORMALS_ALPHA_MIN}f")):
        assert f"#define {macro} {value} " in hdr, macro
    import normals_reference as R
    import test_normals_reference as T
    assert float(R.MIN_NORM2) == float(np.float32(_lib.NORMALS_MIN_NORM2)) and R.ALPHA_MIN == _lib.NORMALS_ALPHA_MIN   # the yardstick's constants are the header's
    assert (T.TILE_W, T.TILE_H, T.MAX_BLOCKS) == (_lib.NORMALS_TILE_W, _lib.NORMALS_TILE_H, _lib.NORMALS_MAX_BLOCKS)


def test_normals_workspace_bytes_follow_the_stated_grid(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    tw, th, mb, rb = _lib.NORMALS_TILE_W, _lib.NORMALS_TILE_H, _lib.NORMALS_MAX_BLOCKS, _lib.NORMALS_RECORD_BYTES
    for W, H in ((1, 1), (37, 29), (800, 800), (1920, 1080), (1 << 14, 1 << 14), (1 << 28, 1), (1, 1 << 28)):
        records = min(-(-W // tw) * -(-H // th), mb)
        assert int(L.gsr_normals_workspace_bytes(W, H)) == -(-rb * records // 256) * 256, (W, H)
    for W, H in ((0, 5), (5, 0), (-1, 5), (1 << 14, (1 << 14) + 1)):
        assert int(L.gsr_normals_workspace_bytes(W, H)) == 0, (W, H)


def test_normals_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN,
    GSR_E_WORKSPACE, in that order."""
    _lib = sub("_lib")
    L = _lib.lib()
    W, H = 37, 29
    wsb = int(L.gsr_normals_workspace_bytes(W, H))
    assert wsb > 0 and wsb % 16 == 0
    inf, nan = float("inf"), float("nan")
    rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    cam_dims = (dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 14, h=(1 << 14) + 1), dict(tx=0.0), dict(ty=-0.5), dict(tx=inf), dict(ty=nan),
                dict(am=nan), dict(am=inf))

    def fwd(d=A, t=A, tx=0.5, ty=0.4, w=W, h=H, am=0.5, n=A, v=A):
        return L.gsr_normals_from_depth(d, t, tx, ty, w, h, am, n, v, None)

    def bwd(d=A, t=A, tx=0.5, ty=0.4, w=W, h=H, am=0.5, g=A, gd=A, ga=A, ws=A, b=wsb):
        return L.gsr_normals_from_depth_backward(d, t, tx, ty, w, h, am, g, gd, ga, ws, b, None)

    def loss(d=A, t=A, tg=A, r=rot, m=A, tx=0.5, ty=0.4, w=W, h=H, am=0.5, wt=0.5, gd=A, ga=A, s=A + 4, ws=A, b=wsb):
        return L.gsr_normals_loss_grad(d, t, tg, r, m, tx, ty, w, h, am, wt, gd, ga, s, ws, b, None)

    for call, required, optional, images in ((fwd, ("d", "t", "n"), ("v",), ("d", "t", "n", "v")),
                                             (bwd, ("d", "t", "g", "gd", "ga", "ws"), (), ("d", "t", "g", "gd", "ga", "ws")),
                                             (loss, ("d", "t", "tg", "s", "ws"), ("m", "r"), ("d", "t", "tg", "m", "gd", "ga", "ws"))):
        for k in required:
            assert call(**{k: None}) == _lib.GSR_E_NULL, (call.__name__, k)
            assert call(**{k: None}, w=0) == call(**{k: None}, am=nan) == _lib.GSR_E_NULL, (call.__name__, k)     # NULL before the dimensions
        for bad in cam_dims:
            assert call(**bad) == _lib.GSR_E_DIMS, (call.__name__, bad)
            assert call(**bad, d=A + 4) == _lib.GSR_E_DIMS, (call.__name__, bad)                                  # ... before alignment
        for k in images:
            assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, (call.__name__, k)              # images, the workspace: 16 bytes
        for k in optional:
            assert call(**{k: None}, w=0) == _lib.GSR_E_DIMS, (call.__name__, k)                                  # optional: NULL is no error
    assert loss(gd=None) == loss(ga=None) == loss(gd=None, w=0) == _lib.GSR_E_NULL       # gD and gA: both or neither
    assert loss(gd=None, ga=None, w=0) == _lib.GSR_E_DIMS
    for wt in (inf, -inf, nan):
        assert loss(wt=wt) == loss(wt=wt, d=A + 4, b=0) == _lib.GSR_E_DIMS
    assert loss(s=A + 2) == loss(s=A + 1, b=0) == _lib.GSR_E_ALIGN                       # sums: 4 bytes
    for call in (bwd, loss):
        assert call(d=A + 4, b=wsb - 1) == _lib.GSR_E_ALIGN                              # alignment before the workspace
        assert call(b=wsb - 1) == call(b=0) == _lib.GSR_E_WORKSPACE
    assert loss(m=None, r=None, gd=None, ga=None, b=wsb - 1) == _lib.GSR_E_WORKSPACE     # (mask, R, gD and gA may be NULL: not an error)


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, loss, normals, forward, backward = sub("_lib"), sub("loss"), sub("normals"), sub("forward"), sub("backward")
    for fn in (forward.render_gaussians, backward.backward):
        assert not [p for p in inspect.signature(fn).parameters if "normal" in p]        # an image-space stage: no new keyword
    assert list(inspect.signature(loss.normal_loss_and_gradients).parameters) == ["depth", "final_Ts", "target", "camera", "mask", "weight",
                                                                                  "target_rotation", "alpha_min", "want_grad", "loss_out"]
    assert list(inspect.signature(normals.normals_from_depth).parameters) == ["depth", "final_Ts", "camera", "alpha_min"]
    assert list(inspect.signature(normals.normals_from_depth_backward).parameters) == ["dL_dnormals", "depth", "final_Ts", "camera", "alpha_min"]
    assert inspect.signature(normals.normals_from_depth).parameters["alpha_min"].default == 0.5

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    cam = {"tan_fovx": 0.5, "tan_fovy": 0.4, "width": 7, "height": 5}
    d, t3 = np.ones((5, 7), np.float32), np.ones((5, 7, 3), np.float32)
    r = normals.pixel_rays(cam)                                                          # host arithmetic: no library
    assert r.shape == (5, 7, 3) and r[0, 0, 0] == (1.0 / 7 - 1.0) * 0.5 and r[4, 6, 1] == (9.0 / 5 - 1.0) * 0.4 and (r[..., 2] == 1.0).all()
    calls = {"fwd": lambda **k: normals.normals_from_depth(**{"depth": d, "final_Ts": d, "camera": cam, **k}),
             "bwd": lambda **k: normals.normals_from_depth_backward(**{"dL_dnormals": t3, "depth": d, "final_Ts": d, "camera": cam, **k}),
             "loss": lambda **k: loss.normal_loss_and_gradients(**{"depth": d, "final_Ts": d, "target": t3, "camera": cam, **k})}
    for name, f in calls.items():
        for bad in (None, {}, {"tan_fovx": 0.5}, dict(cam, tan_fovx=0.0), dict(cam, tan_fovy=float("nan")), dict(cam, width=0), dict(cam, height=2.5)):
            with pytest.raises(ValueError, match="camera|tan_fov|width"):
                f(camera=bad)
        for bad in (np.ones((7, 5), np.float32), np.ones(35, np.float32), t3):
            with pytest.raises(ValueError, match="depth must have shape"):
                f(depth=bad)
            with pytest.raises(ValueError, match="final_Ts must have shape"):
                f(final_Ts=bad)
        with pytest.raises(ValueError, match="alpha_min must be finite"):
            f(alpha_min=float("nan"))
        with pytest.raises(AssertionError, match="library was touched"):
            f()                                                                          # valid arguments pass the checks
    with pytest.raises(ValueError, match="dL_dnormals must have shape"):
        calls["bwd"](dL_dnormals=d)
    f = calls["loss"]
    for bad in (d, np.ones((5, 7, 4), np.float32)):
        with pytest.raises(ValueError, match="target must have shape"):
            f(target=bad)
    with pytest.raises(ValueError, match="mask must have shape"):
        f(mask=t3)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight must be finite"):
            f(weight=bad)
    for bad in (np.eye(4), np.ones(9), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="target_rotation must be a finite 3 x 3 matrix"):
            f(target_rotation=bad)
    for bad in (torch.zeros(2), np.zeros(2, np.float32)):
        with pytest.raises(ValueError, match="loss_out must be a contiguous 2-element float32 device tensor"):
            f(loss_out=bad)
    with pytest.raises(AssertionError, match="library was touched"):
        f(mask=d, target_rotation=np.eye(3), weight=0.0, want_grad=False, depth=d.reshape(5, 7, 1))
    with pytest.raises(ValueError, match="must be a float32 device tensor"):
        normals.depth_to_normals(torch.ones(5, 7), torch.ones(5, 7), cam)


def _train(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_the_normal_flags_and_refuses_a_dataset_without_targets():
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--lambda-normal", "--normal-dir", "--normal-space", "{camera,world}", "--normal-alpha-min"):
        assert flag in p.stdout, flag
    p = _train("--lambda-normal", "-0.1")
    assert p.returncode != 0 and "--lambda-normal must be >= 0" in p.stderr
    p = _train("--lambda-normal", "nan")
    assert p.returncode != 0 and "--lambda-normal must be >= 0" in p.stderr
    p = _train("--lambda-normal", "0.1", "--dataset", os.path.join(ROOT, "data", "lego"))
    assert p.returncode != 0 and "--lambda-normal with --dataset needs --normal-dir" in p.stderr
    p = _train("--normal-dir", "somewhere")
    assert p.returncode != 0 and "--normal-dir needs --dataset" in p.stderr
    p = _train("--normal-space", "tangent")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    p = _train("--normal-alpha-min", "inf")
    assert p.returncode != 0 and "--normal-alpha-min must be finite" in p.stderr
    # valid values are parsed before the other arguments are judged: the refusal below is theirs
    p = _train("--lambda-normal", "0.1", "--normal-alpha-min", "0.3", "--normal-space", "world", "--lambda-dssim", "2")
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr
