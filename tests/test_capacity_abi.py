"""CPU-side checks of the capacity-mode forward (include/gsr_capacity.h): the header is plain C, the library exports its entry
point, every argument is checked before anything is enqueued, the Python surface refuses a bad capacity before it touches the
GPU, and the trainer takes --capacity / --capacity-initial."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from abi_helpers import compile_c99_probe, declared_names, fake_call_setup, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_capacity.h")


def test_capacity_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_capacity.h"\n'
                                'int main(void) { int (*f)(const GsrScene *, const GsrCamera *, const GsrGeom *, const GsrBinning *, const GsrImage *,\n'
                                '                          void *, size_t, void *, size_t, int64_t, void *) = gsr_forward_capacity; (void)f; return 0; }\n')


def test_capacity_entry_point_is_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == {"gsr_forward_capacity"}
    lib = C.CDLL(libpath)
    assert hasattr(lib, "gsr_forward_capacity")
    _lib = sub("_lib")
    assert set(_lib.CAPACITY_EXPORTS) == declared and not (declared & set(_lib.EXPORTS))   # its own table (gsr.h's stays as it is)
    assert "gsr_forward_capacity" not in open(os.path.join(ROOT, "include", "gsr.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "gsr_forward_capacity" in doc and "gsr_capacity.h" in doc
    assert hasattr(_lib.lib(), "gsr_forward_capacity")


def test_capacity_arguments_are_checked_before_any_hip_call(libpath):
    """Fake 16-byte-aligned pointers: every case below returns before anything is dereferenced or enqueued."""
    _lib, L, A, N, W, H, scene, cam = fake_call_setup()
    geom = _lib.GsrGeom(A, A, A, A, A, A, A, A, A, None, None)
    img = _lib.GsrImage(A, A, A, A)
    gbytes = int(L.gsr_geom_workspace_bytes(N))

    def call(K, point_list=A, bws_bytes=None, gws_bytes=gbytes, hint=0, **over):
        b = _lib.GsrBinning(K, point_list, A, A, A, None, 0)
        for k, v in over.items():
            setattr(b, k, v)
        need = int(L.gsr_binning_workspace_bytes(N, max(K, 0), W, H)) if bws_bytes is None else bws_bytes
        return L.gsr_forward_capacity(C.byref(scene), C.byref(cam), C.byref(geom), C.byref(b), C.byref(img), A, gws_bytes, A, need,
                                      hint, None)

    assert call(-1) == _lib.GSR_E_OVERFLOW
    assert call((1 << 30) + 1) == _lib.GSR_E_OVERFLOW
    assert call(100, hint=-5) == _lib.GSR_E_OVERFLOW
    assert call(100, point_list=None) == _lib.GSR_E_NULL
    assert call(100, point_list=A + 4) == _lib.GSR_E_ALIGN
    assert call(100, block_masks=A + 8) == _lib.GSR_E_ALIGN
    assert call(100, backward_ws=A + 4) == _lib.GSR_E_ALIGN
    need = int(L.gsr_binning_workspace_bytes(N, 100, W, H))
    assert call(100, bws_bytes=need - 1) == _lib.GSR_E_WORKSPACE
    assert call(100, gws_bytes=gbytes - 1) == _lib.GSR_E_WORKSPACE
    # the binning workspace is sized by K: one sized for fewer pairs is refused
    assert call(100, bws_bytes=int(L.gsr_binning_workspace_bytes(N, 10, W, H))) == _lib.GSR_E_WORKSPACE
    scene.rotations = A + 4
    assert call(100) == _lib.GSR_E_ALIGN


def test_render_gaussians_refuses_a_bad_capacity_before_the_gpu(monkeypatch):
    gsr = sub("forward")
    host = sub("_host")

    def no_gpu(*a, **k):
        raise AssertionError("reached the GPU")
    monkeypatch.setattr(host, "device_of", no_gpu)
    monkeypatch.setattr(gsr._host, "device_of", no_gpu)
    for bad, exc in ((-1, ValueError), ((1 << 30) + 1, ValueError), ("x", TypeError), (2.5, TypeError), (True, TypeError)):
        with pytest.raises(exc):
            gsr.render_gaussians(background=[0, 0, 0], means3D=[[0, 0, 0]], capacity=bad)
    with pytest.raises(ValueError):
        gsr.render_gaussians(background=[0, 0, 0], means3D=[[0, 0, 0]], capacity=10, capacity_hint=-1)


def test_rendered_count_refuses_a_sized_frame():
    import torch
    fwd = sub("forward")
    with pytest.raises(ValueError, match="capacity-mode"):
        fwd.rendered_count({"point_list": torch.zeros(3, dtype=torch.int32)})


def test_trainer_parses_the_capacity_flags():
    train = os.path.join(ROOT, "examples", "train.py")
    p = subprocess.run([sys.executable, train, "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "--capacity" in p.stdout and "--capacity-initial" in p.stdout, p.stderr[-2000:]
    # a --capacity-initial without --capacity, or out of range, is refused while parsing (before any GPU work)
    for extra in (["--capacity-initial", "1000"], ["--capacity", "--capacity-initial", "-1"]):
        p = subprocess.run([sys.executable, train, *extra], capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and "--capacity-initial needs --capacity" in p.stderr, (extra, p.stderr[-2000:])
