"""What the CPU-side ABI tests share: the library path (built if missing), the names a header declares, a C99 probe compile and
the fake-pointer call set-up.  A plain module: a test file that wants the `libpath` fixture imports it by name."""
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT, PKG_NAME, sub

INCLUDE = os.path.join(ROOT, "include")
A = 0x10000         # any 16-byte aligned non-null value: a fake pointer that a refused call never dereferences


class OnDevice(torch.Tensor):
    """A stand-in that claims to be a device tensor (there is no GPU here): `t.as_subclass(OnDevice)`."""
    is_cuda = True


@pytest.fixture(scope="module")
def libpath():
    path = os.path.join(ROOT, PKG_NAME, "libgsr_hip.so")
    if not os.path.exists(path):   # hipcc cross-compiles gfx950 without a GPU
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, PKG_NAME, "csrc")])
    return path


def declared_names(header_path):
    """The gsr_* functions a header declares (its comments, which name other headers' functions, left out)."""
    code = re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S)
    return set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", code))


def compile_c99_probe(tmp_path, source):
    """Compile `source` as strict C99 against include/; the assertion carries the compiler's complaint."""
    probe = tmp_path / "probe.c"
    probe.write_text(source)
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-c", str(probe), "-o", str(tmp_path / "probe.o")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def fake_call_setup():
    """(_lib, L, A, N, W, H, scene, cam): an 8-Gaussian scene of fake pointers and a 32 x 32 camera."""
    _lib = sub("_lib")
    N, W, H = 8, 32, 32
    scene = _lib.GsrScene(N, A, A, A, A, A, 3, 1.0, 1)
    cam = _lib.GsrCamera()
    cam.W, cam.H, cam.tan_fovx, cam.tan_fovy = W, H, 0.5, 0.5
    return _lib, _lib.lib(), A, N, W, H, scene, cam
