"""CPU-side checks of the kNN stage's C ABI and Python surface (include/gsr_knn.h): the header is plain C99, the library exports what it
declares and _lib binds it in a table of its own, every argument is refused in the documented order before anything is enqueued, the
Python validators raise before the library is touched, load_points reads what it says it reads, and the trainer parses its flags."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_helpers import A, OnDevice, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

HDR = os.path.join(ROOT, "include", "gsr_knn.h")
NAMES = {"gsr_knn_workspace_bytes", "gsr_knn"}


def test_knn_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_knn.h"\n'
                                'typedef char three[GSR_KNN_K == 3 ? 1 : -1];\n'
                                'typedef char block[GSR_KNN_BLOCK_POINTS >= 64 && GSR_KNN_BLOCK_POINTS % 64 == 0 ? 1 : -1];\n'
                                'typedef char most[GSR_KNN_MAX_POINTS == 134217728 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  size_t (*w)(int64_t) = gsr_knn_workspace_bytes;\n'
                                '  int (*f)(int64_t, const float *, float *, int32_t *, void *, size_t, void *) = gsr_knn;\n'
                                '  (void)w; (void)f; return 0; }\n')


def test_knn_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.KNN_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "KNN_EXPORTS"]
    assert len(tables) >= 12                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_knn.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc or f"{name}(" in doc, name
        assert name not in gsr_h
    assert "knn" not in gsr_h.lower()
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_knn" in ln} == declared      # exactly the declared names
    hdr = open(HDR).read()
    assert f"#define GSR_KNN_K {_lib.KNN_K}\n" in hdr
    assert f"#define GSR_KNN_BLOCK_POINTS {_lib.KNN_BLOCK_POINTS} " in hdr
    assert "#define GSR_KNN_MAX_POINTS (1 << 27)\n" in hdr and _lib.KNN_MAX_POINTS == 1 << 27
    import knn_reference as R
    assert R.K == _lib.KNN_K                                                              # the yardstick's k is the header's


def _stated_bytes(n):
    """The formula in the header's comment."""
    up = lambda x: -(-x // 256) * 256
    nb, sb = -(-n // 256), -(-n // 1024)
    h = 256 * sb
    return up(32 * 1025) + 2 * up(8 * n) + 2 * up(4 * h) + up(4 * (-(-h // 1024) + 4)) + up(16 * n) + up(32 * nb)


def test_knn_workspace_bytes_follow_the_stated_formula(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    assert _lib.KNN_BLOCK_POINTS == 256                                                  # (the formula above is written for it)
    last = 0
    for n in (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 100_000, 1_000_000, (1 << 27) - 1, 1 << 27):
        b = int(L.gsr_knn_workspace_bytes(n))
        assert b == _stated_bytes(n), n
        assert b % 256 == 0 and b >= last, n
        last = b
    for n in (0, -1, -(1 << 40), (1 << 27) + 1, 1 << 40):
        assert int(L.gsr_knn_workspace_bytes(n)) == 0, n


def test_knn_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN,
    GSR_E_WORKSPACE, in that order."""
    _lib = sub("_lib")
    L = _lib.lib()
    N = 1000
    wsb = int(L.gsr_knn_workspace_bytes(N))
    assert wsb > 0

    def call(n=N, p=A, m=A, i=A, ws=A, b=wsb):
        return L.gsr_knn(n, p, m, i, ws, b, None)

    for k in ("p", "m", "ws"):
        assert call(**{k: None}) == _lib.GSR_E_NULL, k
        assert call(**{k: None}, n=0, b=0) == call(**{k: None}, i=A + 4) == _lib.GSR_E_NULL, k       # NULL before everything else
    for n in (0, -1, (1 << 27) + 1, 1 << 40):
        assert call(n=n) == _lib.GSR_E_DIMS, n
        assert call(n=n, p=A + 4, b=0) == call(n=n, i=None) == _lib.GSR_E_DIMS, n                    # ... before alignment
    for k in ("p", "m", "i", "ws"):
        assert call(**{k: A + 4}) == call(**{k: A + 8}) == _lib.GSR_E_ALIGN, k
        assert call(**{k: A + 4}, b=wsb - 1) == _lib.GSR_E_ALIGN, k                       # alignment before the workspace
    assert call(b=wsb - 1) == call(b=0) == _lib.GSR_E_WORKSPACE
    assert call(i=None, b=wsb - 1) == _lib.GSR_E_WORKSPACE                                # (nn_index may be NULL: not an error)
    assert call(n=1 << 27, b=wsb) == _lib.GSR_E_WORKSPACE                                 # the largest N is a size like any other


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, knn, pc = sub("_lib"), sub("knn"), sub("point_cloud")
    assert list(inspect.signature(knn.knn).parameters) == ["points", "want_indices", "out"]
    assert list(inspect.signature(knn.init_scales).parameters) == ["points", "floor"]
    assert list(inspect.signature(pc.gaussians_from_points).parameters) == ["xyz", "rgb", "opacity", "device"]
    assert inspect.signature(knn.init_scales).parameters["floor"].default == 1e-7
    assert inspect.signature(pc.gaussians_from_points).parameters["opacity"].default == 0.1

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    dev = lambda t: t.as_subclass(OnDevice)
    good = dev(torch.zeros(5, 3))
    for bad, what in ((np.zeros((5, 3), np.float32), "torch tensor"), (torch.zeros(5, 3), "GPU"), (dev(torch.zeros(5, 3, dtype=torch.float64)), "float32"),
                      (dev(torch.zeros(15)), r"shape \(N, 3\)"), (dev(torch.zeros(5, 4)), r"shape \(N, 3\)"), (dev(torch.zeros(0, 3)), "N >= 1"),
                      (dev(torch.zeros(5, 6)[:, ::2]), "contiguous"), (dev(torch.zeros(3, 5).t()), "contiguous")):
        for f in (knn.knn, knn.init_scales):
            with pytest.raises(ValueError, match=what):
                f(bad)
    for bad in (torch.zeros(5), dev(torch.zeros(4)), dev(torch.zeros(5, 1)), dev(torch.zeros(5, dtype=torch.float64)), dev(torch.zeros(10)[::2]),
                np.zeros(5, np.float32), (dev(torch.zeros(5)), dev(torch.zeros(5, 3, dtype=torch.int32)))):
        with pytest.raises(ValueError, match="mean_dist2"):
            knn.knn(good, out=bad)
    ok_mean, ok_idx = dev(torch.zeros(5)), dev(torch.zeros(5, 3, dtype=torch.int32))
    for bad in (ok_mean, (ok_mean,), (ok_mean, ok_idx, ok_idx)):
        with pytest.raises(ValueError, match="pair"):
            knn.knn(good, want_indices=True, out=bad)
    for bad in (dev(torch.zeros(5, 3)), dev(torch.zeros(5, 3, dtype=torch.int64)), dev(torch.zeros(4, 3, dtype=torch.int32)),
                torch.zeros(5, 3, dtype=torch.int32), dev(torch.zeros(15, dtype=torch.int32))):
        with pytest.raises(ValueError, match="indices"):
            knn.knn(good, want_indices=True, out=(ok_mean, bad))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="floor must be positive"):
            knn.init_scales(good, floor=bad)
    # gaussians_from_points cannot run without a GPU: its shape and dtype contract, through its validator
    xyz = np.zeros((5, 3), np.float64)
    for bad in (np.zeros(15), np.zeros((5, 4)), np.zeros((0, 3)), np.zeros((5, 3, 1))):
        with pytest.raises(ValueError, match=r"xyz must have shape \(N, 3\)"):
            pc.gaussians_from_points(bad)
    with pytest.raises(ValueError, match="xyz must be finite"):
        pc.gaussians_from_points(np.full((5, 3), np.nan))
    for bad in (np.zeros((4, 3)), np.zeros((5, 4)), np.zeros(15)):
        with pytest.raises(ValueError, match="rgb must have shape"):
            pc.gaussians_from_points(xyz, bad)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"opacity must be in \(0, 1\)"):
            pc.gaussians_from_points(xyz, opacity=bad)
    x, c, o = pc.check_points(xyz, torch.full((5, 3), 0.25, dtype=torch.float64), 0.1)
    assert (x.dtype, x.shape, c.dtype, c.shape, o) == (np.float32, (5, 3), np.float32, (5, 3), 0.1)
    # valid arguments pass the checks
    for call in (lambda: knn.knn(good), lambda: knn.knn(good, out=ok_mean), lambda: knn.knn(good, want_indices=True, out=(ok_mean, ok_idx)),
                 lambda: knn.init_scales(good, floor=1e-3)):
        with pytest.raises(AssertionError, match="library was touched"):
            call()


def _write_ply(path, props, rows, fmt="binary_little_endian", tail=b""):
    """props: (ply type, name, numpy type) per vertex property; rows: one array per property."""
    head = ["ply", f"format {fmt} 1.0", "comment written by the test", f"element vertex {len(rows[0])}"]
    head += [f"property {t} {name}" for t, name, _ in props] + ["element face 0", "property list uchar int vertex_indices", "end_header"]
    v = np.zeros(len(rows[0]), np.dtype([(name, nt) for _, name, nt in props]))
    for (_, name, _), r in zip(props, rows):
        v[name] = r
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(v.tobytes() + tail)
    return len(("\n".join(head) + "\n").encode("ascii")), v.nbytes


XYZ = [("float", "x", "<f4"), ("float", "y", "<f4"), ("float", "z", "<f4")]
RGB = [("uchar", "red", "u1"), ("uchar", "green", "u1"), ("uchar", "blue", "u1")]


def test_load_points_reads_xyz_colours_and_skips_the_rest(tmp_path):
    pc = sub("point_cloud")
    rng = np.random.default_rng(3)
    n = 37
    xyz = rng.normal(0, 2, (n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    p = str(tmp_path / "a.ply")
    _write_ply(p, XYZ, list(xyz.T))
    got, col = pc.load_points(p)
    assert got.dtype == np.float32 and got.tobytes() == xyz.tobytes() and col is None
    _write_ply(p, XYZ + RGB, list(xyz.T) + list(rgb.T))
    got, col = pc.load_points(p)
    assert got.tobytes() == xyz.tobytes()
    assert col.dtype == np.float32 and col.shape == (n, 3) and (col == rgb.astype(np.float32) / np.float32(255)).all()
    assert col.min() >= 0.0 and col.max() <= 1.0
    # properties to skip by their declared size, in front of, between and behind the ones that count: COLMAP's normals, a double, a short
    props = [("double", "t", "<f8")] + XYZ[:2] + [("float", "nx", "<f4"), ("short", "label", "<i2")] + XYZ[2:] + RGB + [("float32", "confidence", "<f4")]
    rows = [rng.normal(size=n), xyz[:, 0], xyz[:, 1], rng.normal(size=n), rng.integers(-5, 5, n), xyz[:, 2], *rgb.T, rng.normal(size=n)]
    header, body = _write_ply(p, props, rows)
    got, col = pc.load_points(p)
    assert got.tobytes() == xyz.tobytes() and (col == rgb.astype(np.float32) / np.float32(255)).all()
    # float colours are not uchar colours: no colours
    _write_ply(p, XYZ + [("float", k, "<f4") for _, k, _ in RGB], list(xyz.T) + list(rgb.T))
    assert pc.load_points(p)[1] is None
    # refused: a truncated file, an ASCII file, no z, a list property among the vertices, no PLY at all
    _write_ply(p, props, rows)
    with open(p, "r+b") as f:
        f.truncate(header + body - 1)
    with pytest.raises(ValueError, match="truncated"):
        pc.load_points(p)
    _write_ply(p, XYZ, list(xyz.T), fmt="ascii")
    with pytest.raises(ValueError, match="binary_little_endian"):
        pc.load_points(p)
    _write_ply(p, XYZ[:2], list(xyz.T[:2]))
    with pytest.raises(ValueError, match="x, y, z"):
        pc.load_points(p)
    with open(p, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty list uchar int k\nend_header\n")
    with pytest.raises(ValueError, match="scalar"):
        pc.load_points(p)
    with open(p, "wb") as f:
        f.write(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        pc.load_points(p)
    # load_ply and save_ply stay as they are: a checkpoint still round-trips, and load_points reads its positions and colours
    params = {"positions": xyz, "scales": np.ones((n, 3), np.float32), "rotations": np.zeros((n, 4), np.float32), "opacities": np.ones(n, np.float32),
              "shs": np.zeros((n * 16, 3), np.float32)}
    pc.save_ply(params, p, n)
    assert pc.load_ply(p)["positions"].tobytes() == xyz.tobytes()
    got, col = pc.load_points(p)
    assert got.tobytes() == xyz.tobytes() and (col == np.float32(127) / np.float32(255)).all()   # clip(0 + 0.5) * 255, truncated


def _train(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train.py"), *extra], capture_output=True, text=True, timeout=300)


def test_trainer_parses_the_init_flags_and_refuses_the_conflict(tmp_path):
    p = _train("--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--init-points", "{reference,random,knn}", "three nearest neighbours"):
        assert flag in " ".join(p.stdout.split()), flag
    ply = str(tmp_path / "cloud.ply")
    _write_ply(ply, XYZ, list(np.zeros((3, 4), np.float32)))
    for init in ("reference", "random"):
        p = _train("--init", init, "--init-points", ply)
        assert p.returncode != 0 and f"--init-points starts from the file's points: it cannot be combined with --init {init}" in p.stderr
    p = _train("--init", "nearest")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    p = _train("--init-points", str(tmp_path / "missing.ply"))
    assert p.returncode != 0 and "--init-points:" in p.stderr
    _write_ply(ply, XYZ, list(np.zeros((3, 4), np.float32)), fmt="ascii")
    p = _train("--init-points", ply)
    assert p.returncode != 0 and "--init-points: expected a binary_little_endian PLY" in p.stderr
    # valid values are parsed before the other arguments are judged: the refusal below is theirs
    _write_ply(ply, XYZ, list(np.zeros((3, 4), np.float32)))
    for ok in (("--init", "knn"), ("--init-points", ply), ("--init", "knn", "--init-points", ply)):
        p = _train(*ok, "--lambda-dssim", "2")
        assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr, ok
