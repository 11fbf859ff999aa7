"""CPU-side checks of the TSDF stage's C ABI and Python surface (include/gsr_tsdf.h): the header is plain C99, the library exports
what it declares and _lib binds it in a table of its own, the workspace follows its stated formula, every argument is refused in the
documented order before anything is enqueued, the Python validators raise before the library is touched, save_mesh_ply round-trips
through a parser of the test's own, and the trainer parses --mesh-out."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from abi_helpers import A, compile_c99_probe, declared_names, libpath  # noqa: F401  (libpath: a fixture)
from conftest import ROOT, sub

import tsdf_reference as R

HDR = os.path.join(ROOT, "include", "gsr_tsdf.h")
NAMES = {"gsr_mesh_workspace_bytes", "gsr_tsdf_reset", "gsr_tsdf_integrate", "gsr_tsdf_depth", "gsr_mesh_count", "gsr_mesh_emit"}


def test_tsdf_header_is_plain_c99(tmp_path):
    compile_c99_probe(tmp_path, '#include "gsr_tsdf.h"\n'
                                'typedef char view[sizeof(GsrTsdfView) == 104 ? 1 : -1];\n'
                                'typedef char fits[sizeof(GsrTsdfView) * GSR_TSDF_VIEWS_PER_LAUNCH + 128 <= 4096 ? 1 : -1];\n'
                                'typedef char scan[GSR_MESH_SCAN_GROUPS == 4 * GSR_MESH_GROUP_CELLS ? 1 : -1];\n'
                                'typedef char vox[GSR_TSDF_MAX_VOXELS == 2147483648 && GSR_TSDF_MAX_DIM == 2048 && GSR_MESH_DIRECTIONS == 7 ? 1 : -1];\n'
                                'int main(void) {\n'
                                '  size_t (*w)(int32_t, int32_t, int32_t) = gsr_mesh_workspace_bytes;\n'
                                '  int (*r)(const GsrTsdfVolume *, void *) = gsr_tsdf_reset;\n'
                                '  int (*i)(const GsrTsdfVolume *, int32_t, const GsrTsdfView *, float, float, float, void *) = gsr_tsdf_integrate;\n'
                                '  int (*d)(const float *, const float *, int32_t, int32_t, float, float *, void *) = gsr_tsdf_depth;\n'
                                '  int (*c)(const GsrTsdfVolume *, float, void *, size_t, int64_t *, void *) = gsr_mesh_count;\n'
                                '  int (*e)(const GsrTsdfVolume *, float, const void *, size_t, int64_t, float *, float *, int64_t *, void *) = gsr_mesh_emit;\n'
                                '  (void)w; (void)r; (void)i; (void)d; (void)c; (void)e; return 0; }\n')


def test_tsdf_entry_points_are_exported_bound_and_documented(libpath):
    declared = declared_names(HDR)
    assert declared == NAMES
    _lib = sub("_lib")
    assert set(_lib.TSDF_EXPORTS) == declared
    tables = [getattr(_lib, k) for k in dir(_lib) if k.endswith("EXPORTS") and k != "TSDF_EXPORTS"]
    assert len(tables) >= 15                                                             # EXPORTS and every feature's own table
    for other in tables:
        assert not (declared & set(other))
    lib = C.CDLL(libpath)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gsr_h = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "gsr_tsdf.h" in doc
    for name in declared:
        assert hasattr(lib, name), name
        assert name in doc, name
        assert name not in gsr_h
    assert "tsdf" not in gsr_h.lower() and "gsr_mesh" not in gsr_h
    assert _lib.lib().gsr_abi_version() == 7
    exported = subprocess.run(["nm", "-D", "--defined-only", libpath], capture_output=True, text=True).stdout
    assert {ln.split()[-1] for ln in exported.splitlines() if "gsr_tsdf" in ln or "gsr_mesh" in ln} == declared     # exactly the declared names
    hdr = open(HDR).read()
    for macro, value in (("GSR_TSDF_MAX_DIM", _lib.TSDF_MAX_DIM), ("GSR_TSDF_MAX_VOXELS", _lib.TSDF_MAX_VOXELS),
                         ("GSR_TSDF_VIEWS_PER_LAUNCH", _lib.TSDF_VIEWS_PER_LAUNCH), ("GSR_TSDF_MAX_SIDE", _lib.TSDF_MAX_SIDE), ("GSR_MESH_GROUP_CELLS", _lib.MESH_GROUP_CELLS),
                         ("GSR_MESH_SCAN_GROUPS", _lib.MESH_SCAN_GROUPS), ("GSR_MESH_DIRECTIONS", _lib.MESH_DIRECTIONS)):
        assert f"#define {macro} {value} " in hdr, macro
    assert (R.VIEWS_PER_LAUNCH, R.GROUP_CELLS, R.SCAN_GROUPS, R.DIRECTIONS) == (_lib.TSDF_VIEWS_PER_LAUNCH, _lib.MESH_GROUP_CELLS, _lib.MESH_SCAN_GROUPS,
                                                                               _lib.MESH_DIRECTIONS)    # the yardstick's constants are the header's
    assert C.sizeof(_lib.GsrTsdfView) == 104 and C.sizeof(_lib.GsrTsdfVolume) == 56
    assert _lib.TSDF_VIEWS_PER_LAUNCH == 16


def test_mesh_workspace_bytes_follow_the_stated_formula(libpath):
    _lib = sub("_lib")
    L = _lib.lib()
    gc, sg = _lib.MESH_GROUP_CELLS, _lib.MESH_SCAN_GROUPS
    for G in ((1, 1, 1), (2, 2, 2), (9, 5, 3), (17, 16, 15), (65, 65, 65), (256, 256, 256), (512, 512, 512), (2048, 1024, 1024), (2048, 2048, 512), (1, 2048, 2048)):
        groups = max(1, -(-((G[0] - 1) * (G[1] - 1) * (G[2] - 1)) // gc))
        want = -(-4 * groups // 256) * 256 + -(-8 * -(-groups // sg) // 256) * 256
        assert int(L.gsr_mesh_workspace_bytes(*G)) == want == R.workspace_bytes(*G), G
    for G in ((0, 5, 5), (5, 0, 5), (5, 5, -1), (2049, 1, 1), (2048, 2048, 513), (2048, 2048, 2048)):
        assert int(L.gsr_mesh_workspace_bytes(*G)) == 0 == R.workspace_bytes(*G), G


def test_tsdf_arguments_are_checked_in_order_before_any_hip_call(libpath):
    """Fake aligned pointers: every case returns before anything is dereferenced or enqueued.  GSR_E_NULL, GSR_E_DIMS, GSR_E_ALIGN,
    GSR_E_WORKSPACE, in that order."""
    _lib = sub("_lib")
    L = _lib.lib()
    E = _lib
    inf, nan = float("inf"), float("nan")
    G = (9, 5, 3)
    wsb = int(L.gsr_mesh_workspace_bytes(*G))

    def volume(g=G, s=0.1, o=(0.0, 0.0, 0.0), t=A, w=A, c=A):
        v = _lib.GsrTsdfVolume()
        v.Gx, v.Gy, v.Gz = g
        v.voxel_size = s
        v.origin[:] = list(o)
        v.tsdf, v.weight, v.color = t, w, c
        return v

    def views(n=2, **bad):
        arr = (_lib.GsrTsdfView * n)()
        for k in range(n):
            arr[k].depth, arr[k].color = A, None
            arr[k].view[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
            arr[k].tan_fovx, arr[k].tan_fovy, arr[k].W, arr[k].H, arr[k].w_obs = 0.5, 0.4, 37, 29, 1.0
        for name, value in bad.items():           # the LAST view carries the fault: every record is checked
            if name == "m":
                arr[n - 1].view[5] = value
            else:
                setattr(arr[n - 1], name, value)
        return arr

    def reset(v=None, null=False):
        return L.gsr_tsdf_reset(None if null else C.byref(v or volume()), None)

    def integ(v=None, null=False, n=2, vw="default", trunc=0.4, dmax=inf, wmax=inf):
        arr = views(n if n > 0 else 1) if vw == "default" else vw
        return L.gsr_tsdf_integrate(None if null else C.byref(v or volume()), n, arr, trunc, dmax, wmax, None)

    def count(v=None, null=False, mw=1.0, ws=A, b=wsb, tot=A):
        return L.gsr_mesh_count(None if null else C.byref(v or volume()), mw, ws, b, tot, None)

    def emit(v=None, null=False, mw=1.0, ws=A, b=wsb, cap=10, vt=A, cl=A, ky=A):
        return L.gsr_mesh_emit(None if null else C.byref(v or volume()), mw, ws, b, cap, vt, cl, ky, None)

    def depth(d=A, t=A, w=37, h=29, am=0.5, z=A):
        return L.gsr_tsdf_depth(d, t, w, h, am, z, None)

    bad_volumes = [volume(g=(0, 5, 3)), volume(g=(9, -1, 3)), volume(g=(2049, 1, 1)), volume(g=(2048, 2048, 513)), volume(s=0.0), volume(s=-1.0),
                   volume(s=nan), volume(s=inf), volume(o=(nan, 0, 0)), volume(o=(0, 0, inf))]
    for call in (reset, integ, count, emit):
        assert call(null=True) == E.GSR_E_NULL, call.__name__
        for v in (volume(t=None), volume(w=None), volume(t=None, g=(0, 0, 0))):          # NULL before the dimensions
            assert call(v=v) == E.GSR_E_NULL, call.__name__
        for v in bad_volumes:
            assert call(v=v) == E.GSR_E_DIMS, call.__name__
        for v in (volume(t=A + 4), volume(w=A + 8), volume(c=A + 4)):
            assert call(v=v) == E.GSR_E_ALIGN, call.__name__
        assert call(v=volume(c=None, g=(0, 1, 1))) == E.GSR_E_DIMS                       # colour is optional: NULL is no error
        assert call(v=volume(t=A + 4, s=0.0)) == E.GSR_E_DIMS                            # the dimensions before alignment
    # integrate
    assert integ(vw=None) == E.GSR_E_NULL
    assert integ(vw=views(depth=None)) == integ(vw=views(depth=None), trunc=0.0) == integ(vw=views(depth=None), v=volume(s=0.0)) == E.GSR_E_NULL
    for n in (0, -3):
        assert integ(n=n) == E.GSR_E_DIMS
    for kw in (dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=inf), dict(trunc=nan), dict(dmax=0.0), dict(dmax=nan), dict(dmax=-inf), dict(wmax=0.0),
               dict(wmax=nan)):
        assert integ(**kw) == integ(**kw, v=volume(t=A + 4)) == E.GSR_E_DIMS, kw
    for bad in (dict(W=0), dict(H=-2), dict(W=1 << 14, H=(1 << 14) + 1), dict(W=(1 << 24) + 1, H=1), dict(W=1, H=(1 << 24) + 2), dict(tan_fovx=0.0), dict(tan_fovy=nan), dict(tan_fovx=inf), dict(w_obs=0.0),
                dict(w_obs=-1.0), dict(w_obs=nan), dict(w_obs=inf), dict(m=nan), dict(m=inf)):
        assert integ(vw=views(**bad)) == integ(vw=views(**bad, color=A + 4)) == E.GSR_E_DIMS, bad
    assert integ(vw=views(depth=A + 4)) == integ(vw=views(color=A + 8)) == integ(n=17, vw=views(17, depth=A + 4)) == E.GSR_E_ALIGN
    # count and emit
    for call in (count, emit):
        assert call(ws=None) == call(ws=None, mw=0.0) == E.GSR_E_NULL
        for mw in (0.0, -1.0, nan):
            assert call(mw=mw) == call(mw=mw, ws=A + 4, b=0) == E.GSR_E_DIMS
        assert call(ws=A + 4) == call(ws=A + 8, b=0) == E.GSR_E_ALIGN                    # alignment before the workspace
        assert call(b=wsb - 1) == call(b=0) == E.GSR_E_WORKSPACE
    assert count(tot=None) == E.GSR_E_NULL and count(tot=A + 4) == count(tot=A + 4, b=0) == E.GSR_E_ALIGN
    assert emit(vt=None) == emit(ky=None) == emit(ky=None, cap=-1) == E.GSR_E_NULL
    assert emit(cap=-1) == emit(cap=-1, vt=A + 4) == E.GSR_E_DIMS
    assert emit(vt=A + 4) == emit(cl=A + 4) == emit(ky=A + 8) == E.GSR_E_ALIGN
    assert emit(cl=None, b=wsb - 1) == E.GSR_E_WORKSPACE                                 # colours are optional
    # depth
    for k in ("d", "t", "z"):
        assert depth(**{k: None}) == depth(**{k: None}, w=0) == E.GSR_E_NULL
        assert depth(**{k: A + 4}) == E.GSR_E_ALIGN
    for kw in (dict(w=0), dict(h=-1), dict(w=1 << 14, h=(1 << 14) + 1), dict(am=nan), dict(am=inf)):
        assert depth(**kw) == depth(**kw, d=A + 4) == E.GSR_E_DIMS


def test_python_validators_raise_before_the_library_is_touched(monkeypatch):
    _lib, tsdf, forward, backward = sub("_lib"), sub("tsdf"), sub("forward"), sub("backward")
    for fn in (forward.render_gaussians, backward.backward):
        assert not [p for p in inspect.signature(fn).parameters if "tsdf" in p or "mesh" in p]     # a stage of its own: no new keyword
    assert list(inspect.signature(tsdf.TSDFVolume.__init__).parameters) == ["self", "origin", "voxel_size", "dims", "trunc", "w_max", "color", "device"]
    assert list(inspect.signature(tsdf.TSDFVolume.integrate).parameters) == ["self", "depth", "camera", "color", "depth_max", "weight"]
    assert list(inspect.signature(tsdf.TSDFVolume.integrate_views).parameters) == ["self", "depths", "cameras", "colors", "depth_max", "weights"]
    assert list(inspect.signature(tsdf.TSDFVolume.extract_mesh).parameters) == ["self", "min_weight"]
    assert inspect.signature(tsdf.TSDFVolume.extract_mesh).parameters["min_weight"].default == 1.0
    assert list(inspect.signature(tsdf.depth_from_buffers).parameters) == ["depth_image", "final_Ts", "alpha_min"]
    assert inspect.signature(tsdf.depth_from_buffers).parameters["alpha_min"].default == _lib.NORMALS_ALPHA_MIN
    assert list(inspect.signature(tsdf.weld).parameters) == ["vertices", "keys", "colors"]

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    inf, nan = float("inf"), float("nan")
    make = lambda **k: tsdf.TSDFVolume(**{"origin": (0, 0, 0), "voxel_size": 0.1, "dims": (4, 4, 4), **k})   # noqa: E731
    for bad in ((0, 0), (0, 0, nan), "abc", None):
        with pytest.raises(ValueError, match="origin must be 3 finite numbers"):
            make(origin=bad)
    for bad in (0.0, -1.0, nan, inf, "x"):
        with pytest.raises(ValueError, match="voxel_size must be"):
            make(voxel_size=bad)
    for bad in ((4, 4), (0, 4, 4), (4, 4, 2049), (2.5, 4, 4), (2048, 2048, 513), 7, None):
        with pytest.raises(ValueError, match="dims must be 3 integers"):
            make(dims=bad)
    for bad in (0.0, -0.1, nan, inf):
        with pytest.raises(ValueError, match="trunc must be positive"):
            make(trunc=bad)
    for bad in (0.0, nan, -inf):
        with pytest.raises(ValueError, match="w_max must be positive"):
            make(w_max=bad)
    with pytest.raises(AssertionError, match="library was touched"):
        make(w_max=inf, trunc=0.3)                                                       # valid arguments pass the checks
    # a volume object without the device: the methods' validators
    vol = object.__new__(tsdf.TSDFVolume)
    vol.origin, vol.voxel_size, vol.dims, vol.trunc, vol.w_max = np.zeros(3, np.float32), 0.1, (4, 4, 4), 0.4, inf
    cam = {"tan_fovx": 0.5, "tan_fovy": 0.4, "width": 7, "height": 5, "world_to_camera": np.eye(4, dtype=np.float32)}
    d, c3 = np.ones((5, 7), np.float32), np.ones((5, 7, 3), np.float32)
    for bad in (None, {}, dict(cam, tan_fovx=0.0), dict(cam, width=0), {k: v for k, v in cam.items() if k != "world_to_camera"},
                dict(cam, world_to_camera=np.eye(3)), dict(cam, world_to_camera=np.full((4, 4), nan))):
        with pytest.raises(ValueError, match="camera|tan_fov|width"):
            vol.integrate(d, bad)
    for bad in (np.ones((7, 5), np.float32), c3):
        with pytest.raises(ValueError, match="depth must have shape"):
            vol.integrate(bad, cam)
    with pytest.raises(ValueError, match="color must have shape"):
        vol.integrate(d, cam, color=d)
    for bad in (0.0, nan, -1.0):
        with pytest.raises(ValueError, match="depth_max must be positive"):
            vol.integrate(d, cam, depth_max=bad)
    for bad in (0.0, nan, inf, -2.0):
        with pytest.raises(ValueError, match="weight must be positive"):
            vol.integrate(d, cam, weight=bad)
    with pytest.raises(ValueError, match="at least one view"):
        vol.integrate_views([], [])
    with pytest.raises(ValueError, match="as many cameras"):
        vol.integrate_views([d, d], [cam])
    with pytest.raises(ValueError, match="colors must be None or hold one image"):
        vol.integrate_views([d, d], [cam, cam], colors=[c3])
    with pytest.raises(ValueError, match="weights must be one number or one per view"):
        vol.integrate_views([d, d], [cam, cam], weights=[1.0])
    for bad in (0.0, nan, -1.0):
        with pytest.raises(ValueError, match="min_weight must be positive"):
            vol.extract_mesh(min_weight=bad)
    for call in (lambda: vol.integrate(d, cam, color=c3, depth_max=inf, weight=2.0), lambda: vol.integrate_views([d, d], [cam, cam], [c3, None], weights=[1, 2]),
                 lambda: vol.extract_mesh(), lambda: vol.reset(), lambda: tsdf.depth_from_buffers(d, d.reshape(5, 7, 1))):
        with pytest.raises(AssertionError, match="library was touched"):
            call()
    with pytest.raises(ValueError, match="alpha_min must be finite"):
        tsdf.depth_from_buffers(d, d, alpha_min=nan)
    for bad in (np.ones(35, np.float32), c3):
        with pytest.raises(ValueError, match="depth_image must have shape"):
            tsdf.depth_from_buffers(bad, d)
    with pytest.raises(ValueError, match="final_Ts must have shape"):
        tsdf.depth_from_buffers(d, d.T)
    # weld: host only
    verts, faces, cols = tsdf.weld(np.arange(18, dtype=np.float32).reshape(2, 3, 3), np.array([[5, 3, 9], [3, 5, 7]]))
    rv, rf, _ = R.weld(np.arange(18, dtype=np.float32).reshape(2, 3, 3), np.array([[5, 3, 9], [3, 5, 7]]))
    assert cols is None and np.array_equal(verts, rv) and np.array_equal(faces, rf) and faces.dtype == np.int32
    with pytest.raises(ValueError, match="weld: vertices must have shape"):
        tsdf.weld(np.zeros((2, 3)), np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match="weld: colors must have shape"):
        tsdf.weld(np.zeros((2, 3, 3)), np.zeros((2, 3), np.int64), np.zeros((2, 3)))


def _parse_mesh_ply(path):
    """A reader of the test's own: (verts, rgb or None, faces)."""
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n" and f.readline() == b"format binary_little_endian 1.0\n"
        elements, line = [], f.readline()
        while line != b"end_header\n":
            tok = line.decode("ascii").split()
            if tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                elements[-1][2].append(tok[1:])
            line = f.readline()
        assert [e[0] for e in elements] == ["vertex", "face"]
        (_, nv, vp), (_, nf, fp) = elements
        assert fp == [["list", "uchar", "int", "vertex_indices"]]
        vdt = np.dtype([(p[1], {"float": "<f4", "uchar": "u1"}[p[0]]) for p in vp])
        v = np.frombuffer(f.read(vdt.itemsize * nv), dtype=vdt)
        raw = np.frombuffer(f.read(13 * nf), dtype=np.uint8).reshape(nf, 13)
        assert f.read() == b"" and (raw[:, 0] == 3).all()
        faces = raw[:, 1:].copy().view("<i4").reshape(nf, 3)
    rgb = np.stack([v["red"], v["green"], v["blue"]], axis=1) if "red" in vdt.names else None
    return np.stack([v["x"], v["y"], v["z"]], axis=1), rgb, faces


def test_save_mesh_ply_round_trips(tmp_path):
    pc = sub("point_cloud")
    vol = R.fill_sdf(R.new_volume((-0.5, -0.5, -0.5), 0.1, (11, 12, 10)), R.sphere_sdf((0.02, 0.03, -0.04), 0.33))
    vol["color"][...] = np.random.default_rng(3).uniform(0, 1, vol["color"].shape).astype(np.float32)
    vertices, colors, keys, _ = R.extract(vol, 1.0)
    verts, faces, cols = sub("tsdf").weld(vertices, keys, colors)
    assert len(faces) > 50
    path = str(tmp_path / "sub" / "mesh.ply")
    pc.save_mesh_ply(path, verts, faces, cols)
    v, rgb, f = _parse_mesh_ply(path)
    assert np.array_equal(v.view(np.uint32), verts.view(np.uint32)) and np.array_equal(f, faces)
    assert np.array_equal(rgb, np.clip(cols * np.float32(255), 0, 255).astype(np.int64))
    pc.save_mesh_ply(path, verts, faces)
    v, rgb, f = _parse_mesh_ply(path)
    assert rgb is None and np.array_equal(v, verts) and np.array_equal(f, faces)
    pc.save_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))    # an empty mesh is a valid file
    v, rgb, f = _parse_mesh_ply(path)
    assert len(v) == 0 and len(f) == 0
    with pytest.raises(ValueError, match="faces must be integer indices"):
        pc.save_mesh_ply(path, verts, faces + len(verts))
    with pytest.raises(ValueError, match="one row per vertex"):
        pc.save_mesh_ply(path, verts, faces, cols[:-1])


def _run(script, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), *extra], capture_output=True, text=True, timeout=300)


def test_trainer_and_extractor_parse_their_mesh_flags():
    p = _run("train.py", "--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--mesh-out", "--mesh-resolution", "--mesh-min-weight"):
        assert flag in p.stdout, flag
    p = _run("train.py", "--mesh-out", "m.ply", "--mesh-resolution", "1")
    assert p.returncode != 0 and "--mesh-resolution must be in 2 .. 2048" in p.stderr
    p = _run("train.py", "--mesh-out", "m.ply", "--lambda-dssim", "2")      # a valid --mesh-out is parsed: the refusal is the other flag's
    assert p.returncode != 0 and "--lambda-dssim must be in [0, 1]" in p.stderr
    p = _run("extract_mesh.py", "--help")
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--model", "--dataset", "--views", "--voxel-size", "--resolution", "--trunc", "--depth-max", "--min-weight", "--out"):
        assert flag in p.stdout, flag
    p = _run("extract_mesh.py", "--model", "a.ply", "--dataset", "d", "--voxel-size", "0.1", "--resolution", "64")
    assert p.returncode != 0 and "not allowed with" in p.stderr
