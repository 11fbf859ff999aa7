"""The TSDF stage on the MI355X (include/gsr_tsdf.h) against its numpy restatement (tests/tsdf_reference.py, which
tests/test_tsdf_reference.py holds to analytic surfaces on the CPU).  Every comparison is bit for bit: tsdf, weight, colour, the
triangle count, vertices, colours and keys, in order.  The shapes are the smallest at which the kernels can go wrong: grids with no
cell, one cell, odd sizes, and one that spans several 256-voxel workgroups along every axis; 1 x 1, 5 x 3 and 37 x 29 images; 1, 16 and 17
views (the launch edge is 16)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import pkg, sub
import tsdf_reference as R

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
#          grid            image (W, H)  views
CASES = (((1, 1, 1),      (1, 1),       1),
         ((2, 2, 2),      (5, 3),       16),
         ((9, 5, 3),      (37, 29),     17),
         ((17, 16, 15),   (5, 3),       17),
         ((67, 35, 19),   (37, 29),     16))     # 174 workgroups of 256 voxels: several along x, y and z


def _dev():
    return torch.device("cuda", 0)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "of", g.size)


def _same_volume(vol, ref, what):
    _same(vol.tsdf, ref["tsdf"], what + " tsdf")
    _same(vol.weight, ref["weight"], what + " weight")
    if ref["color"] is not None:
        _same(vol.color, ref["color"], what + " color")


def _same_mesh(vol, ref, min_weight, what):
    vertices, colors, keys = vol.extract_mesh(min_weight)
    rv, rc, rk, tally = R.extract(ref, min_weight)
    assert len(vertices) == len(rv), (what, len(vertices), len(rv))
    _same(vertices, rv, what + " vertices")
    _same(keys, rk, what + " keys")
    if vol.color is not None:
        _same(colors, rc, what + " colors")
    else:
        assert colors is None
    return rv, rc, rk, tally


def _volume(G, s=None, color=True, trunc=None, w_max=INF, origin=None):
    s = s if s is not None else 1.2 / max(G)
    origin = origin if origin is not None else tuple(-0.5 * s * (g - 1) + 0.01 * (k + 1) for k, g in enumerate(G))
    trunc = trunc if trunc is not None else 3.5 * s
    vol = sub("tsdf").TSDFVolume(origin, s, G, trunc=trunc, w_max=w_max, color=color, device=_dev())
    return vol, R.new_volume(origin, s, G, color=color), trunc


def _random_views(rng, V, W, H, colour_every=1):
    """Cameras on a sphere of radius 2.5 around the volume, depth images that scatter around the distance to it, with holes."""
    cams, depths, colors, weights = [], [], [], []
    for k in range(V):
        d = rng.normal(size=3)
        cam = R.look_at_camera(2.5 * d / np.linalg.norm(d), rng.uniform(-0.1, 0.1, 3), W, H, 0.35)
        z = rng.uniform(2.0, 3.0, (H, W)).astype(np.float32)
        z[rng.uniform(size=(H, W)) < 0.1] = 0.0
        cams.append(cam)
        depths.append(z)
        colors.append(rng.uniform(0, 1, (H, W, 3)).astype(np.float32) if k % colour_every == 0 else None)
        weights.append(float(np.float32(rng.uniform(0.5, 2.0))))
    return cams, depths, colors, weights


def _ref_views(cams, depths, colors, weights):
    return [R.make_view(z, c, col, w) for c, z, col, w in zip(cams, depths, colors, weights)]


@pytest.fixture(scope="module")
def fused():
    """Every case's views and the reference volume after them: computed once, shared, left unchanged."""
    out = {}
    for n, (G, (W, H), V) in enumerate(CASES):
        rng = np.random.default_rng(100 + n)
        s = 1.2 / max(G)
        origin = tuple(-0.5 * s * (g - 1) + 0.01 * (k + 1) for k, g in enumerate(G))
        views = _random_views(rng, V, W, H, colour_every=1 if n % 2 else 3)
        ref = R.integrate(R.new_volume(origin, s, G), _ref_views(*views), 3.5 * s, depth_max=2.9, w_max=6.0)
        out[G] = (views, ref)
    return out


@pytest.mark.parametrize("G,image,V", CASES)
def test_integration_and_extraction_match_the_restatement_bit_for_bit(fused, G, image, V):
    (cams, depths, colors, weights), ref = fused[G]
    vol, _, trunc = _volume(G, w_max=6.0)
    _same_volume(vol, R.new_volume(vol.origin, vol.voxel_size, G), "reset")
    vol.integrate_views(depths, cams, colors, depth_max=2.9, weights=weights)
    _same_volume(vol, ref, f"{G} {V} views")
    if G == CASES[-1][0]:
        assert (ref["weight"] == 6.0).any() and (ref["weight"] == 0).any()               # w_max reached somewhere, nothing seen elsewhere
    # one call per view, and a split that is neither: the same bits
    for cuts in ([(k, k + 1) for k in range(V)], [(0, V // 3), (V // 3, V)]):
        vol.reset()
        for a, b in cuts:
            if b > a:
                vol.integrate_views(depths[a:b], cams[a:b], colors[a:b], depth_max=2.9, weights=weights[a:b])
        _same_volume(vol, ref, f"{G} split {len(cuts)}")
    for mw in (1.0, 2.5):
        rv, _, _, _ = _same_mesh(vol, ref, mw, f"{G} min_weight {mw}")
    if min(G) < 2:
        assert len(rv) == 0                                                              # no cell
    if G == CASES[-1][0]:
        assert len(R.extract(ref, 1.0)[0]) > 1000


def test_every_skip_of_the_integrator():
    """An identity camera with unit tangents over a grid whose voxel coordinates are exact in float32: p = X, so the voxel with Z = 0
    has p_z exactly 0, the voxels with X = -Z have u + 0.5 exactly 0 (pixel 0) and those with X = +Z exactly W (refused)."""
    G, s, origin, trunc, W, H = (7, 7, 6), 0.5, (-1.5, -1.5, -1.0), 0.5, 5, 3
    cam = {"world_to_camera": np.eye(4, dtype=np.float32), "tan_fovx": 1.0, "tan_fovy": 1.0, "width": W, "height": H}
    up = float(np.nextafter(np.float32(2.0), np.float32(3.0)))
    below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    col = np.full((H, W, 3), 0.25, np.float32)

    def run(value, depth_max=INF):
        vol, ref0, _ = _volume(G, s=s, origin=origin, trunc=trunc)
        z = np.full((H, W), value, np.float32)
        vol.integrate(z, cam, color=col, depth_max=depth_max)
        ref = R.integrate(ref0, [R.make_view(z, cam, col)], trunc, depth_max=depth_max)
        _same_volume(vol, ref, f"depth {value}")
        return ref

    for value in (0.0, -1.0, NAN, INF, -INF):             # no measurement
        assert run(value)["weight"].sum() == 0
    ref = run(2.0, depth_max=2.0)                         # d exactly depth_max counts
    assert ref["weight"].sum() > 0
    assert (ref["weight"][:3] == 0).all()                 # Z = -1, -0.5 (behind) and Z = 0 (p_z exactly 0): never touched
    assert ref["weight"][3, 3, 2] == 1 and ref["weight"][3, 3, 4] == 0      # Z = 0.5: X = -Z is pixel 0, X = +Z is past the last
    assert ref["weight"][3, 2, 3] == 1 and ref["weight"][3, 4, 3] == 0      # ... and the same along y
    assert run(up, depth_max=2.0)["weight"].sum() == 0    # just above depth_max
    ref = run(1.0)
    assert ref["weight"][5, 3, 3] == 1 and ref["tsdf"][5, 3, 3] == -1.0     # Z = 1.5: sdf exactly -trunc counts, t = -1
    assert ref["tsdf"][4, 3, 3] == 0.0 and ref["tsdf"][3, 3, 3] == 1.0      # Z = 1: sdf 0; Z = 0.5: sdf = trunc, t = 1
    assert np.array_equal(ref["color"][5, 3, 3], [0.25, 0.25, 0.25])
    ref = run(below)
    assert ref["weight"][5, 3, 3] == 0 and ref["weight"][4, 3, 3] == 1      # just below -trunc: skipped
    ref = run(1.75)
    assert ref["tsdf"][3, 3, 3] == 1.0 and ref["weight"][3, 3, 3] == 1      # sdf = 1.25 > trunc: clamped to 1
    # w_max reached, and a view without colour into a colour volume (the weight moves, the colour stays)
    vol, ref0, _ = _volume(G, s=s, origin=origin, trunc=trunc, w_max=2.5)
    zs = [np.full((H, W), v, np.float32) for v in (1.0, 1.2, 1.4, 1.1, 1.3)]
    cols = [col, None, col * 2, None, None]
    vol.integrate_views(zs, [cam] * 5, cols, weights=[1.0, 1.0, 1.0, 0.5, 2.0])
    ref = R.integrate(ref0, [R.make_view(z, cam, c, w) for z, c, w in zip(zs, cols, (1.0, 1.0, 1.0, 0.5, 2.0))], trunc, w_max=2.5)
    _same_volume(vol, ref, "w_max")
    assert ref["weight"].max() == 2.5 and (ref["weight"] == 2.5).sum() > 3
    one = R.integrate(ref0, [R.make_view(zs[0], cam, col), R.make_view(zs[1], cam, None)], trunc)
    assert one["weight"][4, 3, 3] == 2 and np.array_equal(one["color"][4, 3, 3], [0.25, 0.25, 0.25])


def test_same_bits_whatever_the_memory_held_and_on_a_side_stream(fused):
    G = CASES[2][0]
    (cams, depths, colors, weights), ref = fused[G]
    rv, rc, rk, _ = R.extract(ref, 1.0)
    assert len(rv) > 0
    side = torch.cuda.Stream(device=_dev())
    vol, _, _ = _volume(G, w_max=6.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for t in (vol.tsdf, vol.weight, vol.color, vol._total):
            t.view(torch.uint8).fill_(255)
        vol._ws.fill_(255)
        vol.reset()
        vol.integrate_views(depths, cams, colors, depth_max=2.9, weights=weights)
        _same_volume(vol, ref, "0xFF, side stream")
        _same_mesh(vol, ref, 1.0, "0xFF, side stream")
    side.synchronize()


def _set(vol, ref):
    vol.tsdf.copy_(torch.as_tensor(ref["tsdf"]))
    vol.weight.copy_(torch.as_tensor(ref["weight"]))
    if ref["color"] is not None:
        vol.color.copy_(torch.as_tensor(ref["color"]))


def test_extraction_edge_cases():
    G = (9, 5, 3)
    rng = np.random.default_rng(5)
    vol, ref0, _ = _volume(G)
    ref0["color"][...] = rng.uniform(0, 1, ref0["color"].shape).astype(np.float32)
    ones = np.ones(ref0["tsdf"].shape, np.float32)
    for name, ts, w in (("all outside", ones, ones), ("all inside", -ones, ones), ("exact zeros are outside", 0 * ones, ones),
                        ("no weight", rng.normal(size=ones.shape).astype(np.float32), 0 * ones)):
        ref = dict(ref0, tsdf=ts, weight=w)
        _set(vol, ref)
        rv, _, _, _ = _same_mesh(vol, ref, 1.0, name)
        assert len(rv) == 0, name
    # random signs: every mixed case of a tetrahedron occurs
    ref = dict(ref0, tsdf=rng.normal(size=ones.shape).astype(np.float32), weight=ones.copy())
    _set(vol, ref)
    rv, _, rk, tally = _same_mesh(vol, ref, 1.0, "random signs")
    assert (tally.sum(0)[1:15] > 0).all(), tally.sum(0)
    full = len(rv)
    # min_weight gates a cell by each of its corners: one corner just below it silences the (up to) eight cells around it
    gated = dict(ref, weight=ones.copy())
    gated["weight"][1, 2, 4] = np.nextafter(np.float32(1.0), np.float32(0.0))
    _set(vol, gated)
    gv, _, gk, _ = _same_mesh(vol, gated, 1.0, "one corner below min_weight")
    assert 0 < len(gv) < full
    cells = {(z * 4 + y) * 8 + x for z in (0, 1) for y in (1, 2) for x in (3, 4)}       # the cells that have (4, 2, 1) as a corner
    expect = [i for i in range(full) if _cell_of_triangle(ref, rv[i]) not in cells]
    _same(gv, rv[expect], "gated triangles are the others, unchanged")
    _same_mesh(vol, gated, float(np.nextafter(np.float32(1.0), np.float32(0.0))), "min_weight at the corner's weight")   # >= : the corner counts again
    # corners at exactly 0 and -0: outside; their crossed edges put the vertices on the corner, zero-area triangles included
    zeros = dict(ref, tsdf=ref["tsdf"].copy())
    zeros["tsdf"][1, 2, 4], zeros["tsdf"][1, 1, 2], zeros["tsdf"][0, 3, 6] = 0.0, -0.0, 0.0
    _set(vol, zeros)
    zv, _, zk, _ = _same_mesh(vol, zeros, 1.0, "zero corners")
    area = np.linalg.norm(np.cross(zv[:, 1] - zv[:, 0], zv[:, 2] - zv[:, 0]), axis=1)
    assert (area == 0).any() and np.isfinite(zv).all()
    verts, faces, _ = R.weld(zv, zk)
    repeated, unmatched, *_ = R.directed_edge_census(faces)
    assert repeated == 0                                                                 # consistently oriented (open at the grid's faces)
    # a volume without colour: colours are None from Python, zeros from the library
    nvol, nref, _ = _volume(G, color=False)
    nref = dict(nref, tsdf=ref["tsdf"], weight=ones)
    _set(nvol, nref)
    _same_mesh(nvol, nref, 1.0, "no colour")


def test_extraction_over_more_than_one_scan_run():
    """More than GSR_MESH_SCAN_GROUPS workgroups of cells: the second level of the offset scan carries into the second run."""
    G = (80, 70, 60)
    assert -(-(79 * 69 * 59) // R.GROUP_CELLS) > R.SCAN_GROUPS
    vol, ref0, _ = _volume(G, s=0.02, color=False)
    ref = R.fill_sdf(ref0, R.sphere_sdf((0.03, -0.02, 0.05), 0.52))                      # crosses the cells of both runs
    _set(vol, ref)
    rv, _, rk, _ = _same_mesh(vol, ref, 1.0, "two scan runs")
    cells = rk[:, 0] // R.DIRECTIONS // (80 * 70)                                        # z of each triangle's first vertex
    assert len(rv) > 10000 and cells.min() < 20 and cells.max() > 40
    verts, faces, _ = R.weld(rv, rk)
    assert R.directed_edge_census(faces)[:2] == (0, 0)                                   # closed and oriented


def _cell_of_triangle(ref, tri):
    """The linear index of the cell a triangle of the restatement lies in (its centroid's cell)."""
    Gx, Gy, Gz = ref["dims"]
    c = (tri.astype(np.float64).mean(0) - ref["origin"].astype(np.float64)) / float(ref["voxel_size"])
    x, y, z = (int(np.floor(v)) for v in c)
    return (z * (Gy - 1) + y) * (Gx - 1) + x


def _raw(vol):
    _lib = sub("_lib")
    return _lib, _lib.lib(), vol._struct()


def test_capacity_below_the_count_writes_nothing_past_it():
    G = (17, 16, 15)
    rng = np.random.default_rng(11)
    vol, ref0, _ = _volume(G)
    ref = dict(ref0, tsdf=rng.normal(size=ref0["tsdf"].shape).astype(np.float32), weight=np.ones(ref0["tsdf"].shape, np.float32),
               color=rng.uniform(0, 1, ref0["color"].shape).astype(np.float32))
    _set(vol, ref)
    rv, rc, rk, _ = R.extract(ref, 1.0)
    T = len(rv)
    assert T > 3000                                                                      # several workgroups, several scan entries
    _lib, L, v = _raw(vol)
    for cap in (0, 1, T // 2, T - 1, T, T + 5):
        total = torch.full((1,), -1, dtype=torch.int64, device=_dev())
        vertices = torch.full((T + 5, 3, 3), -7.0, device=_dev())
        colors = torch.full((T + 5, 3, 3), -7.0, device=_dev())
        keys = torch.full((T + 5, 3), -7, dtype=torch.int64, device=_dev())
        vol._ws.fill_(255)
        assert L.gsr_mesh_count(C.byref(v), 1.0, vol._ws.data_ptr(), vol._ws.numel(), total.data_ptr(), None) == 0
        assert L.gsr_mesh_emit(C.byref(v), 1.0, vol._ws.data_ptr(), vol._ws.numel(), cap, vertices.data_ptr(), colors.data_ptr(), keys.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(total.item()) == T                                                    # the count does not depend on the capacity
        n = min(cap, T)
        _same(vertices[:n], rv[:n], f"cap {cap} vertices")
        _same(colors[:n], rc[:n], f"cap {cap} colors")
        _same(keys[:n], rk[:n], f"cap {cap} keys")
        assert (vertices[n:] == -7.0).all() and (colors[n:] == -7.0).all() and (keys[n:] == -7).all(), cap
    # colours are optional
    vertices = torch.full((T, 3, 3), -7.0, device=_dev())
    keys = torch.full((T, 3), -7, dtype=torch.int64, device=_dev())
    assert L.gsr_mesh_emit(C.byref(v), 1.0, vol._ws.data_ptr(), vol._ws.numel(), T, vertices.data_ptr(), None, keys.data_ptr(), None) == 0
    _same(vertices, rv, "no colour output")
    _same(keys, rk, "no colour output keys")


def test_every_refused_argument_returns_its_code_and_enqueues_nothing():
    G = (9, 5, 3)
    rng = np.random.default_rng(2)
    vol, ref0, trunc = _volume(G)
    ref = dict(ref0, tsdf=rng.normal(size=ref0["tsdf"].shape).astype(np.float32), weight=np.ones(ref0["tsdf"].shape, np.float32))
    _set(vol, ref)
    _lib, L, v = _raw(vol)
    E = _lib
    T = len(R.extract(ref, 1.0)[0])
    z = torch.full((3, 5), 2.5, device=_dev())
    out = torch.full((3, 5), -7.0, device=_dev())
    total = torch.full((2,), -7, dtype=torch.int64, device=_dev())
    vertices = torch.full((T, 3, 3), -7.0, device=_dev())
    keys = torch.full((T, 3), -7, dtype=torch.int64, device=_dev())
    vol._ws.fill_(255)
    ws, wsb = vol._ws.data_ptr(), vol._ws.numel()
    need = int(L.gsr_mesh_workspace_bytes(*G))

    def view(**kw):
        a = (_lib.GsrTsdfView * 1)()
        a[0].depth, a[0].color = z.data_ptr(), None
        a[0].view[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
        a[0].tan_fovx, a[0].tan_fovy, a[0].W, a[0].H, a[0].w_obs = 0.5, 0.5, 5, 3, 1.0
        for k, val in kw.items():
            setattr(a[0], k, val)
        return a

    def vstruct(**kw):
        s = vol._struct()
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    calls = [
        (E.GSR_E_NULL, lambda: L.gsr_tsdf_reset(vstruct(tsdf=None), None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_reset(vstruct(Gx=0), None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_reset(vstruct(voxel_size=NAN), None)),
        (E.GSR_E_ALIGN, lambda: L.gsr_tsdf_reset(vstruct(weight=vol.weight.data_ptr() + 4), None)),
        (E.GSR_E_NULL, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, None, trunc, INF, INF, None)),
        (E.GSR_E_NULL, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(depth=None), trunc, INF, INF, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_integrate(C.byref(v), 0, view(), trunc, INF, INF, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(), 0.0, INF, INF, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(), trunc, NAN, INF, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(), trunc, INF, 0.0, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(w_obs=0.0), trunc, INF, INF, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(W=0), trunc, INF, INF, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(tan_fovy=-1.0), trunc, INF, INF, None)),
        (E.GSR_E_ALIGN, lambda: L.gsr_tsdf_integrate(C.byref(v), 1, view(depth=z.data_ptr() + 4), trunc, INF, INF, None)),
        (E.GSR_E_ALIGN, lambda: L.gsr_tsdf_integrate(vstruct(color=vol.color.data_ptr() + 8), 1, view(), trunc, INF, INF, None)),
        (E.GSR_E_NULL, lambda: L.gsr_mesh_count(C.byref(v), 1.0, None, wsb, total.data_ptr(), None)),
        (E.GSR_E_NULL, lambda: L.gsr_mesh_count(C.byref(v), 1.0, ws, wsb, None, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_mesh_count(C.byref(v), 0.0, ws, wsb, total.data_ptr(), None)),
        (E.GSR_E_ALIGN, lambda: L.gsr_mesh_count(C.byref(v), 1.0, ws + 8, wsb, total.data_ptr(), None)),
        (E.GSR_E_ALIGN, lambda: L.gsr_mesh_count(C.byref(v), 1.0, ws, wsb, total.data_ptr() + 4, None)),
        (E.GSR_E_WORKSPACE, lambda: L.gsr_mesh_count(C.byref(v), 1.0, ws, need - 1, total.data_ptr(), None)),
        (E.GSR_E_NULL, lambda: L.gsr_mesh_emit(C.byref(v), 1.0, ws, wsb, T, None, None, keys.data_ptr(), None)),
        (E.GSR_E_NULL, lambda: L.gsr_mesh_emit(C.byref(v), 1.0, ws, wsb, T, vertices.data_ptr(), None, None, None)),
        (E.GSR_E_DIMS, lambda: L.gsr_mesh_emit(C.byref(v), 1.0, ws, wsb, -1, vertices.data_ptr(), None, keys.data_ptr(), None)),
        (E.GSR_E_DIMS, lambda: L.gsr_mesh_emit(C.byref(v), NAN, ws, wsb, T, vertices.data_ptr(), None, keys.data_ptr(), None)),
        (E.GSR_E_ALIGN, lambda: L.gsr_mesh_emit(C.byref(v), 1.0, ws, wsb, T, vertices.data_ptr() + 4, None, keys.data_ptr(), None)),
        (E.GSR_E_WORKSPACE, lambda: L.gsr_mesh_emit(C.byref(v), 1.0, ws, need - 1, T, vertices.data_ptr(), None, keys.data_ptr(), None)),
        (E.GSR_E_NULL, lambda: L.gsr_tsdf_depth(z.data_ptr(), None, 5, 3, 0.5, out.data_ptr(), None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_depth(z.data_ptr(), z.data_ptr(), 0, 3, 0.5, out.data_ptr(), None)),
        (E.GSR_E_DIMS, lambda: L.gsr_tsdf_depth(z.data_ptr(), z.data_ptr(), 5, 3, NAN, out.data_ptr(), None)),
        (E.GSR_E_ALIGN, lambda: L.gsr_tsdf_depth(z.data_ptr(), z.data_ptr(), 5, 3, 0.5, out.data_ptr() + 4, None)),
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, k
    torch.cuda.synchronize()
    _same_volume(vol, ref, "after the refused calls")                                    # nothing was enqueued: nothing changed
    assert (vol._ws == 255).all() and (total == -7).all() and (vertices == -7.0).all() and (keys == -7).all() and (out == -7.0).all()
    assert int(L.gsr_mesh_workspace_bytes(*G)) == R.workspace_bytes(*G)
    # and the Python surface turns a library refusal into an exception
    with pytest.raises(ValueError):
        vol.integrate(z, {"world_to_camera": np.eye(4), "tan_fovx": 0.5, "tan_fovy": 0.5, "width": 5, "height": 3}, weight=0.0)


def test_depth_from_buffers_follows_the_normals_rule():
    rng = np.random.default_rng(9)
    H, W = 29, 37
    D = rng.uniform(0.05, 2.0, (H, W)).astype(np.float32)
    T = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    D[0, :6] = (0.0, -1.0, NAN, INF, 1e-30, 3.0)
    T[1, :6] = (0.5, np.nextafter(np.float32(0.5), np.float32(1.0)), NAN, -INF, 1.0, 0.0)
    with np.errstate(all="ignore"):
        A = np.float32(1.0) - T
        want = np.where(np.isfinite(A) & np.isfinite(D) & (A >= np.float32(0.5)) & (D > 0), A / D, np.float32(0.0)).astype(np.float32)
    got = sub("tsdf").depth_from_buffers(torch.as_tensor(D).to(_dev()), torch.as_tensor(T).to(_dev()))
    _same(got, want, "depth_from_buffers")
    assert want[1, 0] > 0 and want[1, 1] == 0 and (want[0, :4] == 0).all()
    _same(sub("tsdf").depth_from_buffers(D.reshape(H, W, 1), T, alpha_min=0.9), np.where(A >= np.float32(0.9), want, np.float32(0)), "alpha_min 0.9")


def test_end_to_end_on_the_trainers_hidden_scene():
    from conftest import render_kwargs
    gsr, tsdf = pkg(), sub("tsdf")
    size, views, G = 100, 8, 48
    hidden = gsr.scenes.synthetic_scene(5000, 0.05, 0.5, seed=7)                         # examples/train.py's hidden scene
    cams = [gsr.cameras.nerf_camera(gsr.scenes.orbit_pose(k, views), size, size, gsr.scenes.LEGO_CAMERA_ANGLE_X) for k in range(views)]
    depths, colors = [], []
    for c in cams:
        image, depth, buffers = gsr.render_gaussians(**render_kwargs(hidden, c))
        depths.append(tsdf.depth_from_buffers(depth.reshape(size, size), buffers["final_Ts"].reshape(size, size)))
        colors.append(image.reshape(size, size, 3).clone())
    s = 3.0 / (G - 1)
    vol = tsdf.TSDFVolume((-1.5, -1.5, -1.5), s, (G, G, G), device=_dev())
    vol.integrate_views(depths, cams, colors)
    views_np = [R.make_view(z.cpu().numpy(), c, col.cpu().numpy()) for z, c, col in zip(depths, cams, colors)]
    ref = R.integrate(R.new_volume((-1.5, -1.5, -1.5), s, (G, G, G)), views_np, vol.trunc)
    _same_volume(vol, ref, "hidden scene")
    rv, rc, rk, _ = _same_mesh(vol, ref, 1.0, "hidden scene")
    assert len(rv) > 1000 and np.isfinite(rv).all() and np.isfinite(rc).all()
    lo, hi = -1.5, -1.5 + s * (G - 1)
    assert rv.min() >= lo - 1e-5 and rv.max() <= hi + 1e-5                               # every vertex lies inside the volume
    vertices, vcolors, keys = vol.extract_mesh(1.0)
    verts, faces, cols = tsdf.weld(vertices, keys, vcolors)
    wv, wf, wc = R.weld(rv, rk, rc)
    _same(verts, wv, "welded vertices")
    assert np.array_equal(faces, wf) and np.array_equal(cols, wc)
    assert R.directed_edge_census(faces)[0] == 0                                         # no directed edge twice: consistently oriented
