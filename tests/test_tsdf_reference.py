"""The TSDF yardstick (tests/tsdf_reference.py) has to mean something before the kernels are held to it bit for bit: its marching
tetrahedra give closed, consistently oriented surfaces of the right topology, volume and place on analytic signed-distance fields, every
tetrahedron meets all 14 mixed sign cases, cells that share an edge agree on its vertex bits and key, and its float32 fusion of
analytic sphere depth maps agrees with its float64 twin.  The two measured margins live in tests/golden/tsdf_margins.json
(`python tests/test_tsdf_reference.py` prints them as measured here; the tests allow twice the recorded values)."""
import functools
import json
import os

import numpy as np

import tsdf_reference as R

MARGINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsdf_margins.json")
CENTRE = (0.137, -0.071, 0.053)                 # off the grid's symmetry planes
SPHERE_R, TORUS_R, TORUS_r = 0.8, 0.55, 0.25
SPHERE_GRIDS = ((23, 0.09), (37, 0.055))        # (voxels per axis, voxel size): two resolutions


def _volume(G, s, color=False):
    return R.new_volume((-0.5 * s * (G - 1) + 0.013,) * 3, s, (G, G + 1, G - 1), color=color)


@functools.lru_cache(maxsize=None)
def _analytic(shape, G, s):
    sdf = R.sphere_sdf(CENTRE, SPHERE_R) if shape == "sphere" else R.torus_sdf(CENTRE, TORUS_R, TORUS_r)
    vol = R.fill_sdf(_volume(G, s), sdf)
    vertices, colors, keys, tally = R.extract(vol, 1.0)
    verts, faces, _ = R.weld(vertices, keys)
    return vol, sdf, vertices, keys, tally, verts, faces


@functools.lru_cache(maxsize=None)
def _fused():
    G, s = 32, 0.07
    vol = _volume(G, s, color=True)
    trunc = float(np.float32(4 * s))               # the float32 the integrator takes
    views = []
    for k, d in enumerate([(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]):
        eye = np.asarray(CENTRE) + 3.0 * np.asarray(d, np.float64) / np.sqrt(3.0) + 0.05 * k
        cam = R.look_at_camera(eye, CENTRE, 96, 80, 0.45)
        depth = R.sphere_depth(cam, CENTRE, SPHERE_R, background=10.0)   # a backdrop: the free space beside the silhouette is observed
        color = np.broadcast_to(np.asarray([0.2 + 0.1 * k, 0.5, 0.9 - 0.1 * k], np.float32), depth.shape + (3,))
        views.append(R.make_view(depth, cam, color))
    f32 = R.integrate(vol, views, trunc)
    f64 = R.integrate(vol, views, trunc, float64=True)
    return vol, trunc, views, f32, f64


def measured_margins():
    rel = []
    for G, s in SPHERE_GRIDS:
        _, _, _, _, _, verts, faces = _analytic("sphere", G, s)
        rel.append(abs(R.signed_volume(verts, faces) / (4.0 / 3.0 * np.pi * SPHERE_R ** 3) - 1.0))
    _, trunc, _, f32, f64 = _fused()
    band = (f32["weight"] > 0) & (np.abs(f32["tsdf"]) < 1)
    dist = np.abs(f32["tsdf"].astype(np.float64) * trunc - f64["tsdf"] * trunc)[band]
    return {"sphere_volume_rel_error": float(max(rel)), "fused_sdf_abs_error": float(dist.max()), "fused_band_voxels": int(band.sum())}


def _recorded():
    with open(MARGINS) as f:
        return json.load(f)


def test_analytic_surfaces_are_closed_oriented_and_of_the_right_topology():
    seen = np.zeros((6, 16), np.int64)
    for shape, euler, grids in (("sphere", 2, SPHERE_GRIDS), ("torus", 0, SPHERE_GRIDS)):
        for G, s in grids:
            vol, sdf, vertices, keys, tally, verts, faces = _analytic(shape, G, s)
            assert len(faces) > 500
            repeated, unmatched, nv, ne, nf = R.directed_edge_census(faces)
            assert repeated == 0 and unmatched == 0, (shape, G)          # every edge: two triangles, once in each direction
            assert nv == len(verts) and nv - ne + nf == euler, (shape, G, nv, ne, nf)
            assert R.signed_volume(verts, faces) > 0, (shape, G)         # normals point outwards, into positive tsdf
            assert np.abs(sdf(verts.astype(np.float64))).max() <= s * np.sqrt(3.0), (shape, G)
            seen += tally
    assert (seen[:, 1:15] > 0).all(), seen                               # every tetrahedron met all 14 mixed cases
    assert (seen[:, 0] > 0).all() and (seen[:, 15] > 0).all()


def test_sphere_volume_error_is_within_twice_the_recorded_margin():
    m, rec = measured_margins(), _recorded()
    assert 0 < rec["sphere_volume_rel_error"] < 0.02                     # a linear interpolant of a curved surface at 18-29 voxels per diameter
    assert m["sphere_volume_rel_error"] <= 2 * rec["sphere_volume_rel_error"], m


def test_fused_sphere_matches_the_float64_restatement_and_extracts_closed():
    vol, trunc, views, f32, f64 = _fused()
    m, rec = measured_margins(), _recorded()
    assert m["fused_band_voxels"] > 1000
    assert 0 < rec["fused_sdf_abs_error"] < 1e-5 * trunc                 # a few float32 roundings of numbers of size 3 (the depths): far below a voxel
    assert m["fused_sdf_abs_error"] <= 2 * rec["fused_sdf_abs_error"], m
    assert np.array_equal(f32["weight"].astype(np.float64), f64["weight"])      # same decisions: the same views counted
    # along z the fused value IS the signed distance where one view alone saw the voxel
    once = (f32["weight"] == 1) & (np.abs(f32["tsdf"]) < 1)
    assert once.sum() > 100 and np.abs(f64["tsdf"][once] * trunc - f64["sdf_z"][once]).max() <= 1e-12
    vertices, colors, keys, _ = R.extract(f32, 1.0)
    verts, faces, cols = R.weld(vertices, keys, colors)
    repeated, unmatched, nv, ne, nf = R.directed_edge_census(faces)
    assert nf > 500 and repeated == 0 and unmatched == 0
    assert R.signed_volume(verts, faces) > 0
    assert np.isfinite(verts).all() and np.isfinite(cols).all() and cols.min() >= 0.0 and cols.max() <= 1.0
    near = np.abs(np.linalg.norm(verts.astype(np.float64) - np.asarray(CENTRE), axis=1) - SPHERE_R)
    assert np.median(near) < vol["voxel_size"]                           # the fused surface is the sphere


def test_cells_that_share_an_edge_agree_on_its_bits_and_key():
    for shape in ("sphere", "torus"):
        _, _, vertices, keys, _, _, _ = _analytic(shape, *SPHERE_GRIDS[0])
        k, v = keys.reshape(-1), vertices.reshape(-1, 3).view(np.uint32)
        order = np.argsort(k, kind="stable")
        k, v = k[order], v[order]
        same = k[1:] == k[:-1]
        assert same.sum() > len(k) // 2                                  # every vertex is shared
        assert (v[1:][same] == v[:-1][same]).all()
    _, _, _, f32, _ = _fused()
    vertices, colors, keys, _ = R.extract(f32, 1.0)
    k = keys.reshape(-1)
    rec = np.concatenate([vertices.reshape(-1, 3), colors.reshape(-1, 3)], axis=1).view(np.uint32)
    order = np.argsort(k, kind="stable")
    same = k[order][1:] == k[order][:-1]
    assert (rec[order][1:][same] == rec[order][:-1][same]).all()
    assert k.min() >= 0 and (k % R.DIRECTIONS).max() <= 6


def test_workspace_formula_and_reference_weld():
    assert R.workspace_bytes(1, 1, 1) == R.workspace_bytes(2, 2, 2) == 512
    assert R.workspace_bytes(512, 512, 512) == -(-4 * -(-511 ** 3 // 256) // 256) * 256 + -(-8 * -(-(-(-511 ** 3 // 256)) // 1024) // 256) * 256
    assert R.workspace_bytes(0, 5, 5) == R.workspace_bytes(2049, 1, 1) == R.workspace_bytes(2048, 2048, 1024) == 0
    verts, faces, cols = R.weld(np.arange(18, dtype=np.float32).reshape(2, 3, 3), np.array([[5, 3, 9], [3, 5, 7]]))
    assert faces.tolist() == [[1, 0, 3], [0, 1, 2]] and verts[0].tolist() == [3.0, 4.0, 5.0] and cols is None


if __name__ == "__main__":
    print(json.dumps(measured_margins(), indent=1))
