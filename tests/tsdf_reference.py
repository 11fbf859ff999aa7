"""A numpy restatement of include/gsr_tsdf.h, written from the header's text: the yardstick of tests/test_gpu_tsdf.py (bit for bit)
and the subject of tests/test_tsdf_reference.py, which holds it to analytic surfaces first.

    integrate(vol, views, trunc, depth_max, w_max)            float32, every step one rounded operation in the header's order
    integrate(..., float64=True)                              the same decisions (pixel, skips, the clamp, the weight cap), taken from the
                                                              float32 values; only the values are float64
    extract(vol, min_weight)                                  marching tetrahedra: (vertices, colors, keys, tally of the 16 sign cases)
    weld(vertices, keys, colors)                              indexed mesh by key

A volume is a dict: origin (3,) float32, voxel_size, dims (Gx, Gy, Gz), tsdf / weight (Gz, Gy, Gx), color (Gz, Gy, Gx, 3) or None.
A view is a dict: depth (H, W), color (H, W, 3) or None, view (16,) row-vector world_to_camera, tan_fovx, tan_fovy, W, H, w_obs."""
import itertools

import numpy as np

F = np.float32
VIEWS_PER_LAUNCH, GROUP_CELLS, SCAN_GROUPS, DIRECTIONS = 16, 256, 1024, 7          # the header's constants
DIRECTION_OF_BITS = {1: 0, 2: 1, 4: 2, 3: 3, 5: 4, 6: 5, 7: 6}                      # (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
PERMS = list(itertools.permutations((0, 1, 2)))                                     # lexicographic: 012 021 102 120 201 210
OTHERS = {0: (1, 2, 3), 1: (0, 3, 2), 2: (3, 0, 1), 3: (2, 1, 0)}


def new_volume(origin, voxel_size, dims, color=True):
    Gx, Gy, Gz = dims
    return {"origin": np.asarray(origin, F), "voxel_size": F(voxel_size), "dims": (int(Gx), int(Gy), int(Gz)),
            "tsdf": np.ones((Gz, Gy, Gx), F), "weight": np.zeros((Gz, Gy, Gx), F), "color": np.zeros((Gz, Gy, Gx, 3), F) if color else None}


def make_view(depth, camera, color=None, w_obs=1.0):
    """A view record from a cameras.nerf_camera-style dict."""
    H, W = np.shape(depth)[:2]
    return {"depth": np.asarray(depth, F).reshape(H, W), "color": None if color is None else np.asarray(color, F).reshape(H, W, 3),
            "view": np.asarray(camera["world_to_camera"], F).reshape(16), "tan_fovx": F(camera["tan_fovx"]), "tan_fovy": F(camera["tan_fovy"]),
            "W": int(W), "H": int(H), "w_obs": F(w_obs)}


def workspace_bytes(Gx, Gy, Gz):
    if not (1 <= min(Gx, Gy, Gz) and max(Gx, Gy, Gz) <= 2048 and Gx * Gy * Gz <= 1 << 31):
        return 0
    groups = max(1, -(-((Gx - 1) * (Gy - 1) * (Gz - 1)) // GROUP_CELLS))
    return -(-4 * groups // 256) * 256 + -(-8 * -(-groups // SCAN_GROUPS) // 256) * 256


def _centres(vol, dtype):
    Gx, Gy, Gz = vol["dims"]
    o, s = vol["origin"].astype(dtype), dtype(vol["voxel_size"])
    X = (o[0] + s * np.arange(Gx, dtype=dtype))[None, None, :]
    Y = (o[1] + s * np.arange(Gy, dtype=dtype))[None, :, None]
    Z = (o[2] + s * np.arange(Gz, dtype=dtype))[:, None, None]
    return X, Y, Z


def _project(XYZ, V, dtype):
    X, Y, Z = XYZ
    V = V.astype(dtype)
    return [((X * V[0 + c] + Y * V[4 + c]) + Z * V[8 + c]) + V[12 + c] for c in range(3)]


def integrate(vol, views, trunc, depth_max=np.inf, w_max=np.inf, float64=False):
    """The volume after the views, in order.  Returns a new volume dict; with float64=True its tsdf, weight and color are float64
    values under the float32 run's decisions, and "sdf_z" holds the last accepted view's float64 d - p_z (NaN where none)."""
    trunc, depth_max, w_max = F(trunc), F(depth_max), F(w_max)
    out = dict(vol, tsdf=vol["tsdf"].copy(), weight=vol["weight"].copy(), color=None if vol["color"] is None else vol["color"].copy())
    ts, w, col = out["tsdf"], out["weight"], out["color"]
    c32 = _centres(vol, F)
    if float64:
        D = np.float64
        ts64, w64, col64 = ts.astype(D), w.astype(D), None if col is None else col.astype(D)
        c64 = _centres(vol, D)
    with np.errstate(all="ignore"):
        for q in views:
            W, H = q["W"], q["H"]
            px, py, pz = _project(c32, q["view"], F)
            ok = (pz > 0) & np.isfinite(pz)
            u = ((px / (pz * q["tan_fovx"]) + F(1)) * F(W) - F(1)) * F(0.5)
            v = ((py / (pz * q["tan_fovy"]) + F(1)) * F(H) - F(1)) * F(0.5)
            fu, fv = np.floor(u + F(0.5)), np.floor(v + F(0.5))
            ok &= (fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H))
            x, y = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
            d = q["depth"][y, x]
            ok &= np.isfinite(d) & (d > 0) & (d <= depth_max)
            sdf = d - pz
            ok &= ~(sdf < -trunc)
            ratio = sdf / trunc
            clamp = ~(ratio < F(1))                      # fminf(1, ratio): 1 unless ratio < 1 (a NaN ratio cannot occur: trunc > 0, sdf not NaN)
            t = np.where(clamp, F(1), ratio)
            wo = q["w_obs"]
            w1 = w + wo
            has_col = col is not None and q["color"] is not None
            if float64:
                _, _, pz64 = _project(c64, q["view"], D)
                sdf64 = d.astype(D) - pz64
                t64 = np.where(clamp, 1.0, sdf64 / D(trunc))
                w1_64 = w64 + D(wo)
                ts64 = np.where(ok, (ts64 * w64 + t64 * D(wo)) / w1_64, ts64)
                if has_col:
                    c = q["color"][y, x].astype(D)
                    col64 = np.where(ok[..., None], (col64 * w64[..., None] + c * D(wo)) / w1_64[..., None], col64)
                w64 = np.where(ok, np.where(w1 > w_max, D(w_max), w1_64), w64)
                out["sdf_z"] = np.where(ok, sdf64, out.get("sdf_z", np.full(ts.shape, np.nan)))
            ts[...] = np.where(ok, (ts * w + t * wo) / w1, ts)
            if has_col:
                c = q["color"][y, x]
                col[...] = np.where(ok[..., None], (col * w[..., None] + c * wo) / w1[..., None], col)
            w[...] = np.where(ok, np.minimum(w1, w_max), w)
    if float64:
        out.update(tsdf=ts64, weight=w64, color=col64)
    return out


# ---- marching tetrahedra ----
def _corner(a, k):
    Gz, Gy, Gx = a.shape[:3]
    dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
    return a[dz:Gz - 1 + dz, dy:Gy - 1 + dy, dx:Gx - 1 + dx]


def _edge_vertex(vol, cells, cp, cq):
    """(positions (n, 3), colours (n, 3), keys (n,)) of the edge from corner code cp to corner code cq of the cells (ix, iy, iz)."""
    Gx, Gy, Gz = vol["dims"]
    o, s = vol["origin"], F(vol["voxel_size"])
    P = [cells[c] + ((cp >> c) & 1) for c in range(3)]
    bits = cq ^ cp
    Dr = [(bits >> c) & 1 for c in range(3)]
    a = vol["tsdf"][P[2], P[1], P[0]]
    b = vol["tsdf"][P[2] + Dr[2], P[1] + Dr[1], P[0] + Dr[0]]
    with np.errstate(all="ignore"):
        t = a / (a - b)
        pos = np.stack([(o[c] + s * P[c].astype(F)) + t * (s * F(Dr[c])) for c in range(3)], axis=1)
        if vol["color"] is not None:
            ca, cb = vol["color"][P[2], P[1], P[0]], vol["color"][P[2] + Dr[2], P[1] + Dr[1], P[0] + Dr[0]]
            col = (F(1) - t)[:, None] * ca + t[:, None] * cb
        else:
            col = np.zeros((len(t), 3), F)
    key = ((P[2].astype(np.int64) * Gy + P[1]) * Gx + P[0]) * DIRECTIONS + DIRECTION_OF_BITS[bits]
    return pos.astype(F), col.astype(F), key


def extract(vol, min_weight):
    """(vertices (T, 3, 3) float32, colors (T, 3, 3) float32 (zeros without volume colour), keys (T, 3) int64, tally (6, 16) int64: how
    often each tetrahedron met each sign case over the active cells), triangles in cell, tetrahedron, triangle order."""
    Gx, Gy, Gz = vol["dims"]
    tally = np.zeros((6, 16), np.int64)
    empty = (np.zeros((0, 3, 3), F), np.zeros((0, 3, 3), F), np.zeros((0, 3), np.int64), tally)
    if min(Gx, Gy, Gz) < 2:
        return empty
    active = np.ones((Gz - 1, Gy - 1, Gx - 1), bool)
    for k in range(8):
        active &= _corner(vol["weight"], k) >= F(min_weight)
    iz, iy, ix = np.nonzero(active)                       # ascending linear cell index
    if len(ix) == 0:
        return empty
    cell_id = (iz.astype(np.int64) * (Gy - 1) + iy) * (Gx - 1) + ix
    inside = [(_corner(vol["tsdf"], k) < 0)[iz, iy, ix] for k in range(8)]
    chunks = []                                           # (cell id, tetrahedron, triangle, pos (n, 3, 3), col, key (n, 3))
    for tet, (a, b, _) in enumerate(PERMS):
        codes = (0, 1 << a, (1 << a) | (1 << b), 7)
        neg = tet in (1, 2, 5)                            # sigma: + - - + + -
        m = sum(inside[codes[i]].astype(np.int64) << i for i in range(4))
        tally[tet] = np.bincount(m, minlength=16)
        for case in range(1, 15):
            sel = np.nonzero(m == case)[0]
            if len(sel) == 0:
                continue
            cells = (ix[sel], iy[sel], iz[sel])
            ins = [i for i in range(4) if case >> i & 1]
            outs = [i for i in range(4) if not case >> i & 1]

            def e(p, q):
                return _edge_vertex(vol, cells, codes[min(p, q)], codes[max(p, q)])
            if len(ins) != 2:
                L = ins[0] if len(ins) == 1 else outs[0]
                j, k, l = OTHERS[L]
                tri = [e(L, j), e(L, k), e(L, l)]
                if neg != (len(ins) == 3):
                    tri = [tri[0], tri[2], tri[1]]
                tris = [tri]
            else:
                (i, j), (k, l) = ins, outs
                cyc = [e(i, k), e(i, l), e(j, l), e(j, k)]
                if neg != ((i, j) in ((0, 2), (1, 3))):
                    cyc = [cyc[0], cyc[3], cyc[2], cyc[1]]
                keys4 = np.stack([c[2] for c in cyc], axis=1)
                rot = (np.argmin(keys4, axis=1)[:, None] + np.arange(4)[None, :]) % 4
                pos4 = np.take_along_axis(np.stack([c[0] for c in cyc], axis=1), rot[:, :, None], axis=1)
                col4 = np.take_along_axis(np.stack([c[1] for c in cyc], axis=1), rot[:, :, None], axis=1)
                key4 = np.take_along_axis(keys4, rot, axis=1)
                q = [(pos4[:, n], col4[:, n], key4[:, n]) for n in range(4)]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            for n, tri in enumerate(tris):
                chunks.append((cell_id[sel], np.full(len(sel), tet), np.full(len(sel), n), np.stack([v[0] for v in tri], axis=1),
                               np.stack([v[1] for v in tri], axis=1), np.stack([v[2] for v in tri], axis=1)))
    if not chunks:
        return empty
    cid, tet, tri, pos, col, key = (np.concatenate([c[n] for c in chunks]) for n in range(6))
    order = np.lexsort((tri, tet, cid))
    return pos[order], col[order], key[order], tally


def weld(vertices, keys, colors=None):
    _, first, inverse = np.unique(np.asarray(keys).reshape(-1), return_index=True, return_inverse=True)
    return (np.asarray(vertices).reshape(-1, 3)[first], inverse.reshape(-1, 3).astype(np.int32),
            None if colors is None else np.asarray(colors).reshape(-1, 3)[first])


# ---- what a closed, oriented mesh is ----
def directed_edge_census(faces):
    """(directed edges seen more than once, undirected edges not matched by exactly one edge in each direction, V, E, F) of an indexed
    mesh, degenerate faces included as they come."""
    f = np.asarray(faces, np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if len(f) else 0
    code = de[:, 0] * n + de[:, 1]
    ucode, counts = np.unique(code, return_counts=True)
    repeated = int((counts != 1).sum())
    rev = (ucode % n) * n + ucode // n
    unmatched = int((~np.isin(rev, ucode)).sum())
    und = np.unique(np.minimum(de[:, 0], de[:, 1]) * n + np.maximum(de[:, 0], de[:, 1]))
    return repeated, unmatched, len(np.unique(f)), len(und), len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---- analytic scenes ----
def grid_points(vol):
    """(Gz, Gy, Gx, 3) float64 voxel centres."""
    X, Y, Z = _centres(vol, np.float64)
    Gx, Gy, Gz = vol["dims"]
    return np.stack(np.broadcast_arrays(X, Y, Z), axis=-1).reshape(Gz, Gy, Gx, 3)


def fill_sdf(vol, sdf_of_points, weight=1.0):
    """The volume with tsdf = the analytic signed distance (float32) and a constant weight."""
    return dict(vol, tsdf=sdf_of_points(grid_points(vol)).astype(F), weight=np.full(vol["tsdf"].shape, weight, F))


def sphere_sdf(centre, radius):
    return lambda p: np.linalg.norm(p - np.asarray(centre, np.float64), axis=-1) - radius


def torus_sdf(centre, R, r):
    def f(p):
        q = p - np.asarray(centre, np.float64)
        return np.hypot(np.hypot(q[..., 0], q[..., 1]) - R, q[..., 2]) - r
    return f


def look_at_camera(eye, target, W, H, tan_fov):
    """A camera dict (world_to_camera in row-vector form, +z forward, y down) at `eye` looking at `target`."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0]))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)                       # world -> camera for row vectors: p = (X - eye) R
    M = np.eye(4)
    M[:3, :3] = R
    M[3, :3] = -eye @ R
    return {"world_to_camera": M.astype(F), "tan_fovx": float(tan_fov), "tan_fovy": float(tan_fov * H / W), "width": int(W), "height": int(H),
            "camera_center": eye}


def sphere_depth(camera, centre, radius, background=0.0):
    """(H, W) float32: the view depth (along the camera's +z) of the first hit of every pixel's ray with the sphere, `background` where
    it misses (0: no measurement; a depth behind the volume: a backdrop, so that the free space beside the silhouette is observed)."""
    W, H = camera["width"], camera["height"]
    M = np.asarray(camera["world_to_camera"], np.float64)
    c = np.append(np.asarray(centre, np.float64), 1.0) @ M
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    r = np.ones((H, W, 3))
    r[..., 0] = (((2 * x + 1) / W - 1) * camera["tan_fovx"])[None, :]
    r[..., 1] = (((2 * y + 1) / H - 1) * camera["tan_fovy"])[:, None]
    rr, rc = (r * r).sum(-1), r @ c[:3]
    disc = rc * rc - rr * (c[:3] @ c[:3] - radius * radius)
    with np.errstate(all="ignore"):
        z = (rc - np.sqrt(disc)) / rr                     # the ray is z * r: z is the view depth
    return np.where((disc > 0) & (z > 0), z, background).astype(F)
