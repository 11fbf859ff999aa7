"""
Checkpoint writer: `save_ply` of reference utils/point_cloud_utils.py:10-98,
called from train.py:796-803.  Same vertex layout, field names and byte order as the file the reference writes through
`plyfile` (binary little-endian, packed records): x y z, scale_0..2, opacity, rot_x..w, red green blue (uchar),
f_dc_0..2, f_rest_0..44.  Host I/O only -- the arrays are copied off the device once and packed with numpy, there is
no per-vertex Python loop.  `load_ply` reads such a file back (the reference has no reader; this one exists for
round-trip tests and for resuming from a checkpoint).

`load_points` reads a plain point cloud (x y z and optional uchar colours: what COLMAP and every point-cloud tool write), and
`gaussians_from_points` turns one into the trainer's five arrays with the original's start: isotropic scales from the three nearest
neighbours (knn.init_scales), opacity 0.1, the colour in the SH DC term.
"""
import os

import numpy as np

VERTEX_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("scale_0", "<f4"), ("scale_1", "<f4"), ("scale_2", "<f4"), ("opacity", "<f4"),
     ("rot_x", "<f4"), ("rot_y", "<f4"), ("rot_z", "<f4"), ("rot_w", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
     ("f_dc_0", "<f4"), ("f_dc_1", "<f4"), ("f_dc_2", "<f4")] + [(f"f_rest_{i}", "<f4") for i in range(45)])
_PLY_TYPE = {"f4": "float", "u1": "uchar"}


def _host(x, shape):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    elif hasattr(x, "numpy"):
        x = x.numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).reshape(shape)


def vertex_records(params, num_points, colors=None):
    """The packed vertex table of point_cloud_utils.py:36-91 as one structured array."""
    n = int(num_points)
    pos = _host(params["positions"], (-1, 3))[:n]
    scl = _host(params["scales"], (-1, 3))[:n]
    rot = _host(params["rotations"], (-1, 4))[:n]
    opa = _host(params["opacities"], (-1,))[:n]
    shs = _host(params["shs"], (-1, 16, 3))[:n]
    if colors is not None:
        col = _host(colors, (-1, 3))[:n]
    else:
        # DC term only: clip(sh_dc + 0.5, 0, 1) in float32 (point_cloud_utils.py:28-34)
        col = np.clip(shs[:, 0, :] + np.float32(0.5), np.float32(0.0), np.float32(1.0)).astype(np.float32)
    v = np.zeros(n, dtype=VERTEX_DTYPE)
    v["x"], v["y"], v["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    v["scale_0"], v["scale_1"], v["scale_2"] = scl[:, 0], scl[:, 1], scl[:, 2]
    v["opacity"] = opa
    v["rot_x"], v["rot_y"], v["rot_z"], v["rot_w"] = rot[:, 0], rot[:, 1], rot[:, 2], rot[:, 3]   # stored order, labelled x y z w (:49-50)
    # int(np.clip(c * 255, 0, 255)): float32 product, truncation toward zero (:53-58)
    rgb = np.clip(col * np.float32(255), np.float32(0), np.float32(255)).astype(np.int64)
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    v["f_dc_0"], v["f_dc_1"], v["f_dc_2"] = shs[:, 0, 0], shs[:, 0, 1], shs[:, 0, 2]
    rest = shs[:, 1:, :].reshape(n, 45)          # coefficient-major, channel-minor (:65-69)
    for i in range(45):
        v[f"f_rest_{i}"] = rest[:, i]
    return v


def ply_header(n):
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property {_PLY_TYPE[VERTEX_DTYPE[name].str[1:]]} {name}" for name in VERTEX_DTYPE.names]
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode("ascii")


def save_ply(params, filepath, num_points, colors=None, filter_3d=None):
    """reference utils/point_cloud_utils.py:10 -- same signature, plus `filter_3d`: with the (N,) filter a model was trained under
    (include/gsr_filter3d.h) the file holds the fused scales and opacities (filter3d.apply_filter_3d; Mip-Splatting's
    create_fused_ply), so a standard viewer shows what was trained."""
    if filter_3d is not None:
        from . import filter3d
        n = int(num_points)
        scales, opacities = filter3d.apply_filter_3d(params["scales"].reshape(-1, 3)[:n], params["opacities"].reshape(-1)[:n], filter_3d)
        params = {**params, "scales": scales, "opacities": opacities}
    v = vertex_records(params, num_points, colors)
    d = os.path.dirname(str(filepath))
    if d:
        os.makedirs(d, exist_ok=True)
    with open(filepath, "wb") as f:
        f.write(ply_header(len(v)))
        v.tofile(f)


def load_ply(filepath):
    """Read a file written by save_ply (or by the reference) back into the trainer's five arrays (+ the uchar colours)."""
    with open(filepath, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        n, fields, fmt = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                if tok[1] != "vertex" or n is not None:
                    raise ValueError("only a single vertex element is supported")
                n = int(tok[2])
            elif tok[0] == "property":
                fields.append((tok[2], {"float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1"}[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian" or n is None:
            raise ValueError("expected a binary_little_endian PLY with a vertex element")
        v = np.fromfile(f, dtype=np.dtype(fields), count=n)
    if len(v) != n:
        raise ValueError("PLY file is truncated")
    shs = np.zeros((n, 16, 3), dtype=np.float32)
    for c in range(3):
        shs[:, 0, c] = v[f"f_dc_{c}"]
    for i in range(45):
        shs[:, 1 + i // 3, i % 3] = v[f"f_rest_{i}"]
    return {"positions": np.stack([v["x"], v["y"], v["z"]], axis=1), "scales": np.stack([v["scale_0"], v["scale_1"], v["scale_2"]], axis=1),
            "rotations": np.stack([v["rot_x"], v["rot_y"], v["rot_z"], v["rot_w"]], axis=1), "opacities": np.array(v["opacity"]),
            "shs": shs.reshape(n * 16, 3), "colors": np.stack([v["red"], v["green"], v["blue"]], axis=1)}


SH_C0 = 0.28209479177387814
_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
                "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def load_points(filepath):
    """A binary little-endian PLY point cloud: (xyz float32 (N, 3), rgb float32 (N, 3) in [0, 1] or None).  The vertex element needs
    x, y, z; uchar red, green, blue are the colours when all three are there; every other scalar property is skipped by its declared
    size.  Elements behind the vertices (faces) are not read.  ASCII files, list properties in the vertex element and truncated
    files are refused with ValueError."""
    with open(filepath, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        n, fields, fmt, element = None, [], None, None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                element = tok[1]
                if element == "vertex":
                    if n is not None or fields:
                        raise ValueError("the vertex element must be the first element of the file, once")
                    n = int(tok[2])
                elif n is None:
                    raise ValueError("the vertex element must be the first element of the file, once")
            elif tok[0] == "property" and element == "vertex":
                if tok[1] == "list" or tok[1] not in _PLY_SCALARS:
                    raise ValueError(f"vertex property {tok[-1]!r}: only scalar properties are supported (got {tok[1]!r})")
                fields.append((tok[2], _PLY_SCALARS[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError(f"expected a binary_little_endian PLY (got {fmt!r}): convert ASCII or big-endian files first")
        names = [k for k, _ in fields]
        if n is None or len(set(names)) != len(names) or not all(k in names for k in "xyz"):
            raise ValueError("expected a vertex element with properties x, y, z")
        v = np.fromfile(f, dtype=np.dtype(fields), count=n)
    if len(v) != n:
        raise ValueError("PLY file is truncated")
    xyz = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32)
    rgb = None
    if all(k in names and v.dtype[k] == np.uint8 for k in ("red", "green", "blue")):
        rgb = np.stack([v["red"], v["green"], v["blue"]], axis=1).astype(np.float32) / np.float32(255)
    return xyz, rgb


def check_points(xyz, rgb=None, opacity=0.1):
    """The arguments of gaussians_from_points, refused with ValueError before the library or the device is touched: xyz (N, 3) with
    N >= 1 and finite, rgb None or (N, 3), opacity in (0, 1).  Returns them as float32 host arrays."""
    if hasattr(xyz, "detach"):
        xyz = xyz.detach().cpu().numpy()
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f"xyz must have shape (N, 3) with N >= 1 (got {xyz.shape})")
    xyz = np.ascontiguousarray(xyz, np.float32)
    if not np.isfinite(xyz).all():
        raise ValueError("xyz must be finite")
    if rgb is not None:
        if hasattr(rgb, "detach"):
            rgb = rgb.detach().cpu().numpy()
        rgb = np.asarray(rgb)
        if rgb.shape != xyz.shape:
            raise ValueError(f"rgb must have shape {xyz.shape}, one colour per point (got {rgb.shape})")
        rgb = np.ascontiguousarray(rgb, np.float32)
    opacity = float(opacity)
    if not 0.0 < opacity < 1.0:
        raise ValueError(f"opacity must be in (0, 1) (got {opacity})")
    return xyz, rgb, opacity


def gaussians_from_points(xyz, rgb=None, opacity=0.1, device="cuda"):
    """The trainer's five-array `params` dict for Gaussians at the points `xyz` (N, 3): scales from the three nearest neighbours
    (knn.init_scales), rotations as densify.init_gaussian_params stores them, `opacity` everywhere, SH DC = (rgb - 0.5) / C0 (0
    without colours), zeros above DC."""
    import torch
    from . import densify, knn
    xyz, rgb, opacity = check_points(xyz, rgb, opacity)
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    n = xyz.shape[0]
    P = densify.alloc_params(n, dev)
    P["positions"].copy_(torch.from_numpy(xyz))
    P["scales"].copy_(knn.init_scales(P["positions"]))
    P["rotations"][:, 0] = 1.0                                  # (1, 0, 0, 0) as stored, as gsr_init_gaussians leaves it
    P["opacities"].fill_(opacity)
    if rgb is not None:
        P["shs"].view(n, 16, 3)[:, 0, :] = torch.from_numpy((rgb - np.float32(0.5)) / np.float32(SH_C0)).to(dev)
    return P


def save_mesh_ply(path, verts, faces, colors=None):
    """An indexed triangle mesh (tsdf.weld's) as a binary little-endian PLY: `element vertex` with x y z (and uchar red green blue from
    `colors` in [0, 1], when given), `element face` with `property list uchar int vertex_indices`: what MeshLab, Blender and Open3D
    read."""
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.float32)).reshape(-1, 3)
    f = np.ascontiguousarray(np.asarray(faces)).reshape(-1, 3)
    if f.dtype.kind not in "iu" or (len(f) and (f.min() < 0 or f.max() >= len(v))):
        raise ValueError("save_mesh_ply: faces must be integer indices into verts")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colors is not None:
        c = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"save_mesh_ply: colors must hold one row per vertex, not {len(c)} for {len(v)}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vr = np.zeros(len(v), dtype=np.dtype(fields))
    vr["x"], vr["y"], vr["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        rgb = np.clip(np.nan_to_num(c) * np.float32(255), np.float32(0), np.float32(255)).astype(np.int64)
        vr["red"], vr["green"], vr["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    fr = np.zeros(len(f), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    fr["n"], fr["i"] = 3, f
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vr)}"]
    lines += [f"property {_PLY_TYPE[t.lstrip('<')]} {name}" for name, t in fields]
    lines += [f"element face {len(fr)}", "property list uchar int vertex_indices", "end_header"]
    d = os.path.dirname(str(path))
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as out:
        out.write(("\n".join(lines) + "\n").encode("ascii"))
        vr.tofile(out)
        fr.tofile(out)


def load_mesh_ply(filepath):
    """The inverse of save_mesh_ply for binary little-endian files: (verts float32 (V, 3), faces int32 (T, 3), colors float32 (V, 3) in
    [0, 1] or None).  The vertex element comes first and is read as load_points reads it; the face element follows it directly with
    one property, `list uchar int` (or uint8 / int32), and every face a triangle.  Anything else -- ASCII, another element between the
    two, another list type, a polygon, an index outside the vertices, a truncated file -- is refused with ValueError."""
    with open(filepath, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, elements = None, []                               # (name, count, [property tokens])
        while True:
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if not elements:
                    raise ValueError("a property in front of the first element")
                elements[-1][2].append(tok[1:])
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError(f"expected a binary_little_endian PLY (got {fmt!r}): convert ASCII or big-endian files first")
        if len(elements) < 2 or elements[0][0] != "vertex" or elements[1][0] != "face":
            raise ValueError("expected a vertex element followed by a face element")
        fields = []
        for p in elements[0][2]:
            if p[0] == "list" or p[0] not in _PLY_SCALARS:
                raise ValueError(f"vertex property {p[-1]!r}: only scalar properties are supported (got {p[0]!r})")
            fields.append((p[1], _PLY_SCALARS[p[0]]))
        names = [k for k, _ in fields]
        if len(set(names)) != len(names) or not all(k in names for k in "xyz"):
            raise ValueError("expected a vertex element with properties x, y, z")
        props = elements[1][2]
        if len(props) != 1 or len(props[0]) != 4 or props[0][0] != "list" or props[0][1] not in ("uchar", "uint8") or props[0][2] not in ("int", "int32"):
            raise ValueError("the face element must have one property, `list uchar int`")
        n, t = elements[0][1], elements[1][1]
        v = np.fromfile(f, dtype=np.dtype(fields), count=n)
        fr = np.fromfile(f, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=t)
    if len(v) != n or len(fr) != t:
        raise ValueError("PLY file is truncated")
    if t and (fr["n"] != 3).any():
        raise ValueError("every face must be a triangle")
    faces = np.ascontiguousarray(fr["i"]).astype(np.int32).reshape(-1, 3)
    if t and (faces.min() < 0 or faces.max() >= n):
        raise ValueError("a face index lies outside the vertices")
    verts = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32).reshape(-1, 3)
    colors = None
    if all(k in names and v.dtype[k] == np.uint8 for k in ("red", "green", "blue")):
        colors = np.stack([v["red"], v["green"], v["blue"]], axis=1).astype(np.float32) / np.float32(255)
    return verts, faces, colors
