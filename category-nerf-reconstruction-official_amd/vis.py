"""Isosurface extraction with the reference's name and call (src/vis.py:6-20): ``marching_cubes(occupancy, level=0.5)`` ->
a mesh with vertices in [0, 1]^3 (index space / (D - 1)), or None when no edge crosses the level (the reference's
``except (RuntimeError, ValueError): return None``).

The extraction runs on the GPU (csrc/mcubes.hip: cnr_mc_count + cnr_mc_emit).  ``Mesh`` is a small host-side
stand-in for the parts of trimesh that Trainer.meshing and train.py use (trimesh is not a dependency); ``load_mesh`` reads the
.obj / .ply meshes that the evaluation (``metrics``, tools/eval_3d_obj.py) compares.

Orientation convention: with gradient_direction='ascent' (the reference's argument) every face's right-hand normal points
towards INCREASING values -- for an occupancy field, into the object -- and the vertex normals (the interpolated, normalised
index-space gradient) point to the same side; 'descent' gives the same faces with columns 1 and 2 swapped and negated
normals.  (skimage's own sign for 'ascent' was not available to check against.)"""
import numpy as np
import torch

from . import _C


class _Visual:
    def __init__(self, n):
        self._colors = np.tile(np.array([102, 102, 102, 255], np.uint8), (n, 1))

    @property
    def vertex_colors(self):
        return self._colors

    @vertex_colors.setter
    def vertex_colors(self, c):
        c = np.asarray(c)
        if c.ndim == 1:
            c = np.tile(c, (len(self._colors), 1))
        c = c.astype(np.uint8)
        if c.shape[1] == 3:
            c = np.concatenate([c, np.full((len(c), 1), 255, np.uint8)], 1)
        self._colors = np.ascontiguousarray(c)


class Mesh:
    """vertices (V,3) float64, faces (F,3) int64, vertex_normals (V,3) float64, visual.vertex_colors (V,4) uint8."""

    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = np.asarray(vertices, np.float64)
        self.faces = np.asarray(faces, np.int64)
        self.vertex_normals = (np.zeros_like(self.vertices) if vertex_normals is None
                               else np.asarray(vertex_normals, np.float64))
        self.visual = _Visual(len(self.vertices))

    @staticmethod
    def _unit(n):
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)

    def subset(self, vertex_index, faces):
        """a new Mesh of the vertices ``vertex_index`` in that order, with their normals and colours, and the given faces"""
        out = Mesh(self.vertices[vertex_index], faces, self.vertex_normals[vertex_index])
        out.visual.vertex_colors = self.visual.vertex_colors[vertex_index]
        return out

    def apply_translation(self, translation):
        self.vertices = self.vertices + np.asarray(translation, np.float64).reshape(1, 3)
        return self

    def apply_scale(self, scaling):
        s = np.asarray(scaling, np.float64)
        if s.ndim == 0:
            self.vertices = self.vertices * float(s)
            return self
        M = np.eye(4)
        M[:3, :3] = np.diag(s.reshape(3))
        return self.apply_transform(M)

    def apply_transform(self, matrix):
        """4x4 affine: vertices by M, normals by the inverse transpose of its 3x3 block (renormalised); faces are flipped when
        that block's determinant is negative (the winding then keeps pointing the normals the same way)."""
        M = np.asarray(matrix, np.float64).reshape(4, 4)
        A, t = M[:3, :3], M[:3, 3]
        self.vertices = self.vertices @ A.T + t
        self.vertex_normals = self._unit(self.vertex_normals @ np.linalg.inv(A))   # (A^-T n) as rows
        if np.linalg.det(A) < 0:
            self.faces = self.faces[:, ::-1].copy()
        return self

    def export(self, path):
        """Wavefront .obj: `v x y z r g b` (colours as floats in [0, 1]), `vn`, `f a//a b//b c//c` (1-based)."""
        if not str(path).endswith(".obj"):
            raise ValueError("Mesh.export writes .obj only")
        col = self.visual.vertex_colors[:, :3].astype(np.float64) / 255.0
        with open(path, "w") as f:
            for (x, y, z), (r, g, b) in zip(self.vertices, col):
                f.write("v %.8f %.8f %.8f %.6f %.6f %.6f\n" % (x, y, z, r, g, b))
            for x, y, z in self.vertex_normals:
                f.write("vn %.8f %.8f %.8f\n" % (x, y, z))
            for a, b, c in self.faces + 1:
                f.write("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c))
        return path


def load_obj(path):
    """-> (vertices (V,3) f64, colours (V,3) f64, normals (V,3) f64, faces (F,3) i64) of a file written by Mesh.export"""
    v, vn, fc = [], [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:7]])
            elif p[0] == "vn":
                vn.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                fc.append([int(x.split("//")[0]) - 1 for x in p[1:4]])
    v = np.array(v, np.float64).reshape(-1, 6)
    return v[:, :3], v[:, 3:], np.array(vn, np.float64).reshape(-1, 3), np.array(fc, np.int64).reshape(-1, 3)


def _fan(polys, counts):
    """polygons (flat index list + per-polygon vertex counts) -> (T,3) triangles fanned from each polygon's first vertex"""
    tris = []
    if len(counts) and (counts == counts[0]).all():
        k = int(counts[0])
        p = np.asarray(polys, np.int64).reshape(-1, k)
        if k < 3:
            return np.zeros((0, 3), np.int64)
        return np.stack([np.stack([p[:, 0], p[:, j], p[:, j + 1]], 1) for j in range(1, k - 1)], 1).reshape(-1, 3)
    pos = 0
    for k in counts:
        p = polys[pos:pos + k]
        pos += k
        tris.extend([p[0], p[j], p[j + 1]] for j in range(1, k - 1))
    return np.array(tris, np.int64).reshape(-1, 3)


def _load_obj_mesh(path):
    v, polys, counts = [], [], []
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                # `a`, `a/b`, `a//c`, `a/b/c`; 1-based, negative = relative to the vertices read so far
                idx = [int(x.split("/")[0]) for x in p[1:]]
                polys.extend(i - 1 if i > 0 else len(v) + i for i in idx)
                counts.append(len(idx))
    return np.array(v, np.float64).reshape(-1, 3), _fan(polys, np.array(counts, np.int64))


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _load_ply_mesh(path):
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: PLY header without end_header")
            p = line.decode("ascii", "replace").split()
            if not p or p[0] in ("comment", "obj_info"):
                continue
            if p[0] == "end_header":
                break
            if p[0] == "format":
                fmt = p[1]
            elif p[0] == "element":
                elements.append((p[1], int(p[2]), []))
            elif p[0] == "property":
                elements[-1][2].append(("list", p[2], p[3], p[4]) if p[1] == "list" else (p[1], p[2]))
        body = f.read()
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
    verts, polys, counts = np.zeros((0, 3)), [], np.zeros(0, np.int64)
    pos, tokens = 0, body.split() if fmt == "ascii" else None
    for name, n, props in elements:
        if fmt == "ascii":
            rows, nprop = [], len(props)
            if all(pr[0] != "list" for pr in props):
                rows = np.array(tokens[pos:pos + n * nprop], np.float64).reshape(n, nprop)
                pos += n * nprop
                if name == "vertex":
                    cols = [pr[1] for pr in props]
                    verts = rows[:, [cols.index("x"), cols.index("y"), cols.index("z")]]
                continue
            lst = []
            for _ in range(n):
                for pr in props:
                    if pr[0] == "list":
                        k = int(tokens[pos])
                        lst.append([int(t) for t in tokens[pos + 1:pos + 1 + k]])
                        pos += 1 + k
                    else:
                        pos += 1
            if name == "face":
                counts = np.array([len(x) for x in lst], np.int64)
                polys = [i for x in lst for i in x]
            continue
        # binary little endian: scalars through a structured dtype; a list property with the same length on every row too
        # (checked), other rows one by one
        if all(pr[0] != "list" for pr in props):
            dt = np.dtype([(pr[1], "<" + _PLY_TYPES[pr[0]]) for pr in props])
            arr = np.frombuffer(body, dt, n, pos)
            pos += n * dt.itemsize
            if name == "vertex":
                verts = np.stack([arr["x"], arr["y"], arr["z"]], 1).astype(np.float64)
            continue
        lists = [pr for pr in props if pr[0] == "list"]
        k0 = None
        if len(lists) == 1 and n > 0:
            off = sum(np.dtype(_PLY_TYPES[pr[0]]).itemsize for pr in props[:props.index(lists[0])])
            k0 = int(np.frombuffer(body, "<" + _PLY_TYPES[lists[0][1]], 1, pos + off)[0])
            dt = _ply_row_dtype(props, k0)
            if pos + n * dt.itemsize <= len(body):
                arr = np.frombuffer(body, dt, n, pos)
                if (arr["__n"] == k0).all():
                    pos += n * dt.itemsize
                    if name == "face":
                        polys = arr[lists[0][3]].astype(np.int64).reshape(-1)
                        counts = np.full(n, k0, np.int64)
                    continue
        lst = []
        for _ in range(n):
            for pr in props:
                if pr[0] == "list":
                    k = int(np.frombuffer(body, "<" + _PLY_TYPES[pr[1]], 1, pos)[0])
                    pos += np.dtype(_PLY_TYPES[pr[1]]).itemsize
                    it = np.dtype("<" + _PLY_TYPES[pr[2]])
                    lst.append(np.frombuffer(body, it, k, pos).astype(np.int64))
                    pos += k * it.itemsize
                else:
                    pos += np.dtype(_PLY_TYPES[pr[0]]).itemsize
        if name == "face":
            counts = np.array([len(x) for x in lst], np.int64)
            polys = np.concatenate(lst) if lst else np.zeros(0, np.int64)
    return np.asarray(verts, np.float64).reshape(-1, 3), _fan(np.asarray(polys, np.int64), counts)


def _ply_row_dtype(props, k):
    """one row of an element whose single list property holds k items: the count field is named __n"""
    fields = []
    for pr in props:
        if pr[0] == "list":
            fields += [("__n", "<" + _PLY_TYPES[pr[1]]), (pr[3], "<" + _PLY_TYPES[pr[2]], (k,))]
        else:
            fields.append((pr[1], "<" + _PLY_TYPES[pr[0]]))
    return np.dtype(fields)


def load_mesh(path):
    """A triangle Mesh from `.obj` (any face syntax: a, a/b, a//c, a/b/c; negative indices) or `.ply` (ascii or
    binary_little_endian; x/y/z from whatever vertex properties there are; face lists with any integer count and index type).
    Polygons are fan-triangulated from their first vertex.  Normals and colours are not read (zeros / the default grey)."""
    p = str(path)
    ext = p.rsplit(".", 1)[-1].lower()
    if ext == "obj":
        v, f = _load_obj_mesh(p)
    elif ext == "ply":
        v, f = _load_ply_mesh(p)
    else:
        raise ValueError(f"load_mesh reads .obj and .ply, got {p}")
    return Mesh(v, f)


def marching_cubes_raw(volume, level=0.5, ascent=True):
    """volume (D,D,D) fp32 device tensor -> (verts (V,3) f32, normals (V,3) f32, faces (F,3) i32) device tensors, or None"""
    D = volume.shape[0]
    if volume.dim() != 3 or tuple(volume.shape) != (D, D, D):
        raise ValueError(f"marching_cubes wants a (D,D,D) volume, got {tuple(volume.shape)}")
    vol = volume.float().contiguous()
    ws = _C.workspace(_C.load().cnr_mc_workspace_bytes(int(D)), vol.device, f"marching_cubes (D = {D}, which must lie in [2, 512])")
    counts = torch.empty(2, device=vol.device, dtype=torch.int64)
    _C.call("cnr_mc_count", vol, int(D), float(level), ws, counts)
    V, F = (int(x) for x in counts.cpu())
    if V == 0 or F == 0:
        return None
    verts = torch.empty(V, 3, device=vol.device, dtype=torch.float32)
    normals = torch.empty(V, 3, device=vol.device, dtype=torch.float32)
    faces = torch.empty(F, 3, device=vol.device, dtype=torch.int32)
    _C.call("cnr_mc_emit", vol, int(D), float(level), 1 if ascent else 0, ws, verts, normals, faces)
    return verts, normals, faces


def marching_cubes(occupancy, level=0.5, gradient_direction="ascent"):
    """src/vis.py:6-20 on the GPU: occupancy (D,D,D), a device tensor or a numpy array (moved to the current device)."""
    if gradient_direction not in ("ascent", "descent"):
        raise ValueError(f"gradient_direction must be 'ascent' or 'descent', got {gradient_direction!r}")
    vol = occupancy if torch.is_tensor(occupancy) else torch.from_numpy(np.ascontiguousarray(occupancy, np.float32))
    if not vol.is_cuda:
        vol = vol.to(torch.device("cuda", torch.cuda.current_device()))
    out = marching_cubes_raw(vol, level, gradient_direction == "ascent")
    if out is None:
        return None
    verts, normals, faces = (t.cpu().numpy() for t in out)
    return Mesh(verts, faces, normals)
