"""Isosurface extraction with the reference's name and call (src/vis.py:6-20): ``marching_cubes(occupancy, level=0.5)`` ->
a mesh with vertices in [0, 1]^3 (index space / (D - 1)), or None when no edge crosses the level (the reference's
``except (RuntimeError, ValueError): return None``).

The extraction runs on the GPU (csrc/mcubes.hip: cnr_mc_count + cnr_mc_emit).  ``Mesh`` is a small host-side
stand-in for the parts of trimesh that Trainer.meshing and train.py use (trimesh is not a dependency).

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


def marching_cubes_raw(volume, level=0.5, ascent=True):
    """volume (D,D,D) fp32 device tensor -> (verts (V,3) f32, normals (V,3) f32, faces (F,3) i32) device tensors, or None"""
    D = volume.shape[0]
    if volume.dim() != 3 or tuple(volume.shape) != (D, D, D):
        raise ValueError(f"marching_cubes wants a (D,D,D) volume, got {tuple(volume.shape)}")
    vol = volume.float().contiguous()
    nbytes = int(_C.load().cnr_mc_workspace_bytes(int(D)))
    if nbytes < 0:
        raise _C.CnrError(f"marching_cubes: D = {D} outside [2, 512]")
    ws = torch.empty(nbytes, device=vol.device, dtype=torch.uint8)
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
