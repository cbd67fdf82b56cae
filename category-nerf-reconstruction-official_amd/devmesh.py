"""The one door for a triangle mesh into the package ("The device mesh"): ``device_mesh`` turns a ``vis.Mesh``, a tuple of arrays or
tensors, or a triangle soup into a ``DeviceMesh``, and every module that hands a mesh to a kernel takes it from here.

A ``DeviceMesh`` that exists has passed the checks it was asked to pass: fp32 positions (V,3) rounded once, int32 faces (F,3)
whose indices were range-checked at their ORIGINAL integer width -- in numpy when they were held in host memory, by
``check_faces`` (an int64 min / max, then cnr_mesh_check_faces) when they were held in device memory, which never downloads
them.  The kernels trust the indices after that.  Every refusal is a ValueError that begins with the caller's ``what``."""
import numpy as np
import torch

from . import _C

__all__ = ["DeviceMesh", "device_mesh", "check_faces", "require_finite"]

INDEX_LIMIT = 2 ** 31 - 1
DEFAULT_COLOR = 102.0 / 255.0           # vis.Mesh's default grey


class DeviceMesh:
    """verts (V,3) f32 contiguous; faces (F,3) i32 contiguous, or None for a soup whose verts is (3F,3); n_faces; colors,
    normals (V,3) f32, or None when not asked for; device.  Built by ``device_mesh``, or around tensors that are valid already: what a kernel
    has just emitted (metrics._clip's soup), faces that ``check_faces`` returned (meshops.deviation)."""
    __slots__ = ("verts", "faces", "n_faces", "colors", "normals")

    def __init__(self, verts, faces, colors=None, normals=None):
        self.verts, self.faces, self.colors, self.normals = verts, faces, colors, normals
        self.n_faces = len(verts) // 3 if faces is None else len(faces)

    @property
    def device(self):
        return self.verts.device


def require_finite(tensor, what):
    """ValueError when a device tensor holds an inf or a NaN (one reduction, one host read)"""
    if not bool(torch.isfinite(tensor).all()):
        raise ValueError(f"{what}: non-finite coordinates")


def check_faces(faces, n_vertices, what):
    """(F,3) device faces -> contiguous int32, range-checked on the device against [0, n_vertices)"""
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must have the shape (F,3), not {tuple(faces.shape)}")
    if not faces.is_cuda:
        raise _C.CnrError(f"{what}: cnr kernels take device tensors only; there is no CPU path")
    n_vertices = int(n_vertices)
    F = faces.shape[0]
    if n_vertices < 0 or n_vertices > INDEX_LIMIT or 3 * F > INDEX_LIMIT:
        raise ValueError(f"{what}: V and 3 F must stay below 2^31")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be int32 or int64")
    if faces.dtype == torch.int64 and F:
        lo, hi = (int(v) for v in torch.stack([faces.min(), faces.max()]).cpu())
        if lo < 0 or hi >= n_vertices:
            raise ValueError(f"{what}: an index lies outside its range")
    f = faces.to(torch.int32).contiguous()
    if F:
        if n_vertices < 1:
            raise ValueError(f"{what}: an index lies outside its range")
        err = torch.zeros(1, device=f.device, dtype=torch.int32)
        _C.call("cnr_mesh_check_faces", f, F, n_vertices, err)
        if int(err.item()):
            raise ValueError(f"{what}: an index lies outside its range")
    return f


def _rows(a, what, name):
    """(n,3) of a numpy array or a tensor; a zero-size array of any shape counts as (0,3)"""
    if a.ndim == 2 and a.shape[1] == 3:
        return a
    if (a.numel() if torch.is_tensor(a) else a.size) == 0:
        return a.reshape(0, 3)
    raise ValueError(f"{what}: {name} must have the shape (n,3), not {tuple(a.shape)}")


def _f32(a, dev):
    """-> contiguous f32 on dev: a host array is rounded in numpy and uploaded, a tensor is converted where it lives"""
    if torch.is_tensor(a):
        return a.detach().to(device=dev, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _faces(f, V, dev, check, what):
    if torch.is_tensor(f) and f.is_cuda:
        f = _rows(f.detach(), what, "faces")
        if f.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: faces must be int32 or int64, not {f.dtype}")
        return (check_faces(f, V, what) if check else f.to(torch.int32).contiguous()).to(dev)
    f = _rows(f.detach().numpy() if torch.is_tensor(f) else np.asarray(f), what, "faces")
    if not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"{what}: faces must have an integer dtype, not {f.dtype}")
    if check and f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError(f"{what}: faces index vertices {f.min()} .. {f.max()} of a mesh with {V} vertices")
    return torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)


def device_mesh(mesh, device=None, check=True, attributes=False, what="mesh"):
    """``mesh`` -> DeviceMesh on ``device``.  ``mesh``: a DeviceMesh (returned as it is when it lives there already), a
    ``vis.Mesh`` or anything with vertices / faces, a tuple (verts, faces[, colors, normals]) of numpy arrays or tensors on any
    device (colours in [0,1]), or (soup_verts (3F,3), None).  device=None: the device of ``verts`` when that is a device
    tensor, the current CUDA device otherwise.  check=False skips the range check of the indices, nothing else.
    attributes=True adds colors and normals: a Mesh's ``visual.vertex_colors / 255`` and ``vertex_normals``, a tuple's third and
    fourth element, 102/255 and zeros where a tuple has none."""
    colors = normals = None
    if isinstance(mesh, DeviceMesh):
        if (device is None or _device(device) == mesh.device) and (mesh.colors is not None or not attributes):
            return mesh
        verts, faces, colors, normals = mesh.verts, mesh.faces, mesh.colors, mesh.normals
    elif hasattr(mesh, "vertices"):
        verts, faces = np.asarray(mesh.vertices), np.ascontiguousarray(mesh.faces)
        if attributes:
            colors = np.ascontiguousarray(mesh.visual.vertex_colors[:, :3], np.float32) / np.float32(255)
            normals = mesh.vertex_normals
    elif isinstance(mesh, (tuple, list)) and 2 <= len(mesh) <= 4:
        verts, faces = mesh[0], mesh[1]
        colors, normals = (mesh[2] if len(mesh) > 2 else None), (mesh[3] if len(mesh) > 3 else None)
    else:
        raise ValueError(f"{what}: a mesh is a DeviceMesh, a vis.Mesh, a tuple (verts, faces[, colors, normals]), or a (F*3,3) "
                         "soup with faces=None")
    dev = verts.device if device is None and torch.is_tensor(verts) and verts.is_cuda else _device(device)
    v = _f32(_rows(verts if torch.is_tensor(verts) else np.asarray(verts), what, "verts"), dev)
    if len(v) > INDEX_LIMIT or (faces is not None and len(faces) > INDEX_LIMIT):
        raise ValueError(f"{what}: V and F must stay below 2^31")
    if faces is None:
        if len(v) % 3:
            raise ValueError(f"{what}: a triangle soup has 3 vertices per face, not {len(v)} in all")
    else:
        faces = _faces(faces, len(v), dev, check, what)
    if not attributes:
        return DeviceMesh(v, faces)
    c = torch.full_like(v, DEFAULT_COLOR) if colors is None else _f32(colors, dev)
    n = torch.zeros_like(v) if normals is None else _f32(normals, dev)
    if c.shape != v.shape or n.shape != v.shape:
        raise ValueError(f"{what}: colors and normals must have the shape of verts {tuple(v.shape)}, not {tuple(c.shape)} and "
                         f"{tuple(n.shape)}")
    return DeviceMesh(v, faces, c, n)


def _device(device):
    """torch.device of a caller's ``device`` argument: None and a bare "cuda" name the current CUDA device"""
    dev = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev
