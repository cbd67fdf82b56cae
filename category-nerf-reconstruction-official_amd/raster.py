"""Mesh rasterisation: a triangle mesh seen from a pinhole camera -- which pixel sees which face at what
z-depth (csrc/raster.hip: cnr_raster_bin_count / _bin_emit / _tiles), colour, instance and normal images from the winning
faces (cnr_raster_attributes), and which faces a set of poses ever sees (cnr_raster_visible).

``MeshScene`` holds one or several ``vis.Mesh`` on the device, ``MeshRasterizer`` the camera (W, H, intrinsics, depth limits,
the ``cameraInfo`` ray table, exactly as ``view.SceneRenderer``).  ``render`` returns the keys and the (W,H,...) layout of
``SceneRenderer.render``, so ``view.render_to_files`` and ``view.shade`` take a single-view result as it is.

Coverage is decided in fp64 in the camera frame without projecting or clipping anything (the header has the formulas), the
nearest face wins a pixel and the lower face index wins among equal depths: the images do not depend on how the poses are split
into launches and are bit-identical from run to run.  tests/raster_cpu.py restates all of it in numpy."""
import numpy as np
import torch

from . import _C
from .devmesh import DeviceMesh, device_mesh
from .vis import Mesh

# the workspace of one launch (80 bytes of coefficients and 8 of tile box per view and face, 16 per view and tile) stays
# under this many bytes: render and visible_faces split their poses accordingly (one view per launch always goes)
WORKSPACE_BOUND = 1 << 30
MAX_PAIRS = 2 ** 31 - 1


class MeshScene:
    """``MeshScene(meshes, labels=None)``: the meshes of a list (each a ``vis.Mesh``, a ``devmesh.DeviceMesh`` or a tuple
    ``(verts, faces[, colors, normals])`` of arrays or tensors, colours in [0,1]; a single mesh may come without the list)
    concatenated on the device: ``verts (Nv,3) f32``, ``faces (F,3) i32``, ``colors (Nv,3) f32`` (``visual.vertex_colors /
    255``), ``normals (Nv,3) f32``, ``face_label (F,) i32`` = the instance id of the face's mesh (``labels``, default its place
    in the list) and ``face_mesh (F,) i32`` = that place.  ``face_offsets`` (host) delimits every mesh's faces.  Face indices
    are checked by ``devmesh.device_mesh`` where they are held (host arrays before they are uploaded, device tensors on the
    device): the kernels trust them."""

    def __init__(self, meshes, labels=None, device=None):
        if isinstance(meshes, (Mesh, DeviceMesh)) or (isinstance(meshes, tuple) and len(meshes)
                                                      and not isinstance(meshes[0], (Mesh, DeviceMesh, tuple, list))):
            meshes = [meshes]
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        parts = [device_mesh(m, dev, attributes=True) for m in meshes]
        if not parts:
            raise ValueError("no mesh")
        if any(p.faces is None for p in parts):
            raise ValueError("a scene takes meshes with faces, not a triangle soup")
        labels = list(range(len(parts))) if labels is None else [int(x) for x in labels]
        if len(labels) != len(parts):
            raise ValueError("{} labels for {} meshes".format(len(labels), len(parts)))
        voff = np.cumsum([0] + [len(p.verts) for p in parts])
        self.face_offsets = [int(x) for x in np.cumsum([0] + [p.n_faces for p in parts])]
        if voff[-1] >= 2 ** 31 or self.face_offsets[-1] >= 2 ** 31:
            raise ValueError("more than 2^31 - 1 vertices or faces")
        if self.face_offsets[-1] == 0:
            raise ValueError("the meshes have no face")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.device = dev
        self.verts = torch.cat([p.verts for p in parts])
        self.faces = torch.cat([p.faces + int(o) for p, o in zip(parts, voff)])
        self.colors = torch.cat([p.colors for p in parts])
        self.normals = torch.cat([p.normals for p in parts])
        self.face_label = up(np.concatenate([np.full(p.n_faces, l, np.int32) for p, l in zip(parts, labels)]))
        self.face_mesh = up(np.concatenate([np.full(p.n_faces, i, np.int32) for i, p in enumerate(parts)]))
        self.n_faces, self.n_meshes = self.face_offsets[-1], len(parts)


def _poses(T_wc):
    """(4,4) or (V,4,4) -> ((V,4,4) float64 numpy, single)"""
    T = np.asarray(T_wc.detach().cpu() if torch.is_tensor(T_wc) else T_wc, np.float64)
    if T.shape == (4, 4):
        return T[None], True
    if T.ndim != 3 or T.shape[1:] != (4, 4) or T.shape[0] < 1:
        raise ValueError("T_wc must have the shape (4,4) or (V,4,4), not {}".format(T.shape))
    return T, False


class MeshRasterizer:
    """``MeshRasterizer(cfg)``: W, H, fx, fy, cx, cy, ``min_depth``, ``max_depth`` and the device from the config, the rays from
    ``cameraInfo(cfg)``, as ``view.SceneRenderer``.  ``from_intrinsics`` serves mesh tools that have no config."""

    def __init__(self, cfg):
        self.device = torch.device(cfg.training_device)
        self.W, self.H = int(cfg.W), int(cfg.H)
        self.fx, self.fy, self.cx, self.cy = float(cfg.fx), float(cfg.fy), float(cfg.cx), float(cfg.cy)
        self.zmin, self.zmax = float(cfg.min_depth), float(cfg.max_depth)
        if not (self.zmin >= 0.0 and self.zmax >= self.zmin):
            raise ValueError("the depth limits must satisfy 0 <= min_depth <= max_depth, not {} and {}".format(self.zmin, self.zmax))
        if not (1 <= self.W <= 32768 and 1 <= self.H <= 32768):
            raise ValueError("W and H must lie in 1 .. 32768")
        self._dirs = None
        self.stage_events = None       # a list: the launches append (stage name, device event) (tools/time_raster.py)

    @classmethod
    def from_intrinsics(cls, W, H, fx, fy, cx, cy, zmin, zmax, device=None):
        from types import SimpleNamespace
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        return cls(SimpleNamespace(W=W, H=H, fx=fx, fy=fy, cx=cx, cy=cy, min_depth=zmin, max_depth=zmax, training_device=str(dev)))

    def dirs(self):
        """the cameraInfo cache rows (W*H, 3), pixel w * H + h"""
        if self._dirs is None:
            from .scene_cateogries import cameraInfo
            from types import SimpleNamespace
            cam = SimpleNamespace(W=self.W, H=self.H, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy)
            self._dirs = cameraInfo(cam, device=self.device).rays_dir_cache.reshape(-1, 3).contiguous()
        return self._dirs

    def _mark(self, name):
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    def views_per_launch(self, scene, want=None):
        """the poses one launch takes: ``want``, or as many as keep the workspace under WORKSPACE_BOUND (at least one)"""
        if want is not None:
            if isinstance(want, bool) or int(want) != want or want < 1:
                raise ValueError("views_per_launch must be a positive integer")
            return int(want)
        one = int(_C.load().cnr_raster_workspace_bytes(scene.n_faces, 1, self.W, self.H))
        if one < 0:
            raise _C.CnrError("cnr_raster_workspace_bytes failed with {}".format(one))
        return max(1, WORKSPACE_BOUND // one)

    def _rasterize(self, scene, T_cw, cull):
        """one launch chain over the poses T_cw (V,4,4) float64 numpy -> (workspace, T_cw on the device, depth, face, bary)"""
        dev, V, F, W, H = self.device, T_cw.shape[0], scene.n_faces, self.W, self.H
        if scene.device != dev:
            raise ValueError("the scene lives on {}, the rasteriser on {}".format(scene.device, dev))
        ws = _C.workspace(_C.load().cnr_raster_workspace_bytes(F, V, W, H), dev, "cnr_raster ({} faces, {} views of {} x {})".format(F, V, W, H))
        T = torch.from_numpy(np.ascontiguousarray(T_cw, np.float64)).to(dev)
        n_pairs = torch.empty(1, device=dev, dtype=torch.int64)
        self._mark("start")
        _C.call("cnr_raster_bin_count", scene.verts, scene.faces, F, T, V, W, H, self.fx, self.fy, self.cx, self.cy, self.zmin,
                1 if cull else 0, ws, n_pairs)
        N = int(n_pairs.item())
        self._mark("setup + count")
        if N > MAX_PAIRS:
            raise ValueError("{} (view, tile, face) pairs in one launch, more than 2^31 - 1: use fewer views per launch".format(N))
        pair_face = torch.empty(max(N, 1), device=dev, dtype=torch.int32)
        _C.call("cnr_raster_bin_emit", F, V, W, H, ws, pair_face)
        self._mark("emit")
        depth = torch.empty(V, W, H, device=dev)
        face = torch.empty(V, W, H, device=dev, dtype=torch.int32)
        bary = torch.empty(V, W, H, 2, device=dev)
        _C.call("cnr_raster_tiles", self.dirs(), F, V, W, H, self.zmin, self.zmax, ws, pair_face, depth, face, bary)
        self._mark("tiles")
        self.pairs = N                 # of the last launch
        return ws, T, depth, face, bary

    def render(self, scene, T_wc, attributes=True, normal="face", cull_backfaces=False, views_per_launch=None):
        """-> {depth (W,H) f32 z-depth (0: nothing hit), face (W,H) i32 index into ``scene.faces`` (-1: nothing hit), bary
        (W,H,2) f32 = the winner's b1, b2 (b0 = 1 - b1 - b2), opacity (W,H) f32 (1 where hit)} and with ``attributes`` also
        {rgb (W,H,3) f32 interpolated vertex colours, instance (W,H) i32 = ``scene.face_label`` of the winner (-1: nothing
        hit), normal (W,H,3) f32 world-frame unit vector}; with ``T_wc`` (V,4,4) every image gains a leading V.

        ``normal="face"``: the geometric normal of the winning face turned towards the camera (n . d_world < 0), the sign
        ``view.shade`` expects, whatever the winding.  ``normal="vertex"``: the normalised interpolation of ``scene.normals``
        with its sign as given.  Zero where nothing was hit or the vector vanishes.

        Faces are two-sided.  ``cull_backfaces=True`` keeps the faces whose corners run CLOCKWISE in the image as it is
        displayed (x right, y down), det = v0 . (v1 x v2) > 0 in the camera frame: faces whose right-hand normal points AWAY
        from the camera.  ``vis.marching_cubes``'s 'ascent' meshes point their right-hand normals into the object, so this keeps
        the outside of an 'ascent' mesh (and the inside of a 'descent' one).

        The poses go through in launches of ``views_per_launch`` (default: what keeps the workspace under WORKSPACE_BOUND);
        the result does not depend on it."""
        T, single = _poses(T_wc)
        if normal not in ("face", "vertex"):
            raise ValueError("normal must be 'face' or 'vertex', not {!r}".format(normal))
        T_cw = np.linalg.inv(T)
        V, W, H, dev = T.shape[0], self.W, self.H, self.device
        step = self.views_per_launch(scene, views_per_launch)
        out = dict(depth=torch.empty(V, W, H, device=dev), face=torch.empty(V, W, H, device=dev, dtype=torch.int32),
                   bary=torch.empty(V, W, H, 2, device=dev))
        if attributes:
            out.update(rgb=torch.empty(V, W, H, 3, device=dev), instance=torch.empty(V, W, H, device=dev, dtype=torch.int32),
                       normal=torch.empty(V, W, H, 3, device=dev))
        with torch.no_grad(), torch.cuda.device(dev):
            for a in range(0, V, step):
                b = min(a + step, V)
                ws, Tdev, depth, face, bary = self._rasterize(scene, T_cw[a:b], cull_backfaces)
                out["depth"][a:b], out["face"][a:b], out["bary"][a:b] = depth, face, bary
                if attributes:
                    _C.call("cnr_raster_attributes", self.dirs(), scene.verts, scene.faces, scene.colors, scene.normals,
                            scene.face_label, Tdev, scene.n_faces, b - a, W, H, 1 if normal == "vertex" else 0, ws, face,
                            out["rgb"][a:b], out["instance"][a:b], out["normal"][a:b])
                    self._mark("attributes")
        out["opacity"] = (out["face"] >= 0).float()
        return {k: v[0] for k, v in out.items()} if single else out

    def visible_faces(self, scene, T_wcs, depth_obs=None, tol=0.0, views_per_launch=None):
        """-> (seen bool (F,), count int32 (F,)): whether, and in how many of the poses ``T_wcs`` (V,4,4), a face wins at
        least one pixel.  With ``depth_obs`` (V,W,H), the frames' own depth images in this project's (W,H) layout, a winning
        pixel counts only where ``depth_obs > 0`` and the face's depth <= ``depth_obs + tol``: a surface hidden behind real
        geometry is not seen."""
        T, _ = _poses(T_wcs)
        T_cw = np.linalg.inv(T)
        V, F, dev = T.shape[0], scene.n_faces, self.device
        if depth_obs is not None:
            depth_obs = torch.as_tensor(depth_obs, dtype=torch.float32)
            if tuple(depth_obs.shape) != (V, self.W, self.H):
                raise ValueError("depth_obs must have the shape {}, not {}".format((V, self.W, self.H), tuple(depth_obs.shape)))
        step = self.views_per_launch(scene, views_per_launch)
        seen, count = torch.zeros(F, device=dev, dtype=torch.uint8), torch.zeros(F, device=dev, dtype=torch.int32)
        with torch.no_grad(), torch.cuda.device(dev):
            for a in range(0, V, step):
                b = min(a + step, V)
                _, _, depth, face, _ = self._rasterize(scene, T_cw[a:b], False)
                obs = None if depth_obs is None else depth_obs[a:b].to(dev).contiguous()
                vws = _C.workspace(_C.load().cnr_raster_visible_workspace_bytes(F, b - a), dev, "cnr_raster_visible")
                _C.call("cnr_raster_visible", face, depth, obs, float(tol), F, b - a, self.W, self.H, vws, seen, count)
                self._mark("visible")
        return seen.bool(), count


def cull_mesh(mesh, keep_faces):
    """A new ``vis.Mesh`` with the faces ``keep_faces`` (a bool mask (F,) or an index array) of ``mesh``: the vertices they use
    in their old order, re-indexed, with their colours and normals."""
    keep = np.asarray(keep_faces.detach().cpu() if torch.is_tensor(keep_faces) else keep_faces)
    F = len(mesh.faces)
    if keep.dtype == np.bool_:
        if keep.shape != (F,):
            raise ValueError("a face mask must have the shape ({},), not {}".format(F, keep.shape))
        keep = np.nonzero(keep)[0]
    keep = keep.astype(np.int64).reshape(-1)
    if keep.size and (keep.min() < 0 or keep.max() >= F):
        raise ValueError("face indices must lie in 0 .. {}".format(F - 1))
    faces = mesh.faces[keep]
    used = np.unique(faces)
    remap = np.full(len(mesh.vertices), -1, np.int64)
    remap[used] = np.arange(len(used))
    return mesh.subset(used, remap[faces].reshape(-1, 3))


def observed_area(scene, seen):
    """per mesh of the scene (seen area, total area) in float64: the faces' areas summed over the faces with ``seen`` set"""
    seen = torch.as_tensor(seen).to(scene.device).bool()
    if tuple(seen.shape) != (scene.n_faces,):
        raise ValueError("seen must have the shape ({},), not {}".format(scene.n_faces, tuple(seen.shape)))
    p = scene.verts.double()[scene.faces.long()]
    area = 0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=-1)
    got = area * seen
    offs = scene.face_offsets
    return [(float(got[a:b].sum()), float(area[a:b].sum())) for a, b in zip(offs[:-1], offs[1:])]
