"""Mesh evaluation with the reference's names and arguments (metric/metrics.py, metric/eval_3D_obj.py:10-39), on the GPU.

``accuracy`` / ``completion`` / ``accuracy_ratio`` / ``completion_ratio`` / ``chamfer`` take point sets (numpy arrays or
tensors, (n,3)) and return Python floats; the exact nearest-neighbour search (the reference's cKDTree query) is
``cnr_nn_dist`` (csrc/metric.hip), fp32 distances of fp32 points, their mean in fp64.  ``calc_3d_metric`` is
the reference's per-object score: the oriented box of ``mesh_ref``, the reconstruction clipped to it, three area-weighted
samples, accuracy / completion in cm and the completion ratio at 5 cm in %; the samples stay on the device.
``point_mesh_distance`` is the exact distance from points to a triangle mesh with the closest face (``cnr_point_mesh_dist``,
csrc/point_mesh.hip), and ``calc_3d_metric_surface`` the same score with every distance taken to the other
mesh instead of to samples of it, plus precision / recall / F-score and normal consistency.  ``MeshIndex`` (opt-in,
csrc/point_mesh_index.hip) answers the same queries bit for bit through a tile-box index that skips most of the mesh.
``winding_number`` is the generalized winding number of a mesh about arbitrary points (``cnr_winding_number``,
csrc/winding.hip), on which ``inside``, ``signed_distance`` and ``volume_iou`` rest; ``mesh_orientation``
tells whether a mesh's normals point outward.  The reference has none of these.

Differences from the reference, all deliberate:
* the ground truth is an argument (``mesh_gt``, default ``mesh_ref``); the reference reads a module-level ``mesh_gt`` and uses
  ``mesh_ref`` for the box only, which is the same whenever no ``--log_dir_ref`` mesh exists;
* the samples come from ``numpy.random.default_rng(seed)`` (three (N,3) uniform draws: reconstruction, clipped
  reconstruction, ground truth), so a score is reproducible; trimesh draws from numpy's global state;
* the ratios are float64 (the reference's ``np.float`` is gone from numpy >= 1.24); distances compare with ``<``.
"""
import numpy as np
import torch

from . import _C
from .devmesh import DeviceMesh, device_mesh, require_finite

__all__ = ["accuracy", "completion", "accuracy_ratio", "completion_ratio", "chamfer", "nn_dist", "dist_stats",
           "sample_surface", "oriented_bounds", "box_planes", "slice_box", "calc_3d_metric", "depth_l1", "depth_l1_images",
           "point_mesh_distance", "sample_surface_faces", "calc_3d_metric_surface", "MeshIndex", "winding_number",
           "mesh_orientation", "inside", "signed_distance", "volume_iou"]


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _points(x, dev=None):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
    if dev is None:
        dev = t.device if t.is_cuda else _device()
    t = t.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    if len(t) == 0:
        raise ValueError("empty point set")
    return t


# ---- distances ---------------------------------------------------------------------------------------------------------
def nn_dist(query, ref):
    """-> (nq,) f32 device tensor: the distance of every query point to the nearest reference point (exact, cnr_nn_dist)"""
    q = _points(query)
    p = _points(ref, q.device)
    ws = _C.workspace(_C.load().cnr_nn_workspace_bytes(len(q), len(p)), q.device, "cnr_nn_dist")
    out = torch.empty(len(q), device=q.device, dtype=torch.float32)
    _C.call("cnr_nn_dist", q, len(q), p, len(p), out, ws)
    return out


def _stats_device(dist, th):
    d = dist.contiguous()
    ws = _C.workspace(_C.load().cnr_dist_stats_workspace_bytes(len(d)), d.device, "cnr_dist_stats")
    s = torch.empty(1, device=d.device, dtype=torch.float64)
    c = torch.empty(1, device=d.device, dtype=torch.int64)
    _C.call("cnr_dist_stats", d, len(d), float(th), ws, s, c)
    return s, c


def dist_stats(dist, th=float("inf")):
    """(sum of the distances in fp64, number below th) of an f32 device tensor -> (float, int)"""
    s, c = _stats_device(dist, th)
    return float(s.item()), int(c.item())


def _mean_ratio(dist, th):
    s, c = dist_stats(dist, th)
    return s / len(dist), c / len(dist)


def accuracy(gt_points, rec_points):
    """mean over the reconstruction's points of the distance to the nearest ground-truth point"""
    return _mean_ratio(nn_dist(rec_points, gt_points), float("inf"))[0]


def completion(gt_points, rec_points):
    """mean over the ground-truth points of the distance to the nearest reconstructed point"""
    return _mean_ratio(nn_dist(gt_points, rec_points), float("inf"))[0]


def accuracy_ratio(gt_points, rec_points, dist_th=0.01):
    """fraction of the reconstruction's points closer than dist_th to the ground truth"""
    return _mean_ratio(nn_dist(rec_points, gt_points), dist_th)[1]


def completion_ratio(gt_points, rec_points, dist_th=0.01):
    """fraction of the ground-truth points closer than dist_th to the reconstruction"""
    return _mean_ratio(nn_dist(gt_points, rec_points), dist_th)[1]


def chamfer(gt_points, rec_points):
    """(completion + accuracy) / 2"""
    return (completion(gt_points, rec_points) + accuracy(gt_points, rec_points)) / 2.0


# ---- triangles on the device: a devmesh.DeviceMesh (faces None: a soup, three rows of verts per face) ---------------------
def _area_scan(tri):
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    ws = _C.workspace(_C.load().cnr_face_area_workspace_bytes(F), verts.device, "cnr_face_area_scan")
    area = torch.empty(F, device=verts.device, dtype=torch.float64)
    cum = torch.empty(F, device=verts.device, dtype=torch.float64)
    _C.call("cnr_face_area_scan", verts, faces, F, ws, area, cum)
    return area, cum


def _sample(tri, count, rng, with_face=False):
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    if F < 1:
        raise ValueError("cannot sample a mesh without faces")
    _, cum = _area_scan(tri)
    u = torch.from_numpy(rng.random((int(count), 3))).to(verts.device)
    out = torch.empty(int(count), 3, device=verts.device, dtype=torch.float32)
    _C.call("cnr_sample_surface", verts, faces, F, cum, u, int(count), out)
    if not with_face:
        return out
    face = torch.empty(int(count), device=verts.device, dtype=torch.int32)
    _C.call("cnr_sample_faces", cum, F, u, int(count), face)
    return out, face


def sample_surface(mesh, count, seed=0):
    """trimesh.sample.sample_surface's algorithm on the GPU: `count` area-weighted points of `mesh` (a vis.Mesh or anything
    devmesh.device_mesh takes) from numpy.random.default_rng(seed).random((count, 3)) -> (count, 3) f32 device tensor.
    seed may be a numpy Generator, which default_rng hands back as it is: the draw then advances the caller's stream."""
    return _sample(device_mesh(mesh), count, np.random.default_rng(seed))


def sample_surface_faces(mesh, count, seed=0):
    """sample_surface with the face every sample was drawn from -> (points (count,3) f32, face (count,) i32) device tensors;
    the same draws, so points is bit-equal to sample_surface(mesh, count, seed)"""
    return _sample(device_mesh(mesh), count, np.random.default_rng(seed), with_face=True)


# ---- point to mesh -----------------------------------------------------------------------------------------------------
def _point_mesh(q, tri, closest=False):
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    if F < 1:
        raise ValueError("point_mesh_distance of a mesh without faces")
    nq, dev = len(q), q.device
    ws = _C.workspace(_C.load().cnr_point_mesh_workspace_bytes(nq, F), dev, "cnr_point_mesh_dist")
    dist = torch.empty(nq, device=dev, dtype=torch.float32)
    face = torch.empty(nq, device=dev, dtype=torch.int32)
    near = torch.empty(nq, 3, device=dev, dtype=torch.float32) if closest else None
    _C.call("cnr_point_mesh_dist", q, nq, verts, faces, F, dist, face, near, ws)
    return (dist, face, near) if closest else (dist, face)


class MeshIndex:
    """The tile-box index of one mesh (csrc/point_mesh_index.hip, DESIGN.md §3.20 "The tile-box index"): the faces ordered along
    a Morton curve, a bounding box per tile of `tile_faces` consecutive faces.  Built once (three launches and a sort), it
    answers any number of ``query`` calls with cnr_point_mesh_dist's result bit for bit while evaluating only the tiles that can
    hold a query group's minimum.  `mesh` and `check` as for point_mesh_distance.  Holds device tensors only."""

    def __init__(self, mesh, check=True):
        tri = device_mesh(mesh, check=check, what="MeshIndex")
        verts, faces, F, dev = tri.verts, tri.faces, tri.n_faces, tri.device
        if F < 1:
            raise ValueError("MeshIndex of a mesh without faces")
        if check:
            require_finite(verts, "MeshIndex")
        self.device, self.faces, self.check = dev, F, check
        self.tile_faces, self.group_queries = _index_params()
        self.tiles = -(-F // self.tile_faces)
        self.bbox = torch.cat([verts.amin(0), verts.amax(0)]).contiguous()
        keys = torch.empty(F, device=dev, dtype=torch.int32)
        _C.call("cnr_pm_index_keys", verts, faces, F, self.bbox, keys)
        order = torch.sort(keys, stable=True).indices
        self.index = _C.workspace(_C.load().cnr_pm_index_bytes(F), dev, "cnr_pm_index_build")
        _C.call("cnr_pm_index_build", verts, faces, F, keys, order, self.index)

    def _query(self, q, closest=False):
        nq, dev = len(q), q.device
        if dev != self.device:
            raise ValueError("MeshIndex.query: the points are on another device than the index")
        keys = torch.empty(nq, device=dev, dtype=torch.int32)
        _C.call("cnr_pm_query_keys", q, nq, self.bbox, keys)
        order = torch.sort(keys, stable=True).indices
        ws = _C.workspace(_C.load().cnr_point_mesh_indexed_workspace_bytes(nq, self.faces), dev, "cnr_point_mesh_dist_indexed")
        dist = torch.empty(nq, device=dev, dtype=torch.float32)
        face = torch.empty(nq, device=dev, dtype=torch.int32)
        near = torch.empty(nq, 3, device=dev, dtype=torch.float32) if closest else None
        _C.call("cnr_point_mesh_dist_indexed", q, nq, keys, order, self.index, self.faces, dist, face, near, ws)
        groups = -(-nq // self.group_queries)
        return dist, face, near, ws[:4 * groups].view(torch.int32)

    def query(self, points, closest=False, stats=False, check=None):
        """-> (dist, face[, closest][, stats]) as point_mesh_distance; stats = dict(tiles, groups, tiles_visited, tile_faces,
        group_queries): tiles_visited of groups * tiles tile evaluations were made (the one host read of the call).
        check: whether non-finite points raise ValueError; None takes the index's own setting"""
        q = _points(points, self.device)
        if self.check if check is None else check:
            require_finite(q, "point_mesh_distance")
        dist, face, near, visited = self._query(q, closest)
        out = (dist, face, near) if closest else (dist, face)
        if stats:
            out += (dict(tiles=self.tiles, groups=len(visited), tiles_visited=int(visited.sum()), tile_faces=self.tile_faces,
                         group_queries=self.group_queries),)
        return out


def _index_params():
    import ctypes
    tile, group = ctypes.c_int(0), ctypes.c_int(0)
    rc = _C.load().cnr_pm_index_params(ctypes.byref(tile), ctypes.byref(group))
    if rc != 0:
        raise _C.CnrError(f"cnr_pm_index_params failed with {rc}")
    return tile.value, group.value


def _distance(q, tri, index):
    """(dist, face) of device points to a DeviceMesh: brute force, or through a throw-away MeshIndex"""
    if not index:
        return _point_mesh(q, tri)
    return MeshIndex(tri, check=False)._query(q)[:2]


def point_mesh_distance(points, mesh, closest=False, check=True, index=None):
    """The exact distance of every point to a triangle mesh (cnr_point_mesh_dist, csrc/point_mesh.hip): brute
    force over all faces in fp32, difference first.  `mesh`: a vis.Mesh, a (verts, faces) pair, or a ((F*3,3) soup, None) pair.
    -> (dist (n,) f32, face (n,) i32: the lowest index among the closest faces) and, with closest=True, the closest point
    (n,3) f32; device tensors.  A face with coincident or collinear corners counts as the segment or point it covers.
    check=True (the default) raises ValueError for non-finite coordinates and faces that index outside the vertices.
    index: None or False is the brute force; True builds a throw-away MeshIndex of `mesh` and queries it; a MeshIndex is used
    as given (`mesh` is then not read, and `check` applies to the points alone: the mesh was checked, or not, when the index
    was built).  The result is the same bit for bit."""
    if isinstance(index, MeshIndex):
        return index.query(points, closest=closest, check=check)
    q = _points(points)
    tri = device_mesh(mesh, q.device, check=check, what="point_mesh_distance")
    if index:
        return MeshIndex(tri, check=check).query(q, closest=closest)
    if check:
        require_finite(q, "point_mesh_distance")
        require_finite(tri.verts, "point_mesh_distance")
    return _point_mesh(q, tri, closest)


# ---- inside and outside ------------------------------------------------------------------------------------------------
def _winding(q, tri):
    """w (nq,) f64 of device points about a DeviceMesh with at least one face (the callers refuse an empty one by name)"""
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    nq, dev = len(q), q.device
    ws = _C.workspace(_C.load().cnr_winding_workspace_bytes(nq, F), dev, "cnr_winding_number")
    w = torch.empty(nq, device=dev, dtype=torch.float64)
    _C.call("cnr_winding_number", q, nq, verts, faces, F, w, ws)
    return w


def _winding_inputs(points, mesh, check, what):
    q = _points(points)
    tri = device_mesh(mesh, q.device, check=check, what=what)
    if tri.n_faces < 1:
        raise ValueError(f"{what} of a mesh without faces")
    if check:
        require_finite(q, what)
        require_finite(tri.verts, what)
    return q, tri


def winding_number(points, mesh, check=True):
    """The generalized winding number (Jacobson et al. 2013) of a triangle mesh about every point (cnr_winding_number,
    csrc/winding.hip): the sum over all faces of the signed solid angle, divided by 4 pi, brute force in fp64.
    `mesh` and `check` as for point_mesh_distance.  -> (n,) f64 device tensor: +1 inside a closed mesh whose right-hand normals
    point outward (-1 when they point inward, as vis.marching_cubes' do), 0 outside; on an open mesh it falls off smoothly across a hole, and
    is thresholded at 0.5.  A point in the plane of a face gets nothing from that face, so on the surface itself the value
    is the mean of the two sides.  A mesh whose faces are not consistently oriented has no meaningful winding number
    (meshops.orient repairs one; inside, signed_distance and volume_iou take orientation="repair")."""
    q, tri = _winding_inputs(points, mesh, check, "winding_number")
    return _winding(q, tri)


def _signed_volume(verts, faces):
    """sum over the faces of (a - c0) . ((b - c0) x (c - c0)) in fp64, c0 the centre of the vertices' box; tensors on any device"""
    v = verts.double()
    c = v - 0.5 * (v.amin(0) + v.amax(0))
    c = c.view(-1, 3, 3) if faces is None else c[faces.long()]
    return (c[:, 0] * torch.linalg.cross(c[:, 1], c[:, 2])).sum()


def mesh_orientation(mesh):
    """+1 when the mesh's right-hand normals point outward, -1 when inward: the sign (>= 0 -> +1) of the fp64 signed volume
    sum_f (a - c0) . ((b - c0) x (c - c0)) about the centre c0 of the vertices' box, in torch on the device.  Exact for a closed
    mesh; for an open one it is a heuristic (a bowl seen from far outside its box centre can fool it), and it does not detect
    faces that are not consistently oriented.  vis.marching_cubes' meshes (Trainer.meshing's) are inward, loaded ground truths
    usually outward."""
    tri = device_mesh(mesh, what="mesh_orientation")
    if tri.n_faces < 1:
        raise ValueError("mesh_orientation of a mesh without faces")
    return _orientation_sign("auto", tri)


def _repair(orientation, tri):
    """orientation="repair": the mesh through meshops.orient(..., outward=True), then treated as "outward";
    any other orientation: as it is.  -> (orientation, DeviceMesh)"""
    if orientation != "repair":
        return orientation, tri
    from . import meshops
    if tri.faces is None:
        raise ValueError('orientation="repair" needs an indexed mesh, not a triangle soup (weld it first)')
    fixed = meshops.orient(tri.faces, len(tri.verts), verts=tri.verts, outward=True)
    return "outward", DeviceMesh(tri.verts, fixed.faces, tri.colors, tri.normals)


def _orientation_sign(orientation, tri):
    if orientation == "auto":
        return 1 if float(_signed_volume(tri.verts, tri.faces)) >= 0 else -1
    if orientation in ("outward", "inward"):
        return 1 if orientation == "outward" else -1
    raise ValueError(f'orientation must be "auto", "outward", "inward" or "repair", not {orientation!r}')


def _inside(q, tri, threshold, orientation):
    s = _orientation_sign(orientation, tri)
    w = _winding(q, tri)
    return (w if s > 0 else -w) > threshold


def inside(points, mesh, threshold=0.5, orientation="auto", check=True):
    """-> (n,) bool device tensor: s w > threshold with w = winding_number(points, mesh) and s = +1 for orientation="outward",
    -1 for "inward", mesh_orientation(mesh) for "auto".  orientation="repair" first makes the faces consistent and every patch
    outward (meshops.orient), then takes s = +1.  `mesh` and `check` as for point_mesh_distance."""
    q, tri = _winding_inputs(points, mesh, check, "inside")
    orientation, tri = _repair(orientation, tri)
    return _inside(q, tri, threshold, orientation)


def signed_distance(points, mesh, threshold=0.5, orientation="auto", closest=False, index=None, check=True):
    """point_mesh_distance with the distance negated where inside(points, mesh, threshold, orientation): negative is inside.
    -> (sdist (n,) f32, face (n,) i32[, closest (n,3) f32]); the magnitude, the face and the closest point are
    point_mesh_distance's bit for bit, with or without `index` (which is passed through; the winding number itself is always
    taken over all faces of `mesh`, so `mesh` is read also when index is a MeshIndex).  orientation="repair" as for inside."""
    q, tri = _winding_inputs(points, mesh, check, "signed_distance")
    out = point_mesh_distance(q, tri, closest=closest, check=False, index=index)     # both were checked above
    orientation, wound = _repair(orientation, tri)     # flipping a face moves no surface point: the distance is of `mesh` as given
    flag = _inside(q, wound, threshold, orientation)
    return (torch.where(flag, -out[0], out[0]),) + tuple(out[1:])


def _box_points(u, box, meshes):
    """the (N,3) uniforms u (f64, host) scaled in fp64 into the box, rounded to fp32 once -> (points f32 host, box volume)"""
    if box is None:
        lo = np.min([m.verts.amin(0).double().cpu().numpy() for m in meshes], 0)
        hi = np.max([m.verts.amax(0).double().cpu().numpy() for m in meshes], 0)
        return (lo + u * (hi - lo)).astype(np.float32), float(np.prod(hi - lo))
    extents = np.asarray(box[1], np.float64).reshape(3)
    Ti = np.linalg.inv(np.asarray(box[0], np.float64).reshape(4, 4))    # box_planes' box: |local| <= extents / 2 at inv(transform)
    return (((u - 0.5) * extents) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32), float(np.prod(extents))


def volume_iou(mesh_a, mesh_b, N=100000, seed=0, box=None, points=None, threshold=0.5, orientation=("auto", "auto")):
    """Volumetric intersection over union of two meshes by counting: N points numpy.random.default_rng(seed).random((N,3)),
    scaled in fp64 and rounded to fp32 once, fill the axis-aligned box of both meshes' vertices (box=None) or the oriented box
    box=(transform, extents) as oriented_bounds returns it (the one box_planes(transform, extents) describes); points= takes
    explicit points instead.  Each is classified by inside(., mesh, threshold, orientation[k]).
    -> dict(iou, intersection, union, inside_a, inside_b, n (exact integer counts; iou = nan when union == 0), volume_a, volume_b
    (the inside share times the box volume; nan with points=, which have no box), orientation_a, orientation_b (+1 / -1 as used)).
    Open meshes are welcome (the winding number closes a hole smoothly); inconsistently oriented ones are not, unless their
    orientation is "repair": that mesh goes through meshops.orient(..., outward=True) first and is reported as +1."""
    dev = _device()
    a = device_mesh(mesh_a, dev, what="volume_iou")
    b = device_mesh(mesh_b, dev, what="volume_iou")
    for m in (a, b):
        if m.n_faces < 1:
            raise ValueError("volume_iou of a mesh without faces")
        require_finite(m.verts, "volume_iou")
    if points is not None:
        q, volume = _points(points, dev), float("nan")
        require_finite(q, "volume_iou")
    else:
        if int(N) < 1:
            raise ValueError("volume_iou needs N >= 1 points")
        host, volume = _box_points(np.random.default_rng(seed).random((int(N), 3)), box, (a, b))
        q = torch.from_numpy(host).to(dev)
    (oa, a), (ob, b) = _repair(orientation[0], a), _repair(orientation[1], b)
    sa, sb = _orientation_sign(oa, a), _orientation_sign(ob, b)
    ia = _inside(q, a, threshold, "outward" if sa > 0 else "inward")
    ib = _inside(q, b, threshold, "outward" if sb > 0 else "inward")
    n = len(q)
    na, nb, inter, union = (int(v) for v in torch.stack([ia.sum(), ib.sum(), (ia & ib).sum(), (ia | ib).sum()]).cpu())
    return dict(iou=inter / union if union else float("nan"), intersection=inter, union=union, inside_a=na, inside_b=nb, n=n,
                volume_a=na / n * volume, volume_b=nb / n * volume, orientation_a=sa, orientation_b=sb)


def _unit_face_normals(tri):
    """(F,3) f64 unit normals: the fp64 cross product of the fp32 corners, normalised; zero rows for faces without one"""
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    c = verts.double().view(F, 3, 3) if faces is None else verts.double()[faces.long()]
    n = torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    ln = n.norm(dim=1, keepdim=True)
    return torch.where(ln > 0, n / torch.where(ln > 0, ln, torch.ones_like(ln)), torch.zeros_like(n))


def _normal_consistency(n_src, n_dst):
    """mean |n_src . n_dst| over the pairs where both normals exist -> (mean or nan, pairs)"""
    ok = (n_src.abs().sum(1) > 0) & (n_dst.abs().sum(1) > 0)
    pairs = int(ok.sum())
    if pairs == 0:
        return float("nan"), 0
    return float(((n_src * n_dst).sum(1).abs() * ok).sum() / pairs), pairs


def _metric_inputs(mesh_rec, mesh_ref, mesh_gt, seed):
    """The opening calc_3d_metric and calc_3d_metric_surface share -> (rec, rec clipped to mesh_ref's oriented box, gt, rng),
    or None after printing "no mesh found".  The draws from rng, in this order: the whole reconstruction, its clip, the ground
    truth -- (N,3) uniforms each."""
    transform, extents = oriented_bounds(mesh_ref)
    dev = _device()
    rec = device_mesh(mesh_rec, dev)
    rec_acc = _clip(rec, box_planes(transform, extents))
    if rec_acc is None:
        print("no mesh found")
        return None
    return rec, rec_acc, device_mesh(mesh_ref if mesh_gt is None else mesh_gt, dev), np.random.default_rng(seed)


def calc_3d_metric_surface(mesh_rec, mesh_ref, N=200000, mesh_gt=None, seed=0, threshold=0.05, index=False):
    """calc_3d_metric with every distance taken from a sample to the other MESH, not to samples of it: the same oriented box
    and clip, the same three draws in the same order from numpy.random.default_rng(seed).  Accuracy: the clipped
    reconstruction's samples to the ground-truth mesh; completion: the ground truth's samples to the whole reconstruction.
    -> dict(accuracy_cm, completion_cm, completion_ratio (% below threshold), precision, recall (fractions below threshold),
    fscore (their harmonic mean, 0 when both are 0), normal_consistency_acc, normal_consistency_comp, normal_consistency (their
    mean), normal_pairs (acc, comp)), or None after printing "no mesh found".  Normal consistency is the mean |n_src . n_dst| of
    the unit normal of the face a sample came from and that of its closest face (unsigned: ground-truth meshes are not
    consistently oriented); pairs with a face without a normal on either side are left out and counted.  index=True takes the two
    distances through a MeshIndex of each mesh (the same numbers, fewer pairs)."""
    inputs = _metric_inputs(mesh_rec, mesh_ref, mesh_gt, seed)
    if inputs is None:
        return None
    rec, rec_acc, gt, rng = inputs
    rng.random((int(N), 3))                                 # calc_3d_metric's first draw (the whole reconstruction): not needed here
    acc_pc, acc_src = _sample(rec_acc, N, rng, with_face=True)
    gt_pc, gt_src = _sample(gt, N, rng, with_face=True)
    d_acc, f_acc = _distance(acc_pc, gt, index)
    d_comp, f_comp = _distance(gt_pc, rec, index)
    s_acc, c_acc = (v.item() for v in _stats_device(d_acc, threshold))
    s_comp, c_comp = (v.item() for v in _stats_device(d_comp, threshold))
    precision, recall = c_acc / N, c_comp / N
    n_rec_acc, n_gt, n_rec = _unit_face_normals(rec_acc), _unit_face_normals(gt), _unit_face_normals(rec)
    nc_acc, p_acc = _normal_consistency(n_rec_acc[acc_src.long()], n_gt[f_acc.long()])
    nc_comp, p_comp = _normal_consistency(n_gt[gt_src.long()], n_rec[f_comp.long()])
    return dict(accuracy_cm=s_acc / N * 100, completion_cm=s_comp / N * 100, completion_ratio=c_comp / N * 100,
                precision=precision, recall=recall,
                fscore=2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0,
                normal_consistency_acc=nc_acc, normal_consistency_comp=nc_comp, normal_consistency=(nc_acc + nc_comp) / 2,
                normal_pairs=(p_acc, p_comp))


# ---- oriented bounding box (host) --------------------------------------------------------------------------------------
_MAX_NORMALS = 512
_MAX_HULL_POINTS = 4096


def _plane_frame(n):
    """rows e1, e2, n: a right-handed orthonormal frame with n as its third axis"""
    n = n / np.linalg.norm(n)
    a = np.eye(3)[np.argmin(np.abs(n))]
    e1 = np.cross(n, a)
    e1 /= np.linalg.norm(e1)
    return np.stack([e1, np.cross(n, e1), n])


def _min_rect(p2):
    """minimum-area rectangle of 2-D points over the directions of their hull's edges -> (area, 2x2 rotation rows)"""
    from scipy.spatial import ConvexHull
    try:
        h = p2[ConvexHull(p2).vertices]
    except Exception:           # collinear / a single point: the principal direction
        h = p2
        _, _, vt = np.linalg.svd(p2 - p2.mean(0), full_matrices=False)
        d = vt[:1]
    else:
        e = np.roll(h, -1, 0) - h
        ln = np.linalg.norm(e, axis=1)
        d = e[ln > 0] / ln[ln > 0, None]
    perp = np.stack([-d[:, 1], d[:, 0]], 1)
    pu, pv = h @ d.T, h @ perp.T
    area = (pu.max(0) - pu.min(0)) * (pv.max(0) - pv.min(0))
    k = int(np.argmin(area))
    return float(area[k]), np.stack([d[k], perp[k]])


def oriented_bounds(mesh):
    """trimesh.bounds.oriented_bounds' search: for every distinct face normal of the convex hull of the vertices, the
    minimum-area rectangle of the hull projected along it (rotating hull-edge directions) times the extent along it; the box
    of least volume.  The coordinate axes and the principal axes are candidates too, so the box is never larger than the
    axis-aligned or the PCA box.  `mesh`: a mesh (the vertices its faces use) or an (n,3) point array.  A flat (or degenerate) point set gets a zero extent along its normal.  Hulls beyond
    _MAX_NORMALS distinct normals (finely tessellated round shapes) try the normals of their largest faces only, and beyond
    _MAX_HULL_POINTS vertices choose the rotation on every k-th of them; the extents always bound every point.
    -> (transform (4,4): moves the box centre to the origin and its edges onto the axes, extents (3,))"""
    from scipy.spatial import ConvexHull
    if hasattr(mesh, "vertices"):
        pts = np.asarray(mesh.vertices, np.float64).reshape(-1, 3)
        faces = np.asarray(getattr(mesh, "faces", np.zeros(0)), np.int64).reshape(-1)
        if len(faces):                          # the vertices the faces use (a mesh may carry unreferenced ones)
            pts = pts[np.unique(faces)]
    else:
        pts = np.asarray(mesh, np.float64).reshape(-1, 3)
    if len(pts) == 0:
        raise ValueError("oriented_bounds of an empty point set")
    c0 = pts.mean(0)
    _, _, vt = np.linalg.svd(pts - c0, full_matrices=False)
    cands = [np.eye(3), vt]
    try:
        hull = ConvexHull(pts)
        hp = pts[hull.vertices]
        nrm = hull.equations[:, :3]
        _, first = np.unique(np.round(nrm, 9), axis=0, return_index=True)
        first = np.sort(first)
        if len(first) > _MAX_NORMALS:           # a finely tessellated round hull: the normals of its largest faces
            tri = pts[hull.simplices[first]]
            area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
            first = np.sort(first[np.argsort(-area, kind="stable")[:_MAX_NORMALS]])
        cands.append(nrm[first])
    except Exception:           # flat or degenerate: the principal frame covers it
        hp = pts
    if len(hp) > _MAX_HULL_POINTS:              # the search on every k-th hull point; the extents below use every point
        hp = hp[::-(-len(hp) // _MAX_HULL_POINTS)]
    best = None
    for n in np.concatenate(cands, 0):
        if not np.isfinite(n).all() or np.linalg.norm(n) == 0:
            continue
        Fr = _plane_frame(n)
        loc = (hp - c0) @ Fr.T
        h = loc[:, 2].max() - loc[:, 2].min()
        area, R2 = _min_rect(loc[:, :2])
        vol = area * h
        key = (vol, area)
        if best is None or key < best[0]:
            R = np.eye(3)
            R[:2] = R2 @ Fr[:2]
            R[2] = Fr[2]
            best = (key, R)
    R = best[1]
    loc = pts @ R.T
    lo, hi = loc.min(0), loc.max(0)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -(lo + hi) / 2.0
    return T, hi - lo


def box_planes(transform, extents):
    """the six faces of the box of `extents` at inv(transform), as (6,6) f64 rows (origin, inward normal)"""
    T = np.asarray(transform, np.float64).reshape(4, 4)
    Ti = np.linalg.inv(T)
    ext = np.asarray(extents, np.float64).reshape(3)
    rows = []
    for i in range(3):
        for s in (1.0, -1.0):
            o, n = np.zeros(3), np.zeros(3)
            o[i], n[i] = s * ext[i] / 2.0, -s
            rows.append(np.concatenate([Ti[:3, :3] @ o + Ti[:3, 3], T[:3, :3].T @ n]))
    return np.array(rows)


def _clip(tri, planes):
    """the part of a DeviceMesh inside the box of `planes` -> a soup DeviceMesh, or None when nothing is inside"""
    verts, faces, F = tri.verts, tri.faces, tri.n_faces
    if F < 1:
        return None
    dev = verts.device
    pl = torch.from_numpy(np.ascontiguousarray(planes, np.float64)).to(dev)
    ws = _C.workspace(_C.load().cnr_clip_box_workspace_bytes(F), dev, "cnr_clip_box")
    cnt = torch.empty(1, device=dev, dtype=torch.int64)
    _C.call("cnr_clip_box_count", verts, faces, F, pl, ws, cnt)
    T = int(cnt.item())
    if T == 0:
        return None
    tris = torch.empty(T, 3, 3, device=dev, dtype=torch.float32)
    _C.call("cnr_clip_box_emit", verts, faces, F, pl, ws, tris)
    return DeviceMesh(tris.view(T * 3, 3), None)


def slice_box(mesh, transform, extents):
    """mesh.slice_plane(box.facets_origin, -box.facets_normal) for box = the box of `extents` at inv(transform): the part of
    the mesh inside the box, crossing triangles split, no cap -> vis.Mesh (an unindexed soup: 3 vertices per triangle; no
    vertices when nothing is inside)"""
    from .vis import Mesh
    out = _clip(device_mesh(mesh), box_planes(transform, extents))
    if out is None:
        return Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    v = out.verts.double().cpu().numpy()
    return Mesh(v, np.arange(len(v), dtype=np.int64).reshape(-1, 3))


def calc_3d_metric(mesh_rec, mesh_ref, N=200000, mesh_gt=None, seed=0):
    """metric/eval_3D_obj.py:10-39: [[accuracy cm], [completion cm], [completion ratio at 5 cm, %]], or None (after printing
    "no mesh found") when nothing of mesh_rec lies in mesh_ref's oriented box.  Accuracy uses the reconstruction clipped to
    that box, completion and its ratio the whole reconstruction."""
    inputs = _metric_inputs(mesh_rec, mesh_ref, mesh_gt, seed)
    if inputs is None:
        return None
    rec, rec_acc, gt, rng = inputs
    rec_pc = _sample(rec, N, rng)
    rec_pc_for_acc = _sample(rec_acc, N, rng)
    gt_pc = _sample(gt, N, rng)
    s_acc, _ = _stats_device(nn_dist(rec_pc_for_acc, gt_pc), float("inf"))
    s_comp, c_comp = _stats_device(nn_dist(gt_pc, rec_pc), 0.05)
    acc, comp, cnt = (v.item() for v in (s_acc, s_comp, c_comp))
    return [[acc / N * 100], [comp / N * 100], [cnt / N * 100]]


# ---- depth L1 ----------------------------------------------------------------------------------------------------------
def depth_l1_images(depth_rec, depth_gt):
    """Two stacks of depth images of one shape (tensors on any device, 0 = nothing hit) -> (sum of |rec - gt| over the pixels
    hit in both, float64 tensor; both, only_rec, only_gt, neither: Python ints)"""
    a, b = torch.as_tensor(depth_rec), torch.as_tensor(depth_gt)
    if a.shape != b.shape:
        raise ValueError("depth images of different shapes: {} and {}".format(tuple(a.shape), tuple(b.shape)))
    ha, hb = a > 0, b > 0
    both = ha & hb
    total = ((a.double() - b.double()).abs() * both).sum()
    n = [int(x) for x in torch.stack([both.sum(), (ha & ~hb).sum(), (~ha & hb).sum(), (~ha & ~hb).sum()]).tolist()]
    return total, n[0], n[1], n[2], n[3]


def depth_l1(mesh_rec, mesh_gt, T_wcs, rasterizer, views_per_launch=None):
    """The depth L1 of the usual reconstruction table: both meshes (``vis.Mesh``, a tuple, or a ``raster.MeshScene``) rendered
    by ``rasterizer`` (``raster.MeshRasterizer``) from the poses ``T_wcs`` (V,4,4) -> {l1: the mean |depth_rec - depth_gt| in
    metres over the pixels of all views where both were hit (summed in fp64 on the device; nan when there is no such pixel),
    both, only_rec, only_gt, neither: the pixel counts}."""
    from . import raster
    scenes = [m if isinstance(m, raster.MeshScene) else raster.MeshScene(m, device=rasterizer.device) for m in (mesh_rec, mesh_gt)]
    T, _ = raster._poses(T_wcs)
    step = min(rasterizer.views_per_launch(s, views_per_launch) for s in scenes)
    total, counts = torch.zeros((), dtype=torch.float64, device=rasterizer.device), [0, 0, 0, 0]
    for a in range(0, T.shape[0], step):
        d = [rasterizer.render(s, T[a:a + step], attributes=False, views_per_launch=step)["depth"] for s in scenes]
        part = depth_l1_images(d[0], d[1])
        total = total + part[0]
        counts = [c + p for c, p in zip(counts, part[1:])]
    l1 = float(total) / counts[0] if counts[0] else float("nan")
    return dict(l1=l1, both=counts[0], only_rec=counts[1], only_gt=counts[2], neither=counts[3])
