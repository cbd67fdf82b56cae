"""The mesh as a graph, on the device (csrc/mesh_topo.hip): welding of coincident vertices, connected
components by edge or by vertex with their table (faces, vertices, area, bounding box, boundary / non-manifold edges,
watertightness), compaction of a face selection, ``clean_mesh``: dropping the floaters of a marching-cubes mesh, and ``orient``:
consistent winding per patch and outward patches.  And making
it smaller (csrc/mesh_simplify.hip): ``simplify``, uniform vertex clustering with quadric placement, and
``vertex_normals``.

Device tensors in and out (``clean_mesh``, ``simplify_mesh`` and ``deviation_mesh`` take a host ``vis.Mesh``).  The sorts are
``torch.sort(stable=True)``, every other step is a HIP kernel; there is no CPU path.  A union/find loop that runs out of its bound
raises CnrError, an out-of-range face index raises ValueError."""
import numpy as np
import torch

from . import _C
from .devmesh import DeviceMesh, check_faces, device_mesh, require_finite
from .vis import Mesh

CONNECTIVITY = ("edge", "vertex")
LARGEST_BY = ("area", "faces", "diag")


def _raise_if_set(err, what):
    e = int(err.item())
    if e & 4:
        raise ValueError(f"{what}: a vertex is not finite, or the grid has more than 2^21 cells on an axis")
    if e & 2:
        raise ValueError(f"{what}: an index lies outside its range")
    if e & 1:
        raise _C.CnrError(f"{what}: a union/find loop ran out of its bound (the label array is corrupt)")


def _flatten(labels, n, err):
    ws = _C.workspace(_C.load().cnr_mesh_flatten_workspace_bytes(n), labels.device, "cnr_mesh_flatten")
    _C.call("cnr_mesh_flatten", labels, n, ws, err)


def _roots(labels, used, n):
    """the ascending roots (C,) int32 of a flattened label array"""
    dev = labels.device
    ws = _C.workspace(_C.load().cnr_mesh_roots_workspace_bytes(n), dev, "cnr_mesh_roots")
    cnt = torch.empty(1, device=dev, dtype=torch.int64)
    _C.call("cnr_mesh_roots_count", labels, used, n, ws, cnt)
    C = int(cnt.item())
    roots = torch.empty(C, device=dev, dtype=torch.int32)
    if C:
        _C.call("cnr_mesh_roots_emit", labels, used, n, ws, roots)
    return roots


def union_find(pairs, n, check=True):
    """labels (n,) int32 of the partition of 0 .. n-1 that the pairs (m,2) int32 generate: labels[i] = the smallest element of
    i's set, whatever the order of the pairs."""
    n = int(n)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs must have the shape (m,2)")
    pairs = pairs.to(torch.int32).contiguous()
    dev = pairs.device
    labels = torch.empty(n, device=dev, dtype=torch.int32)
    if n == 0:
        return labels
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    _C.call("cnr_mesh_labels_init", labels, n)
    if len(pairs):
        _C.call("cnr_mesh_union_pairs", pairs, len(pairs), n, labels, err)
    _flatten(labels, n, err)
    if check:
        _raise_if_set(err, "cnr_mesh_union_pairs")
    return labels


class MeshComponents:
    """The component table of ``components``.  n components, numbered by their smallest element (``first``: a face index with
    connectivity "edge", a vertex index with "vertex").  face_component (F,) i32; vertex_component (V,) i32, -1 for a vertex no
    face uses -- with "edge" a vertex where two components touch belongs to the lower one, and counts in its n_vertices.
    n_faces, n_vertices (n,) i32; area (n,) f64, bbox_min / bbox_max (n,3) f32, diag (n,) f64 (None without verts);
    edge_counts (n,3) i32 = boundary, non-manifold and same-direction interior edges per component; boundary_edges and
    nonmanifold_edges their totals (python ints); watertight (n,) bool."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def table(self):
        """one line per component, for printing"""
        cols = {k: getattr(self, k).cpu().numpy() for k in ("first", "n_faces", "n_vertices", "watertight")}
        area = self.area.cpu().numpy() if self.area is not None else np.full(self.n, np.nan)
        diag = self.diag.cpu().numpy() if self.diag is not None else np.full(self.n, np.nan)
        ec = self.edge_counts.cpu().numpy()
        lines = ["%5s %9s %9s %9s %14s %12s %8s %8s %5s" % ("id", "first", "faces", "vertices", "area", "diag", "boundary",
                                                          "nonmanif", "tight")]
        for c in range(self.n):
            lines.append("%5d %9d %9d %9d %14.8g %12.6g %8d %8d %5s" % (c, cols["first"][c], cols["n_faces"][c], cols["n_vertices"][c],
                                                                      area[c], diag[c], ec[c, 0], ec[c, 1],
                                                                      "yes" if cols["watertight"][c] else "no"))
        return "\n".join(lines)


def _empty_components(F, V, dev, with_verts):
    z32 = torch.zeros(0, device=dev, dtype=torch.int32)
    return MeshComponents(n=0, connectivity=None, face_component=torch.zeros(F, device=dev, dtype=torch.int32),
                          vertex_component=torch.full((V,), -1, device=dev, dtype=torch.int32), first=z32, n_faces=z32.clone(),
                          n_vertices=z32.clone(), area=torch.zeros(0, device=dev, dtype=torch.float64) if with_verts else None,
                          bbox_min=torch.zeros(0, 3, device=dev) if with_verts else None,
                          bbox_max=torch.zeros(0, 3, device=dev) if with_verts else None,
                          diag=torch.zeros(0, device=dev, dtype=torch.float64) if with_verts else None,
                          edge_counts=torch.zeros(0, 3, device=dev, dtype=torch.int32), boundary_edges=0, nonmanifold_edges=0,
                          watertight=torch.zeros(0, device=dev, dtype=torch.bool), labels=z32.clone())


def components(faces, n_vertices, verts=None, connectivity="edge", timer=None):
    """Connected components of the faces (F,3) over n_vertices vertices -> MeshComponents.  "edge": two faces are connected when
    they share an edge (trimesh's ``split``, open3d's ``cluster_connected_triangles``); "vertex": when they share a vertex.
    verts (V,3) f32 adds area, bounding boxes and diagonals.  timer(name), when given, is called after every stage."""
    if connectivity not in CONNECTIVITY:
        raise ValueError(f"connectivity must be one of {CONNECTIVITY}, not {connectivity!r}")
    V = int(n_vertices)
    f = check_faces(faces, V, "components")
    F, dev = f.shape[0], f.device
    mark = timer or (lambda name: None)
    if verts is not None:
        if tuple(verts.shape) != (V, 3):
            raise ValueError(f"verts must have the shape ({V},3), not {tuple(verts.shape)}")
        verts = verts.float().contiguous()
    if F == 0:
        out = _empty_components(F, V, dev, verts is not None)
        out.connectivity = connectivity
        return out
    mark("check")
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    keys = torch.empty(3 * F, device=dev, dtype=torch.int64)
    _C.call("cnr_mesh_edge_keys", f, F, keys)
    mark("edge_keys")
    skeys, perm = torch.sort(keys, stable=True)
    mark("sort_edges")
    face_comp = torch.empty(F, device=dev, dtype=torch.int32)
    vert_comp = torch.empty(V, device=dev, dtype=torch.int32)
    by_vertex = connectivity == "vertex"                 # the sets are of vertices (those a face uses), else of faces
    n = V if by_vertex else F
    labels = torch.empty(n, device=dev, dtype=torch.int32)
    used = torch.zeros(V, device=dev, dtype=torch.uint8) if by_vertex else None
    _C.call("cnr_mesh_labels_init", labels, n)
    if by_vertex:
        _C.call("cnr_mesh_union_faces", f, F, V, labels, used, err)
    else:
        _C.call("cnr_mesh_union_edges", skeys, perm, F, labels, err)
    mark("union")
    _flatten(labels, n, err)
    mark("flatten")
    roots = _roots(labels, used, n)
    _raise_if_set(err, "components")
    _C.call("cnr_mesh_assign", labels, used, n, roots, len(roots), vert_comp if by_vertex else face_comp, err)
    _C.call("cnr_mesh_cross_component", f, F, V, 1 if by_vertex else 0, face_comp, vert_comp)
    C = len(roots)
    mark("roots_assign")
    edge_counts = torch.zeros(C, 3, device=dev, dtype=torch.int32)
    _C.call("cnr_mesh_edge_stats", skeys, perm, f, F, face_comp, C, edge_counts)
    mark("edge_stats")
    scomp, order = torch.sort(face_comp, stable=True)
    mark("sort_faces")
    n_faces = torch.empty(C, device=dev, dtype=torch.int32)
    n_verts = torch.empty(C, device=dev, dtype=torch.int32)
    area = bmin = bmax = diag = None
    if verts is not None:
        area = torch.empty(C, device=dev, dtype=torch.float64)
        bmin = torch.empty(C, 3, device=dev, dtype=torch.float32)
        bmax = torch.empty(C, 3, device=dev, dtype=torch.float32)
    ws = None
    if verts is not None:
        ws = _C.workspace(_C.load().cnr_mesh_component_stats_workspace_bytes(F), dev, "cnr_mesh_component_stats")
    _C.call("cnr_mesh_component_stats", verts, f, order, scomp, F, V, C, vert_comp, ws, n_faces, n_verts, area, bmin, bmax)
    mark("component_stats")
    _raise_if_set(err, "components")
    if verts is not None:
        d = bmax.double() - bmin.double()
        diag = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt()        # each step rounded once, in this order
    totals = edge_counts.sum(0).cpu()
    return MeshComponents(n=C, connectivity=connectivity, face_component=face_comp, vertex_component=vert_comp, first=roots,
                          n_faces=n_faces, n_vertices=n_verts, area=area, bbox_min=bmin, bbox_max=bmax, diag=diag,
                          edge_counts=edge_counts, boundary_edges=int(totals[0]), nonmanifold_edges=int(totals[1]),
                          watertight=(edge_counts == 0).all(dim=1), labels=labels)


class MeshOrientation:
    """The result of ``orient``.  faces (F,3) i32: the input with corners 1 and 2 swapped where flip (F,) u8 is set;
    face_patch (F,) i32; n patches, numbered by their smallest face ``first`` (n,) i32.  Per patch: n_faces (n,) i32,
    orientable (n,) bool, closed (n,) bool (every edge of its non-degenerate faces occurs exactly twice), inconsistent_edges
    (n,) i32 (links whose two faces ran the edge in the same direction in the INPUT), n_flipped (n,) i32, signed_volume (n,) f64
    after repair (None without verts)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def table(self):
        """one line per patch, for printing"""
        cols = {k: getattr(self, k).cpu().numpy() for k in ("first", "n_faces", "orientable", "closed", "inconsistent_edges",
                                                           "n_flipped")}
        vol = self.signed_volume.cpu().numpy() if self.signed_volume is not None else np.full(self.n, np.nan)
        lines = ["%5s %9s %9s %10s %6s %12s %9s %16s" % ("id", "first", "faces", "orientable", "closed", "inconsistent", "flipped",
                                                        "signed_volume")]
        for c in range(self.n):
            lines.append("%5d %9d %9d %10s %6s %12d %9d %16.9g" % (c, cols["first"][c], cols["n_faces"][c],
                                                                 "yes" if cols["orientable"][c] else "no",
                                                                 "yes" if cols["closed"][c] else "no", cols["inconsistent_edges"][c],
                                                                 cols["n_flipped"][c], vol[c]))
        return "\n".join(lines)


def orient(faces, n_vertices, verts=None, outward=None, timer=None):
    """Orientation repair (trimesh's ``fix_normals``) -> MeshOrientation.  Two faces are LINKED when they are
    the only two on an undirected edge; patches are the connected components under links (a non-manifold edge joins nothing,
    a face with two equal corners is a patch of its own and is never flipped).  Within an orientable patch every face is
    brought to the winding of the patch's smallest face; a patch that cannot be oriented (a Moebius band) is left as it is and
    flagged.  With verts (V,3) f32 and outward (default: verts is not None), a patch whose fp64 signed volume about the centre
    of its vertex box is negative is flipped as a whole: exact for a closed patch, for an open one the heuristic of
    ``metrics.mesh_orientation``.  Integer work plus one fixed-order fp64 sum per patch: bit-identical run to run.
    timer(name), when given, is called after every stage."""
    V = int(n_vertices)
    if outward is None:
        outward = verts is not None
    if outward and verts is None:
        raise ValueError("orient: outward=True needs verts")
    f = check_faces(faces, V, "orient")
    F, dev = f.shape[0], f.device
    mark = timer or (lambda name: None)
    if verts is not None:
        if tuple(verts.shape) != (V, 3):
            raise ValueError(f"verts must have the shape ({V},3), not {tuple(verts.shape)}")
        verts = verts.float().contiguous()
    if F == 0:
        z32 = torch.zeros(0, device=dev, dtype=torch.int32)
        zb = torch.zeros(0, device=dev, dtype=torch.bool)
        return MeshOrientation(n=0, faces=f, flip=torch.zeros(0, device=dev, dtype=torch.uint8), face_patch=z32, first=z32.clone(),
                               n_faces=z32.clone(), orientable=zb, closed=zb.clone(), inconsistent_edges=z32.clone(),
                               n_flipped=z32.clone(),
                               signed_volume=torch.zeros(0, device=dev, dtype=torch.float64) if verts is not None else None)
    mark("check")
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    keys = torch.empty(3 * F, device=dev, dtype=torch.int64)
    _C.call("cnr_mesh_orient_keys", f, F, keys)
    mark("edge_keys")
    skeys, perm = torch.sort(keys, stable=True)
    mark("sort_edges")
    words = torch.empty(F, device=dev, dtype=torch.int32)
    _C.call("cnr_mesh_orient_union", skeys, perm, f, F, words, err)
    mark("union")
    labels = torch.empty(F, device=dev, dtype=torch.int32)
    flip0 = torch.empty(F, device=dev, dtype=torch.uint8)
    ws = _C.workspace(_C.load().cnr_mesh_flatten_workspace_bytes(F), dev, "cnr_mesh_orient_flatten")
    _C.call("cnr_mesh_orient_flatten", words, F, ws, labels, flip0, err)
    mark("flatten")
    roots = _roots(labels, None, F)
    _raise_if_set(err, "orient")
    C = len(roots)
    face_patch = torch.empty(F, device=dev, dtype=torch.int32)
    _C.call("cnr_mesh_assign", labels, None, F, roots, C, face_patch, err)
    mark("roots_assign")
    bad = torch.empty(C, device=dev, dtype=torch.int32)
    counts = torch.empty(C, 2, device=dev, dtype=torch.int32)
    _C.call("cnr_mesh_orient_check", skeys, perm, f, F, face_patch, C, flip0, bad, counts, err)
    mark("check_links")
    spatch, order = torch.sort(face_patch, stable=True)
    mark("sort_faces")
    n_faces = torch.empty(C, device=dev, dtype=torch.int32)
    n_flipped = torch.empty(C, device=dev, dtype=torch.int32)
    sign = torch.empty(C, device=dev, dtype=torch.uint8)
    volume = torch.empty(C, device=dev, dtype=torch.float64) if verts is not None else None
    ws = _C.workspace(_C.load().cnr_mesh_orient_stats_workspace_bytes(F), dev, "cnr_mesh_orient_stats")
    _C.call("cnr_mesh_orient_stats", verts, f, order, spatch, face_patch, F, V, C, flip0, bad, 1 if outward else 0, ws, n_faces,
            n_flipped, sign, volume)
    mark("patch_stats")
    out = torch.empty(F, 3, device=dev, dtype=torch.int32)
    flip = torch.empty(F, device=dev, dtype=torch.uint8)
    _C.call("cnr_mesh_orient_apply", f, F, face_patch, C, flip0, sign, out, flip)
    mark("apply")
    _raise_if_set(err, "orient")
    return MeshOrientation(n=C, faces=out, flip=flip, face_patch=face_patch, first=roots, n_faces=n_faces, orientable=bad == 0,
                           closed=counts[:, 0] == 0, inconsistent_edges=counts[:, 1].contiguous(), n_flipped=n_flipped,
                           signed_volume=volume)


def orient_mesh(mesh, outward=True, device=None):
    """``orient`` on a ``vis.Mesh`` -> (mesh, MeshOrientation): the same vertices and per-vertex attributes, the repaired faces."""
    d = device_mesh(mesh, device, what="orient_mesh")
    out = orient(d.faces, len(d.verts), verts=d.verts, outward=outward)
    return mesh.subset(np.arange(len(d.verts), dtype=np.int64), out.faces.cpu().numpy().astype(np.int64).reshape(-1, 3)), out


def compact(faces, n_vertices, keep_face, reindex=True):
    """The faces with keep_face (F,) set, in their old order, re-indexed to the vertices they use in their old order (the rule of
    raster.cull_mesh) -> (faces (F',3) i32, vertex_map (V,) i32 with -1 = dropped, kept_vertices (V',) i32 ascending); gather
    attributes with ``attr.index_select(0, kept_vertices.long())``.  reindex=False keeps the indices -> faces only."""
    V = int(n_vertices)
    f = check_faces(faces, V, "compact")
    F, dev = f.shape[0], f.device
    if tuple(keep_face.shape) != (F,):
        raise ValueError(f"keep_face must have the shape ({F},), not {tuple(keep_face.shape)}")
    keep = (keep_face != 0).to(torch.uint8).contiguous()
    if F == 0 or V == 0:
        out = torch.zeros(0, 3, device=dev, dtype=torch.int32)
        return (out, torch.full((V,), -1, device=dev, dtype=torch.int32), torch.zeros(0, device=dev, dtype=torch.int32)) if reindex else out
    ws = _C.workspace(_C.load().cnr_mesh_compact_workspace_bytes(F, V), dev, "cnr_mesh_compact")
    cnt = torch.empty(2, device=dev, dtype=torch.int64)
    _C.call("cnr_mesh_compact_count", f, F, V, keep, 1 if reindex else 0, ws, cnt)
    nf, nv = (int(v) for v in cnt.cpu())
    out = torch.empty(nf, 3, device=dev, dtype=torch.int32)
    if nf == 0:                                  # nothing kept: nothing to emit (an empty tensor has no address to hand over)
        return (out, torch.full((V,), -1, device=dev, dtype=torch.int32), torch.zeros(0, device=dev, dtype=torch.int32)) if reindex else out
    if not reindex:
        _C.call("cnr_mesh_compact_emit", f, F, V, keep, 0, ws, out, None, None)
        return out
    vmap = torch.empty(V, device=dev, dtype=torch.int32)
    kept = torch.empty(nv, device=dev, dtype=torch.int32)
    _C.call("cnr_mesh_compact_emit", f, F, V, keep, 1, ws, out, vmap, kept)
    return out, vmap, kept


def _lex_order(rows):
    """the permutation (n,) i64 that puts the rows (n,3) i32 in (column 0, 1, 2) order: three stable sorts, the last column first"""
    perm = torch.arange(len(rows), device=rows.device)
    for axis in (2, 1, 0):
        perm = perm[torch.sort(rows[perm, axis], stable=True)[1]]
    return perm.contiguous()


def _number_runs(rep, err):
    """cnr_weld_runs' representatives (n,) i32 -> (roots (C,) i32 ascending, the number 0 .. C-1 of every element's run (n,) i32)"""
    n = len(rep)
    roots = _roots(rep, None, n)
    number = torch.empty(n, device=rep.device, dtype=torch.int32)
    _C.call("cnr_mesh_assign", rep, None, n, roots, len(roots), number, err)
    return roots, number


def _clusters(verts, cell, err, strict=False, mark=lambda name: None):
    """the cells of cnr_voxel_keys numbered by their lowest vertex (weld's cell > 0, simplify's clusters) -> (min (3,) f32, keys
    (V,) i64, roots (C,) i32, cluster (V,) i32).  strict is simplify's contract: cnr_simplify_check_keys flags a non-finite
    vertex or more than 2^21 cells on an axis, and a set flag raises before the runs are counted; weld takes such rows as they come."""
    V, dev = len(verts), verts.device
    mn = torch.empty(3, device=dev, dtype=torch.float32)
    _C.call("cnr_points_min", verts, V, _C.workspace(_C.load().cnr_points_min_workspace_bytes(V), dev, "cnr_points_min"), mn)
    keys = torch.empty(V, device=dev, dtype=torch.int64)
    _C.call("cnr_voxel_keys", verts, V, mn, float(cell), keys)
    if strict:
        _C.call("cnr_simplify_check_keys", keys, V, err)
    mark("keys")
    skeys, perm = torch.sort(keys, stable=True)
    mark("sort_keys")
    rep = torch.empty(V, device=dev, dtype=torch.int32)
    _C.call("cnr_weld_runs", None, skeys, perm, V, rep, err)
    if strict:
        _raise_if_set(err, "simplify")
    return (mn, keys) + _number_runs(rep, err)


def weld(verts, faces=None, cell=0.0, drop_degenerate=True):
    """Merge coincident vertices.  verts (V,3) f32 with faces (F,3), or faces=None and verts (F,3,3): a triangle soup.
    cell == 0: rows weld when their three fp32 values are bit-equal after -0 -> +0; a row holding a NaN welds with nothing.
    cell > 0: rows weld when they round to the same point of the grid of pitch `cell` anchored at the per-axis minimum, i.e.
    share floor((p - (min - cell / 2)) / cell) per axis (cnr_voxel_keys) -- the rounding-grid semantics of trimesh's
    merge_vertices(digits), on a grid through the minimum instead of the origin; a non-finite row welds with nothing.
    The representative of a set is its lowest input index, representatives are numbered in ascending input order, and a welded
    vertex takes the representative's attributes (no averaging).
    -> (kept_vertices (V',) i32 ascending: gather positions / normals / colours with index_select, faces (F',3) i32, remap (V,)
    i32).  Faces whose corners stop being distinct are dropped unless drop_degenerate=False."""
    if faces is None:
        if verts.dim() != 3 or tuple(verts.shape[1:]) != (3, 3):
            raise ValueError(f"a soup must have the shape (F,3,3), not {tuple(verts.shape)}")
        verts = verts.reshape(-1, 3)
        faces = torch.arange(len(verts), device=verts.device, dtype=torch.int32).view(-1, 3)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must have the shape (V,3), not {tuple(verts.shape)}")
    if not cell >= 0:
        raise ValueError("cell must be >= 0")
    verts = verts.float().contiguous()
    V, dev = len(verts), verts.device
    f = check_faces(faces, V, "weld")
    if V == 0:
        z = torch.zeros(0, device=dev, dtype=torch.int32)
        return z, f, z.clone()
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    if cell == 0:
        rows = (verts + 0.0).view(torch.int32).contiguous()              # -0 + +0 = +0; every other value as it is
        rep = torch.empty(V, device=dev, dtype=torch.int32)
        _C.call("cnr_weld_runs", rows, None, _lex_order(rows), V, rep, err)
        kept, remap = _number_runs(rep, err)
    else:
        _, _, kept, remap = _clusters(verts, cell, err)
    _raise_if_set(err, "weld")
    F = len(f)
    if F == 0:
        return kept, f, remap
    out = torch.empty(F, 3, device=dev, dtype=torch.int32)
    keep = torch.empty(F, device=dev, dtype=torch.uint8)
    _C.call("cnr_mesh_remap_faces", f, F, remap, 1 if drop_degenerate else 0, out, keep)
    if drop_degenerate:
        out = compact(out, len(kept), keep, reindex=False)
    return kept, out, remap


_weld = weld                        # (clean_mesh's options of the same names shadow the functions)
_orient = orient


def select_components(table, keep_largest=None, min_faces=0, min_area=0.0, min_diag=0.0, min_area_fraction=0.0, largest_by="area"):
    """-> keep (n,) bool on the host: the components that pass every threshold (>=: a value exactly on it is kept) and, with
    keep_largest = k, are among the k largest of those by `largest_by` ("area", "faces" or "diag"; ties go to the lower
    component id).  Never empty unless the table is: when nothing passes, the single largest component is kept."""
    if largest_by not in LARGEST_BY:
        raise ValueError(f"largest_by must be one of {LARGEST_BY}, not {largest_by!r}")
    if keep_largest is not None and int(keep_largest) < 1:
        raise ValueError("keep_largest must be at least 1")
    n = table.n
    if n == 0:
        return np.zeros(0, bool)
    n_faces = table.n_faces.cpu().numpy().astype(np.int64)
    needs_geometry = min_area > 0 or min_diag > 0 or min_area_fraction > 0 or largest_by != "faces"
    if needs_geometry and table.area is None:
        raise ValueError("area and diagonal thresholds need a table built with verts")
    area = table.area.cpu().numpy() if table.area is not None else None
    diag = table.diag.cpu().numpy() if table.diag is not None else None
    ok = n_faces >= int(min_faces)
    if min_area > 0:
        ok &= area >= float(min_area)
    if min_diag > 0:
        ok &= diag >= float(min_diag)
    if min_area_fraction > 0:
        ok &= area >= float(min_area_fraction) * float(area.sum())
    size = {"area": area, "faces": n_faces, "diag": diag}[largest_by]
    rank = np.lexsort((np.arange(n), -np.asarray(size, np.float64)))          # largest first, the lower id first among equals
    if not ok.any():
        ok = np.zeros(n, bool)
        ok[rank[0]] = True
    elif keep_largest is not None:
        best = [c for c in rank if ok[c]][:int(keep_largest)]
        ok = np.zeros(n, bool)
        ok[best] = True
    return ok


def clean_device(verts, faces, weld=None, connectivity="edge", keep_largest=None, min_faces=0, min_area=0.0, min_diag=0.0,
                 min_area_fraction=0.0, largest_by="area", orient=False):
    """clean_mesh on device tensors: verts (V,3) f32, faces (F,3) i32 -> (faces (F',3) i32 re-indexed, kept_vertices (V',) i32
    into the INPUT vertices, report).  weld: None (no welding), 0.0 (exact) or a cell size.  orient=True runs
    ``orient(..., outward=True)`` on what the component filter kept; report["orientation"] is its MeshOrientation."""
    V = len(verts)
    verts = verts.float().contiguous()
    f = check_faces(faces, V, "clean_mesh")
    kept0 = None
    if weld is not None:
        kept0, f, _ = _weld(verts, f, cell=float(weld))
        verts = verts.index_select(0, kept0.long())
    table = components(f, len(verts), verts=verts, connectivity=connectivity)
    keep_c = select_components(table, keep_largest, min_faces, min_area, min_diag, min_area_fraction, largest_by)
    report = dict(components=table, kept=keep_c, n_components=table.n, n_kept=int(keep_c.sum()), faces_in=int(len(faces)),
                  vertices_in=int(V))
    if table.n == 0:
        out_f, kept = f, torch.zeros(0, device=f.device, dtype=torch.int32)
    else:
        keep_face = torch.from_numpy(keep_c).to(f.device)[table.face_component.long()]
        out_f, _, kept = compact(f, len(verts), keep_face)
    if orient:
        report["orientation"] = _orient(out_f, len(kept), verts=verts.index_select(0, kept.long()), outward=True)
        out_f = report["orientation"].faces
    if kept0 is not None:
        kept = kept0.index_select(0, kept.long())
    report.update(faces_out=int(len(out_f)), vertices_out=int(len(kept)))
    return out_f, kept, report


def clean_mesh(mesh, weld=None, connectivity="edge", keep_largest=None, min_faces=0, min_area=0.0, min_diag=0.0,
               min_area_fraction=0.0, largest_by="area", device=None, orient=False):
    """A ``vis.Mesh`` without its floaters -> (mesh, report).  Optionally weld first (None / 0.0 = exact / cell size), split into
    components by `connectivity`, keep those with n_faces >= min_faces, area >= min_area, bounding-box diagonal >= min_diag and
    area >= min_area_fraction x the total area, and of those the keep_largest largest by `largest_by`; ties go to the lower
    component id, and the result is never empty unless the input is.  Positions, normals and colours of the kept vertices are
    the input's (float64 positions stay float64: the device sees their fp32 roundings, the output gathers the originals).
    orient=True then repairs the orientation of what is left (``orient``, outward patches).
    report: dict(components=MeshComponents, kept=(n,) bool, n_components, n_kept, faces_in/out, vertices_in/out[, orientation])."""
    d = device_mesh(mesh, device, what="clean_mesh")
    out_f, kept, report = clean_device(d.verts, d.faces, weld, connectivity, keep_largest, min_faces, min_area, min_diag,
                                       min_area_fraction, largest_by, orient)
    return mesh.subset(kept.cpu().numpy().astype(np.int64), out_f.cpu().numpy().astype(np.int64).reshape(-1, 3)), report


def _parse_options(text, kinds, flag):
    """a tool's "name=value,name=value" string -> the dict of options, each value read by kinds[name]"""
    out = {}
    for item in (text or "").split(","):
        if not item.strip():
            continue
        k, _, v = item.partition("=")
        k = k.strip()
        if k not in kinds or not v.strip():
            raise ValueError(f"{flag}: cannot read {item!r}; options are {sorted(kinds)} as name=value")
        out[k] = kinds[k](v.strip())
    return out


def _flag(text):
    if text.lower() in ("1", "true", "yes"):
        return True
    if text.lower() in ("0", "false", "no"):
        return False
    raise ValueError(f"cannot read {text!r} as a flag (1 / 0)")


def parse_clean_options(text):
    """the tools' ``--clean`` string, e.g. "keep_largest=1,min_faces=20,weld=0" -> the dict of clean_mesh options"""
    return _parse_options(text, dict(weld=float, connectivity=str, keep_largest=int, min_faces=int, min_area=float, min_diag=float,
                                     min_area_fraction=float, largest_by=str, orient=_flag), "--clean")


# ---- simplification: uniform vertex clustering with quadric placement (csrc/mesh_simplify.hip) -------
PLACEMENT = ("quadric", "mean", "representative")
SEARCH_TRIALS = 24
TOTAL_BLOCK = 256


def _segment_sum(items, gather, gather_div, sorted_seg, C, err):
    """(C,K) f64: cnr_segment_sum_f64 of items (n,K) f64 over the positions of sorted_seg (N,) i32, ascending"""
    K, N = items.shape[1], len(sorted_seg)
    out = torch.empty(C, K, device=items.device, dtype=torch.float64)
    _C.call("cnr_segment_sum_f64", items, gather, int(gather_div), sorted_seg, N, len(items), K, C, out, err)
    return out


def _fixed_order_total(values, err):
    """the sum of values (n,) f64 in an order fixed by n alone: cnr_segment_sum_f64 over blocks of TOTAL_BLOCK consecutive values,
    again over the blocks' sums while more than TOTAL_BLOCK are left, then over what is left as one segment -> (1,) f64"""
    dev = values.device
    while len(values) > TOTAL_BLOCK:
        n = len(values)
        seg = (torch.arange(n, device=dev) // TOTAL_BLOCK).to(torch.int32)
        values = _segment_sum(values.view(n, 1), None, 1, seg, -(-n // TOTAL_BLOCK), err).view(-1)
    return _segment_sum(values.view(len(values), 1), None, 1, torch.zeros(len(values), device=dev, dtype=torch.int32), 1, err).view(-1)


def _cluster_faces(f, cluster, C, err, mark=lambda name: None):
    """-> (corner clusters (F,3) i32 of EVERY input face, the faces with three distinct clusters (F1,3) i32 in their old order,
    keep (F1,) u8 = 1 for the lowest face of every run of equal rows).  Rows: the face rotated so that its smallest index leads;
    (a, c, b) is another row than (a, b, c)."""
    F, dev = len(f), f.device
    corners = torch.empty(F, 3, device=dev, dtype=torch.int32)
    keep = torch.empty(F, device=dev, dtype=torch.uint8)
    _C.call("cnr_mesh_remap_faces", f, F, cluster, 1, corners, keep)
    f1 = compact(corners, C, keep, reindex=False)
    mark("remap")
    F1 = len(f1)
    if F1 == 0:
        return corners, f1, torch.zeros(0, device=dev, dtype=torch.uint8)
    rows = torch.empty(F1, 3, device=dev, dtype=torch.int32)
    _C.call("cnr_simplify_face_rows", f1, F1, rows)
    mark("face_rows")
    perm = _lex_order(rows)                                              # as weld's exact mode
    mark("sort_rows")
    rep = torch.empty(F1, device=dev, dtype=torch.int32)
    _C.call("cnr_weld_runs", rows, None, perm, F1, rep, err)
    keep1 = (rep == torch.arange(F1, device=dev, dtype=torch.int32)).to(torch.uint8)
    mark("duplicates")
    return corners, f1, keep1


def _faces_out(verts, f, cell):
    """the integer stages only: the number of faces simplify(cell) returns"""
    err = torch.zeros(1, device=verts.device, dtype=torch.int32)
    _, _, roots, cluster = _clusters(verts, cell, err, strict=True)
    _, _, keep1 = _cluster_faces(f, cluster, len(roots), err)
    _raise_if_set(err, "simplify")
    return int(keep1.sum().item()) if len(keep1) else 0


def search_cell(target_faces, diag, faces_out):
    """Bisection of the cell size on the host, in its logarithm, between diag and diag / 2^20, at most SEARCH_TRIALS calls of
    faces_out(cell) -> (cell, [(cell, faces_out), ...]): the finest cell tried whose faces_out <= target_faces."""
    target = int(target_faces)
    if target < 0:
        raise ValueError("target_faces must be >= 0")
    if not (diag > 0 and np.isfinite(diag)):
        raise ValueError("target_faces needs a bounding box with a finite, positive diagonal")
    trials = []

    def run(cell):
        trials.append((cell, int(faces_out(cell))))
        return trials[-1][1]
    hi, lo = float(diag), float(diag) / 2.0 ** 20
    if run(hi) > target:
        raise ValueError(f"target_faces={target}: even a cell of the bounding-box diagonal leaves {trials[-1][1]} faces")
    if run(lo) > target:
        while len(trials) < SEARCH_TRIALS:
            mid = float(np.sqrt(lo * hi))
            if not lo < mid < hi:
                break
            if run(mid) <= target:
                hi = mid
            else:
                lo = mid
    return min(c for c, n in trials if n <= target), trials


def _bbox_diag(verts):
    lo, hi = verts.amin(0).double().cpu().numpy(), verts.amax(0).double().cpu().numpy()
    d = hi - lo
    return float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def simplify(verts, faces, cell=None, target_faces=None, placement="quadric", tau=1e-3, details=False, timer=None):
    """Uniform vertex clustering with quadric placement (Lindstrom 2000; the quadrics per corner, as open3d's
    simplify_vertex_clustering).  verts (V,3) f32, faces (F,3) on the device -> (verts' (V',3) f32, faces' (F',3) i32,
    vertex_map (V,) i32: the output vertex of every input vertex or -1, report).

    The clusters are the cells of the grid of pitch `cell` through min - cell / 2 (weld's), numbered by their lowest input
    vertex.  Every input face adds its plane quadric, weighted by its squared area, to the cluster of each of its corners.
    placement: "quadric" = the minimiser of the cluster's quadric about the cluster mean, eigenvalues <= tau x the largest
    dropped, clamped per axis to the cluster's cell; "mean" = the mean of the cluster's vertices; "representative" = the
    lowest input vertex, bit-exact (weld's choice).  Faces with fewer than three distinct clusters are dropped, then every face
    that repeats an earlier one (the same three clusters in the same cyclic order; the opposite orientation is another face);
    clusters no face uses are dropped last.  A surviving face keeps its corner order.
    Exactly one of cell and target_faces: target_faces bisects the cell on the host (search_cell) over the integer stages.
    report: cell, clusters, faces_in, faces_collapsed, faces_duplicate, faces_out, vertices_out, clamped (clusters the clamp
    moved), quadric_error (the clusters' errors x^T A x - 2 b^T x + c summed in a fixed order: _fixed_order_total), search
    [(cell, faces_out), ...], representatives (V',) i32 = the lowest input vertex of every output vertex's cluster; with
    details=True also cluster (V,) i32, roots (C,), quadrics (C,10), possum (C,3), cluster_error (C,), cluster_clamped (C,),
    cluster_verts (C,3), kept_clusters (V',).  A non-finite vertex or more than 2^21 cells on an axis raises ValueError."""
    if placement not in PLACEMENT:
        raise ValueError(f"placement must be one of {PLACEMENT}, not {placement!r}")
    if (cell is None) == (target_faces is None):
        raise ValueError("give exactly one of cell and target_faces")
    if cell is not None and not (float(cell) > 0 and np.isfinite(float(cell))):
        raise ValueError("cell must be > 0")
    if not 0 <= float(tau) < 1:
        raise ValueError("tau must lie in [0, 1)")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must have the shape (V,3), not {tuple(verts.shape)}")
    verts = verts.float().contiguous()
    V, dev = len(verts), verts.device
    f = check_faces(faces, V, "simplify")
    F = len(f)
    if V > 0x7f800000:
        raise ValueError("simplify: V must stay below 2^31 - 2^23 (the face rows are compared as cnr_weld_runs compares rows)")
    mark = timer or (lambda name: None)
    z32 = torch.zeros(0, device=dev, dtype=torch.int32)
    report = dict(cell=None if cell is None else float(cell), clusters=0, faces_in=F, faces_collapsed=0, faces_duplicate=0,
                  faces_out=0, vertices_out=0, clamped=0, quadric_error=0.0, search=[], representatives=z32)

    def empty():
        return (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev, dtype=torch.int32),
                torch.full((V,), -1, device=dev, dtype=torch.int32), report)
    if F == 0 or V == 0:
        return empty()
    if cell is None:
        cell, report["search"] = search_cell(target_faces, _bbox_diag(verts), lambda c: _faces_out(verts, f, c))
        report["cell"] = cell
    cell = float(cell)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    mn, keys, roots, cluster = _clusters(verts, cell, err, strict=True, mark=mark)
    C = len(roots)
    mark("cluster_ids")
    corners, f1, keep1 = _cluster_faces(f, cluster, C, err, mark)
    _raise_if_set(err, "simplify")
    F1 = len(f1)
    report.update(clusters=C, faces_collapsed=F - F1)
    if details:
        report.update(cluster=cluster, roots=roots, keys=keys, min=mn)
    if F1 == 0:
        return empty()
    out_f, cmap, kept_c = compact(f1, C, keep1)
    mark("compact")
    # the fp64 part: every input face's record to the cluster of each corner, the clusters' position sums, the placement
    records = torch.empty(F, 10, device=dev, dtype=torch.float64)
    _C.call("cnr_simplify_face_records", verts, f, mn, F, V, records, err)
    mark("records")
    sseg, cperm = torch.sort(corners.view(-1), stable=True)
    mark("sort_corners")
    quadrics = _segment_sum(records, cperm, 3, sseg, C, err)
    mark("sum_quadrics")
    possum = sclu = None
    if placement != "representative":
        q = torch.empty(V, 3, device=dev, dtype=torch.float64)
        _C.call("cnr_simplify_vertex_q", verts, mn, V, q)
        sclu, vperm = torch.sort(cluster, stable=True)
        mark("sort_vertices")
        possum = _segment_sum(q, vperm, 1, sclu, C, err)
        mark("sum_positions")
    placed = torch.empty(C, 3, device=dev, dtype=torch.float32)
    cerr = torch.empty(C, device=dev, dtype=torch.float64)
    clamped = torch.empty(C, device=dev, dtype=torch.uint8)
    _C.call("cnr_simplify_place", quadrics, possum, sclu, verts, roots, keys, mn, V, C, cell, float(tau), PLACEMENT.index(placement),
            placed, cerr, clamped, err)
    mark("place")
    total = _fixed_order_total(cerr, err)
    mark("total_error")
    _raise_if_set(err, "simplify")
    out_v = placed.index_select(0, kept_c.long())
    vertex_map = cmap.index_select(0, cluster.long())
    mark("gather")
    report.update(faces_duplicate=F1 - len(out_f), faces_out=len(out_f), vertices_out=len(kept_c), clamped=int(clamped.sum().item()),
                  quadric_error=float(total.item()), representatives=roots.index_select(0, kept_c.long()))
    if details:
        report.update(quadrics=quadrics, possum=possum, cluster_error=cerr, cluster_clamped=clamped, cluster_verts=placed,
                      kept_clusters=kept_c)
    return out_v, out_f, vertex_map, report


def vertex_normals(verts, faces):
    """(V,3) f32: the normalised sum of (p1 - p0) x (p2 - p0) over the faces at each vertex (area-weighted), summed in fp64 in
    cnr_segment_sum_f64's order over the corners sorted stably by vertex.  By vis.py's orientation convention it points to the
    side the marching-cubes normals point to.  A vertex no face uses, or whose sum is zero, gets zeros."""
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"verts must have the shape (V,3), not {tuple(verts.shape)}")
    verts = verts.float().contiguous()
    V, dev = len(verts), verts.device
    f = check_faces(faces, V, "vertex_normals")
    F = len(f)
    out = torch.zeros(V, 3, device=dev, dtype=torch.float32)
    if F == 0 or V == 0:
        return out
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    fn = torch.empty(F, 3, device=dev, dtype=torch.float64)
    _C.call("cnr_mesh_face_normals_f64", verts, f, F, V, fn, err)
    sseg, perm = torch.sort(f.view(-1), stable=True)
    sums = _segment_sum(fn, perm, 3, sseg, V, err)
    _raise_if_set(err, "vertex_normals")
    _C.call("cnr_mesh_normals_finish", sums, V, out)
    return out


def simplify_mesh(mesh, cell=None, target_faces=None, placement="quadric", tau=1e-3, device=None):
    """``simplify`` of a ``vis.Mesh`` -> (mesh, report).  Positions are the device result as float64; the colour of an output
    vertex is its cluster representative's (the lowest input index, as weld: no averaging); normals are ``vertex_normals`` of
    the output."""
    d = device_mesh(mesh, device, what="simplify_mesh")
    v, f, _, report = simplify(d.verts, d.faces, cell=cell, target_faces=target_faces, placement=placement, tau=tau)
    out = Mesh(v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64).reshape(-1, 3),
               vertex_normals(v, f).cpu().numpy().astype(np.float64))
    out.visual.vertex_colors = mesh.visual.vertex_colors[report["representatives"].cpu().numpy().astype(np.int64)]
    return out, report


# ---- deviation between two meshes (csrc/point_mesh.hip) ---------------------------------------------------
def _one_sided(mesh, other, samples, rng, include_vertices, index=False):
    """the distances from one DeviceMesh's vertices and samples to the surface of the other -> dict(mean, rms, max, n)"""
    from . import metrics
    parts = []
    if include_vertices:
        parts.append(mesh.verts.index_select(0, torch.unique(mesh.faces.view(-1).long())))
    if samples > 0:
        parts.append(metrics.sample_surface(mesh, samples, rng))
    if not parts:
        raise ValueError("deviation: nothing to measure (samples=0 and include_vertices=False)")
    q = torch.cat(parts).contiguous()
    d, _ = metrics.point_mesh_distance(q, other, check=False, index=bool(index))
    n = len(d)
    total, _ = metrics.dist_stats(d)
    d64 = d.double()
    return dict(mean=total / n, rms=float(torch.sqrt((d64 * d64).sum() / n)), max=float(d.max()), n=n)


def deviation(verts_a, faces_a, verts_b, faces_b, samples=100000, seed=0, include_vertices=True, index=False):
    """Two-sided Metro-style deviation of two meshes on the device (verts (V,3) f32, faces (F,3)): the vertices of A that its
    faces use (when include_vertices) and `samples` area-weighted samples of A, each measured against the surface of B by the
    exact point-to-mesh distance (metrics.point_mesh_distance), and the same from B to A.  The samples come from
    numpy.random.default_rng(seed), A's first; samples=0 measures the vertices only.  index=True takes the distances through a
    metrics.MeshIndex of each mesh: the same numbers from fewer pairs.
    -> {"a_to_b": {mean, rms, max, n}, "b_to_a": {...}, "hausdorff": the larger max, "diag": the bounding-box diagonal of A}"""
    sides = []
    for v, f, name in ((verts_a, faces_a, "A"), (verts_b, faces_b, "B")):
        if v.dim() != 2 or v.shape[1] != 3:
            raise ValueError(f"verts must have the shape (V,3), not {tuple(v.shape)}")
        v = v.float().contiguous()
        require_finite(v, "deviation")
        m = DeviceMesh(v, check_faces(f, len(v), "deviation"))
        if m.n_faces == 0:
            raise ValueError(f"deviation: mesh {name} has no faces")
        sides.append(m)
    rng = np.random.default_rng(seed)
    a, b = sides
    a_to_b = _one_sided(a, b, int(samples), rng, include_vertices, index)
    b_to_a = _one_sided(b, a, int(samples), rng, include_vertices, index)
    return dict(a_to_b=a_to_b, b_to_a=b_to_a, hausdorff=max(a_to_b["max"], b_to_a["max"]), diag=_bbox_diag(a.verts))


def deviation_mesh(mesh_a, mesh_b, samples=100000, seed=0, include_vertices=True, device=None, index=False):
    """``deviation`` of two ``vis.Mesh``"""
    a, b = (device_mesh(m, device, what="deviation_mesh") for m in (mesh_a, mesh_b))
    return deviation(a.verts, a.faces, b.verts, b.faces, samples=samples, seed=seed, include_vertices=include_vertices, index=index)


def parse_simplify_options(text):
    """the tools' ``--simplify`` string, e.g. "cell=0.02,placement=mean" or "target_faces=20000" -> the dict of simplify options"""
    return _parse_options(text, dict(cell=float, target_faces=int, placement=str, tau=float), "--simplify")
