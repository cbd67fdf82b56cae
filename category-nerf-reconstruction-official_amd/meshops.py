"""The mesh as a graph, on the device (csrc/mesh_topo.hip): welding of coincident vertices, connected
components by edge or by vertex with their table (faces, vertices, area, bounding box, boundary / non-manifold edges,
watertightness), compaction of a face selection, and ``clean_mesh``: dropping the floaters of a marching-cubes mesh.

Device tensors in and out (``clean_mesh`` and ``mesh_to_device`` take a host ``vis.Mesh``).  The sorts are
``torch.sort(stable=True)``, every other step is a HIP kernel; there is no CPU path.  A union/find loop that runs out of its bound
raises CnrError, an out-of-range face index raises ValueError."""
import numpy as np
import torch

from . import _C
from .vis import Mesh

CONNECTIVITY = ("edge", "vertex")
LARGEST_BY = ("area", "faces", "diag")


def _raise_if_set(err, what):
    e = int(err.item())
    if e & 2:
        raise ValueError(f"{what}: an index lies outside its range")
    if e & 1:
        raise _C.CnrError(f"{what}: a union/find loop ran out of its bound (the label array is corrupt)")


def _faces_i32(faces, n_vertices, what):
    """(F,3) device faces -> contiguous int32, range-checked on the device against [0, n_vertices)"""
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must have the shape (F,3), not {tuple(faces.shape)}")
    if not faces.is_cuda:
        raise _C.CnrError(f"{what}: cnr kernels take device tensors only; there is no CPU path")
    n_vertices = int(n_vertices)
    F = faces.shape[0]
    if n_vertices < 0 or n_vertices > 2 ** 31 - 1 or 3 * F > 2 ** 31 - 1:
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
        _raise_if_set(err, what)
    return f


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
    f = _faces_i32(faces, V, "components")
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
    if connectivity == "edge":
        labels = torch.empty(F, device=dev, dtype=torch.int32)
        _C.call("cnr_mesh_labels_init", labels, F)
        _C.call("cnr_mesh_union_edges", skeys, perm, F, labels, err)
        mark("union")
        _flatten(labels, F, err)
        mark("flatten")
        roots = _roots(labels, None, F)
        _raise_if_set(err, "components")
        _C.call("cnr_mesh_assign", labels, None, F, roots, len(roots), face_comp, err)
        _C.call("cnr_mesh_cross_component", f, F, V, 0, face_comp, vert_comp)
    else:
        labels = torch.empty(V, device=dev, dtype=torch.int32)
        used = torch.zeros(V, device=dev, dtype=torch.uint8)
        _C.call("cnr_mesh_labels_init", labels, V)
        _C.call("cnr_mesh_union_faces", f, F, V, labels, used, err)
        mark("union")
        _flatten(labels, V, err)
        mark("flatten")
        roots = _roots(labels, used, V)
        _raise_if_set(err, "components")
        _C.call("cnr_mesh_assign", labels, used, V, roots, len(roots), vert_comp, err)
        _C.call("cnr_mesh_cross_component", f, F, V, 1, face_comp, vert_comp)
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


def compact(faces, n_vertices, keep_face, reindex=True):
    """The faces with keep_face (F,) set, in their old order, re-indexed to the vertices they use in their old order (the rule of
    raster.cull_mesh) -> (faces (F',3) i32, vertex_map (V,) i32 with -1 = dropped, kept_vertices (V',) i32 ascending); gather
    attributes with ``attr.index_select(0, kept_vertices.long())``.  reindex=False keeps the indices -> faces only."""
    V = int(n_vertices)
    f = _faces_i32(faces, V, "compact")
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
    f = _faces_i32(faces, V, "weld")
    if V == 0:
        z = torch.zeros(0, device=dev, dtype=torch.int32)
        return z, f, z.clone()
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    rep = torch.empty(V, device=dev, dtype=torch.int32)
    if cell == 0:
        rows = (verts + 0.0).view(torch.int32).contiguous()              # -0 + +0 = +0; every other value as it is
        perm = torch.arange(V, device=dev)
        for axis in (2, 1, 0):                                           # three stable sorts: rows in (x, y, z) order
            perm = perm[torch.sort(rows[perm, axis], stable=True)[1]]
        _C.call("cnr_weld_runs", rows, None, perm.contiguous(), V, rep, err)
    else:
        lib = _C.load()
        mn = torch.empty(3, device=dev, dtype=torch.float32)
        _C.call("cnr_points_min", verts, V, _C.workspace(lib.cnr_points_min_workspace_bytes(V), dev, "cnr_points_min"), mn)
        keys = torch.empty(V, device=dev, dtype=torch.int64)
        _C.call("cnr_voxel_keys", verts, V, mn, float(cell), keys)
        skeys, perm = torch.sort(keys, stable=True)
        _C.call("cnr_weld_runs", None, skeys, perm, V, rep, err)
    kept = _roots(rep, None, V)
    remap = torch.empty(V, device=dev, dtype=torch.int32)
    _C.call("cnr_mesh_assign", rep, None, V, kept, len(kept), remap, err)
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


_weld = weld                        # (clean_mesh's option of the same name shadows the function)


# ---- vis.Mesh on the device ------------------------------------------------------------------------------------------------
def mesh_to_device(mesh, device=None):
    """vis.Mesh -> dict(verts (V,3) f32, faces (F,3) i32) on the device (positions rounded to fp32 once)"""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return dict(verts=torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float32)).to(dev),
                faces=torch.from_numpy(np.ascontiguousarray(mesh.faces, np.int32)).to(dev))


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
                 min_area_fraction=0.0, largest_by="area"):
    """clean_mesh on device tensors: verts (V,3) f32, faces (F,3) i32 -> (faces (F',3) i32 re-indexed, kept_vertices (V',) i32
    into the INPUT vertices, report).  weld: None (no welding), 0.0 (exact) or a cell size."""
    V = len(verts)
    verts = verts.float().contiguous()
    f = _faces_i32(faces, V, "clean_mesh")
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
    if kept0 is not None:
        kept = kept0.index_select(0, kept.long())
    report.update(faces_out=int(len(out_f)), vertices_out=int(len(kept)))
    return out_f, kept, report


def clean_mesh(mesh, weld=None, connectivity="edge", keep_largest=None, min_faces=0, min_area=0.0, min_diag=0.0,
               min_area_fraction=0.0, largest_by="area", device=None):
    """A ``vis.Mesh`` without its floaters -> (mesh, report).  Optionally weld first (None / 0.0 = exact / cell size), split into
    components by `connectivity`, keep those with n_faces >= min_faces, area >= min_area, bounding-box diagonal >= min_diag and
    area >= min_area_fraction x the total area, and of those the keep_largest largest by `largest_by`; ties go to the lower
    component id, and the result is never empty unless the input is.  Positions, normals and colours of the kept vertices are
    the input's (float64 positions stay float64: the device sees their fp32 roundings, the output gathers the originals).
    report: dict(components=MeshComponents, kept=(n,) bool, n_components, n_kept, faces_in/out, vertices_in/out)."""
    d = mesh_to_device(mesh, device)
    out_f, kept, report = clean_device(d["verts"], d["faces"], weld, connectivity, keep_largest, min_faces, min_area, min_diag,
                                       min_area_fraction, largest_by)
    idx = kept.cpu().numpy().astype(np.int64)
    out = Mesh(mesh.vertices[idx], out_f.cpu().numpy().astype(np.int64).reshape(-1, 3), mesh.vertex_normals[idx])
    out.visual.vertex_colors = mesh.visual.vertex_colors[idx]
    return out, report


def parse_clean_options(text):
    """the tools' ``--clean`` string, e.g. "keep_largest=1,min_faces=20,weld=0" -> the dict of clean_mesh options"""
    kinds = dict(weld=float, connectivity=str, keep_largest=int, min_faces=int, min_area=float, min_diag=float,
                 min_area_fraction=float, largest_by=str)
    out = {}
    for item in (text or "").split(","):
        if not item.strip():
            continue
        k, _, v = item.partition("=")
        k = k.strip()
        if k not in kinds or not v.strip():
            raise ValueError(f"--clean: cannot read {item!r}; options are {sorted(kinds)} as name=value")
        out[k] = kinds[k](v.strip())
    return out
