"""Numpy restatement of the mesh clean-up contracts (csrc/mesh_topo.hip, cnr_amd.meshops): labels as the
minimum of every scipy connected component, the component table in the kernel's order of operations, edge statistics,
compaction and the welding rules -- plus the fixtures of the host and GPU tests and a brute-force breadth-first labelling."""
import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components as scipy_cc


# ---- labels ----------------------------------------------------------------------------------------------------------------
def labels_from_pairs(pairs, n):
    """labels (n,) int32: the smallest element of every set of the partition the pairs generate"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    g = sp.coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, lab = scipy_cc(g, directed=False)
    mins = np.full(lab.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(mins, lab, np.arange(n))
    return mins[lab].astype(np.int32)


def labels_bfs(pairs, n):
    """the same by a breadth-first search over adjacency lists, element by element in ascending order"""
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(pairs, np.int64).reshape(-1, 2):
        adj[a].append(b)
        adj[b].append(a)
    lab = np.full(n, -1, np.int32)
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = s
        queue = [s]
        while queue:
            nxt = []
            for q in queue:
                for r in adj[q]:
                    if lab[r] < 0:
                        lab[r] = s
                        nxt.append(r)
            queue = nxt
    return lab


def edge_keys(faces):
    """(3F,) int64: slot 3 f + k = the edge of corners k, (k + 1) % 3 as min << 32 | max, -1 when they are equal"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f, np.roll(f, -1, axis=1)
    k = (np.minimum(a, b) << 32) | np.maximum(a, b)
    return np.where(a == b, -1, k).reshape(-1)


def vertex_pairs(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [0, 2]]])


def edge_pairs(faces):
    """face pairs that share an edge: neighbours in the stable sort of the edge keys"""
    keys = edge_keys(faces)
    perm = np.argsort(keys, kind="stable")
    sk = keys[perm]
    j = np.nonzero((sk[1:] == sk[:-1]) & (sk[1:] >= 0))[0] + 1
    return np.stack([perm[j] // 3, perm[j - 1] // 3], 1)


# ---- the component table -----------------------------------------------------------------------------------------------------
def face_areas(verts, faces):
    """fp64 from the fp32 corners: 0.5 sqrt((cx cx + cy cy) + cz cz), c = (p1 - p0) x (p2 - p0), no fused multiply-add"""
    p = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    u, v = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def _lane_tree(a, op):
    """(64, ...) -> the fixed tree of lane distances 32, 16, .., 1 as lane 0 sees it"""
    for d in (32, 16, 8, 4, 2, 1):
        a = op(a[:d], a[d:2 * d])
    return a[0]


def wave_sum(values):
    """the kernel's sum of one run: lane l adds positions l, l + 64, ... in ascending order from 0.0, then the lane tree"""
    values = np.asarray(values, np.float64)
    rows = -(-len(values) // 64)
    pad = np.zeros(rows * 64)
    pad[:len(values)] = values
    acc = np.zeros(64)
    for r in pad.reshape(rows, 64):
        acc = acc + r                    # (a lane past the end of the last row adds nothing in the kernel: + 0.0 is the same)
    return _lane_tree(acc, np.add)


def components(faces, n_vertices, verts=None, connectivity="edge"):
    """dict of numpy arrays with the fields of meshops.MeshComponents"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F, V = len(f), int(n_vertices)
    if F == 0:
        return dict(n=0, face_component=np.zeros(0, np.int32), vertex_component=np.full(V, -1, np.int32), first=np.zeros(0, np.int32),
                    n_faces=np.zeros(0, np.int32), n_vertices=np.zeros(0, np.int32), edge_counts=np.zeros((0, 3), np.int32),
                    boundary_edges=0, nonmanifold_edges=0, watertight=np.zeros(0, bool))
    if connectivity == "edge":
        lab = labels_from_pairs(edge_pairs(f), F)
        first = np.unique(lab)
        face_c = np.searchsorted(first, lab).astype(np.int32)
        vert_c = np.full(V, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(vert_c, f.reshape(-1), np.repeat(face_c, 3))
        vert_c = np.where(vert_c == np.iinfo(np.int64).max, -1, vert_c).astype(np.int32)
    else:
        lab = labels_from_pairs(vertex_pairs(f), V)
        used = np.zeros(V, bool)
        used[f.reshape(-1)] = True
        first = np.unique(lab[used])
        vert_c = np.where(used, np.searchsorted(first, lab), -1).astype(np.int32)
        face_c = vert_c[f[:, 0]]
    C = len(first)
    out = dict(n=C, face_component=face_c, vertex_component=vert_c, first=first.astype(np.int32), labels=lab,
               n_faces=np.bincount(face_c, minlength=C).astype(np.int32),
               n_vertices=np.bincount(vert_c[vert_c >= 0], minlength=C).astype(np.int32))
    # edge statistics
    keys = edge_keys(f)
    perm = np.argsort(keys, kind="stable")
    sk = keys[perm]
    head = np.nonzero((sk >= 0) & np.concatenate([[True], sk[1:] != sk[:-1]]))[0]
    ends = np.searchsorted(sk, sk[head], side="right")
    mult = ends - head
    comp = face_c[perm[head] // 3]
    asc = (f.reshape(-1) < np.roll(f, -1, axis=1).reshape(-1))[perm]
    two = head[mult == 2]
    same = np.zeros(len(head), bool)
    same[mult == 2] = asc[two] == asc[two + 1]
    ec = np.zeros((C, 3), np.int32)
    np.add.at(ec[:, 0], comp[mult == 1], 1)
    np.add.at(ec[:, 1], comp[mult > 2], 1)
    np.add.at(ec[:, 2], comp[same], 1)
    out.update(edge_counts=ec, boundary_edges=int(ec[:, 0].sum()), nonmanifold_edges=int(ec[:, 1].sum()), watertight=(ec == 0).all(1))
    if verts is not None:
        v32 = np.asarray(verts, np.float32)
        areas = face_areas(v32, f)
        order = np.argsort(face_c, kind="stable")
        starts = np.searchsorted(face_c[order], np.arange(C + 1))
        area = np.zeros(C)
        bmin, bmax = np.zeros((C, 3), np.float32), np.zeros((C, 3), np.float32)
        for c in range(C):
            run = order[starts[c]:starts[c + 1]]
            area[c] = wave_sum(areas[run])
            p = v32[f[run]].reshape(-1, 3)
            bmin[c], bmax[c] = np.fmin.reduce(p, 0), np.fmax.reduce(p, 0)        # exact, so any order
        d = bmax.astype(np.float64) - bmin.astype(np.float64)
        out.update(area=area, bbox_min=bmin, bbox_max=bmax, diag=np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    return out


def fsum_area(verts, faces, face_component, c):
    return math.fsum(face_areas(verts, faces)[np.asarray(face_component) == c])


# ---- compaction --------------------------------------------------------------------------------------------------------------
def compact(faces, n_vertices, keep):
    f = np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(keep, bool)]
    used = np.unique(f)
    vmap = np.full(n_vertices, -1, np.int32)
    vmap[used] = np.arange(len(used))
    return vmap[f].reshape(-1, 3).astype(np.int32), vmap, used.astype(np.int32)


# ---- welding -----------------------------------------------------------------------------------------------------------------
def voxel_keys(verts, cell):
    """cnr_voxel_keys: floor((p - (min - cell / 2)) / cell) per axis in fp64, 21 bits per axis, -1 outside / non-finite;
    also the smallest distance, in cells, of any finite coordinate to a cell boundary"""
    p = np.asarray(verts, np.float32)
    with np.errstate(invalid="ignore"):
        mn = np.fmin.reduce(p, 0).astype(np.float64) - cell * 0.5
        q = (p.astype(np.float64) - mn) / cell
        i = np.floor(q)
        ok = ((i >= 0) & (i < 2 ** 21)).all(1)
        frac = (q - i)[ok]
    ii = np.where(ok[:, None], i, 0).astype(np.int64)
    keys = np.where(ok, (ii[:, 0] << 42) | (ii[:, 1] << 21) | ii[:, 2], -1)
    margin = float(np.minimum(frac, 1 - frac).min()) if ok.any() else np.inf
    return keys, margin


def weld(verts, faces=None, cell=0.0, drop_degenerate=True):
    """-> (kept_vertices, faces, remap[, margin]) by the rules of meshops.weld"""
    v = np.asarray(verts, np.float32)
    if faces is None:
        v = v.reshape(-1, 3)
        faces = np.arange(len(v)).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    rep = np.arange(V)
    if cell == 0:
        bits = (v + np.float32(0)).view(np.int32)
        lonely = np.isnan(v).any(1)
        seen = {}
        for i in range(V):
            if lonely[i]:
                continue
            rep[i] = seen.setdefault(bits[i].tobytes(), i)
    else:
        keys, _ = voxel_keys(v, cell)
        seen = {}
        for i in range(V):
            if keys[i] >= 0:
                rep[i] = seen.setdefault(int(keys[i]), i)
    kept = np.nonzero(rep == np.arange(V))[0]
    remap = np.searchsorted(kept, rep).astype(np.int32)
    nf = remap[f].reshape(-1, 3)
    if drop_degenerate:
        nf = nf[(nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 2] != nf[:, 0])]
    return kept.astype(np.int32), nf.astype(np.int32), remap


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def disjoint_triangles(F):
    """F triangles on 3 F + 2 vertices (the last two unreferenced)"""
    rng = np.random.default_rng(F)
    verts = rng.random((3 * F + 2, 3)).astype(np.float32)
    return verts, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def ladder(n, order="ascending", seed=0):
    """a strip of 2 (n - 1) triangles between two rails of n vertices (rail a: 0 .. n-1, rail b: n .. 2n-1)"""
    i = np.arange(n - 1)
    f = np.concatenate([np.stack([i, i + 1, n + i], 1), np.stack([i + 1, n + i + 1, n + i], 1)]).reshape(2, n - 1, 3)
    f = f.transpose(1, 0, 2).reshape(-1, 3)                                 # faces ascend along the ladder
    rng = np.random.default_rng(seed)
    if order == "descending":
        f = f[::-1]
    elif order == "shuffled":
        f = f[rng.permutation(len(f))]
    elif order == "permuted":
        f = rng.permutation(2 * n)[f]
    x = np.arange(n, dtype=np.float32)
    verts = np.concatenate([np.stack([x, 0 * x, 0 * x], 1), np.stack([x, 0 * x + 1, 0 * x], 1)]).astype(np.float32)
    if order == "permuted":
        inv = np.empty(2 * n, np.int64)
        inv[np.random.default_rng(seed).permutation(2 * n)] = np.arange(2 * n)
        verts = verts[inv]
    return verts, np.ascontiguousarray(f, np.int32)


TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)          # outward for the corners below
TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)


def pinch():
    """two tetrahedra that share vertex 3 only"""
    second = np.array([3, 4, 5, 6])[TETRA]
    verts = np.concatenate([TETRA_V, TETRA_V[[0, 1, 2]] + np.float32([0, 0, 2])])
    return verts.astype(np.float32), np.concatenate([TETRA, second]).astype(np.int32)


def sheets(sizes):
    """open sheets of n x m unit quads side by side, one component each: area n m, 2 n m faces, exactly"""
    vs, fs, off = [], [], 0
    for k, (n, m) in enumerate(sizes):
        v, f = open_sheet(n, m)
        vs.append(v + np.float32([0, 0, 3 * k]))
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def open_sheet(n=5, m=7):
    """an n x m grid of quads, two triangles each, consistently wound"""
    ii, jj = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a = (ii * (m + 1) + jj).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + m + 1], 1), np.stack([a + 1, a + m + 2, a + m + 1], 1)])
    gi, gj = np.meshgrid(np.arange(n + 1), np.arange(m + 1), indexing="ij")
    verts = np.stack([gi, gj, 0 * gi], -1).reshape(-1, 3).astype(np.float32)
    return verts, f.astype(np.int32)


def fan3():
    """three triangles on the edge (0, 1)"""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return verts, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


def flipped_tetra():
    f = TETRA.copy()
    f[2] = f[2, ::-1]
    return TETRA_V.copy(), f


def icosphere(level=2):
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)


def sphere_halves(level=2):
    """an icosphere cut into the faces with centroid z >= 0 and the rest, each half with vertices of its own: the seam vertices
    appear twice, bit-equal.  -> (verts, faces) of the two halves side by side"""
    v, f = icosphere(level)
    up = v[f].mean(1)[:, 2] >= 0
    parts, off = [], 0
    for sel in (up, ~up):
        nf, vmap, used = compact(f, len(v), sel)
        parts.append((v[used], nf + off))
        off += len(used)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]).astype(np.int32)


def exact_weld_case():
    """an indexed mesh whose vertices are first used in ascending order (so that welding its soup restores its very indices),
    with a -0 / +0 pair among the coordinates, plus one face that has a NaN corner"""
    v, f = open_sheet(3, 4)
    v = v.copy()
    v[:, 2] = np.where(np.arange(len(v)) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    order = []
    for i in f.reshape(-1):
        if i not in order:
            order.append(int(i))
    assert len(order) == len(v)
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    v, f = v[order], rank[f].astype(np.int32)
    soup = v[f].copy()                                                      # (F,3,3)
    soup[1, 0, 2] = np.float32(0.0) if np.signbit(soup[1, 0, 2]) else np.float32(-0.0)      # the same corner, the other zero
    nan_face = np.array([[[np.nan, 0, 0], [5, 5, 5], [6, 5, 5]]], np.float32)
    return v, f, np.concatenate([soup, nan_face]).astype(np.float32)


def jittered_lattice(n=6, cell=0.25, copies=3, seed=0):
    """n^3 lattice points at cell centres (relative to the minimum corner, which is a lattice point itself), `copies` times, each
    copy jittered by at most 0.2 cell; point 0 is kept exactly at the corner so the minimum is known"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts, ids = [], []
    for k in range(copies):
        j = rng.uniform(-0.2, 0.2, g.shape) * cell
        j = np.where((g == 0), np.abs(j), j)                                # nothing below the minimum corner
        if k == 0:
            j[0] = 0
        pts.append(g * cell + j)
        ids.append(np.arange(len(g)))
    order = rng.permutation(len(g) * copies)
    order = np.concatenate([[0], order[order != 0]])                        # the exact corner stays first
    return np.concatenate(pts)[order].astype(np.float32), np.concatenate(ids)[order], cell
