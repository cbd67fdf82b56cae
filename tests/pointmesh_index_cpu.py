"""numpy restatement of csrc/point_mesh_index.hip ("The tile-box index"): the Morton keys, the stable order,
the tile table, the skip rule and the minimum rule, on numpy float32 with one IEEE rounding per operation as the kernels'
under `fp contract(off)`.  The pair values themselves are pointmesh_cpu's (`_pairs`, `face_records`): the index only decides
WHICH pairs are evaluated, and ``search`` must return what ``pointmesh_cpu.closest_f32`` returns, bit for bit."""
import numpy as np

import pointmesh_cpu as P

TILE, GROUP = 64, 64                    # cnr_pm_index_params
f32 = np.float32

# The skip rule's margin.  MEASURED_EXCESS: the largest (lb - sqrt(d2_32)) / (2^-24 (lb + L)) over ALL (query, face) pairs --
# lb the fp32 box distance as the kernel forms it (per-face box, the face's tile box, group box to tile box), d2_32 the pair's
# fp32 squared distance of pointmesh_cpu._pairs, L the face's fp32 longest edge -- on every BIT_CASES scene, the same with the
# queries shifted by 100 m and 1000 m, and near_planar_scene; measured by
# test_pointmesh_index_host.py::test_margin_constant_is_four_times_the_measured_excess: 4.452 (per-face box, at (2049, 1000);
# the tile box 2.553, the group box below 0).  C_MARGIN is a power of two >= 4 x that.
MEASURED_EXCESS = 4.46
C_MARGIN = 32
MARGIN = f32(C_MARGIN * 2.0 ** -24)


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def bbox_of(verts):
    """(6,) f32: lo xyz, hi xyz of all vertices"""
    v = np.asarray(verts, f32).reshape(-1, 3)
    return np.concatenate([v.min(0), v.max(0)])


def _cell(x, lo, hi):
    with np.errstate(over="ignore"):
        ext = f32(hi) - f32(lo)
    if not (ext > 0 and ext < np.inf):                                  # no extent, or one that overflows fp32: cell 0
        return np.zeros(len(x), np.int32)
    xc = np.minimum(np.maximum(x.astype(f32), f32(lo)), f32(hi))
    t = (xc - f32(lo)) / ext
    return np.minimum((t * f32(1024.0)).astype(np.int32), 1023)


def _spread(v):
    v = v.astype(np.int64)
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def _keys(p, bbox):
    c = [_spread(_cell(p[:, k], bbox[k], bbox[3 + k])) for k in range(3)]
    return (c[0] | (c[1] << 1) | (c[2] << 2)).astype(np.int32)


def face_keys(tri, bbox):
    """tri (F,3,3) f32 corners -> (F,) i32: the Morton code of the box centre 0.5 (min + max)"""
    return _keys(f32(0.5) * (tri.min(1) + tri.max(1)), bbox)


def query_keys(q, bbox):
    return _keys(np.asarray(q, f32).reshape(-1, 3), bbox)


# ---- the index ----------------------------------------------------------------------------------------------------------------
def build(verts, faces=None):
    """-> dict(bbox, keys (F,) i32, order (F,) i64, rec: pointmesh_cpu.face_records in key order, orig (F,) original indices
    in key order, lo / hi (T,3) f32, lmax (T,) f32, first (T,) i32, edge (F,) f32: every face's longest fp32 edge, original order)"""
    tri = P.corners(verts, faces, f32)
    bbox = bbox_of(verts)
    keys = face_keys(tri, bbox)
    order = np.argsort(keys, kind="stable")
    F = len(tri)
    T = -(-F // TILE)
    ts = tri[order]
    ab, ac, bc = ts[:, 1] - ts[:, 0], ts[:, 2] - ts[:, 0], ts[:, 2] - ts[:, 1]
    e2 = np.maximum(np.maximum(P._dot(ab, ab), P._dot(ac, ac)), P._dot(bc, bc))
    starts = np.arange(T) * TILE
    lo = np.minimum.reduceat(ts.min(1), starts, axis=0)
    hi = np.maximum.reduceat(ts.max(1), starts, axis=0)
    lmax = np.sqrt(np.maximum.reduceat(e2, starts))
    edge = np.empty(F, f32)
    edge[order] = np.sqrt(e2)
    return dict(bbox=bbox, keys=keys, order=order, rec=P.face_records(ts), orig=order.astype(np.int64), lo=lo, hi=hi,
                lmax=lmax.astype(f32), first=keys[order][starts], edge=edge, F=F, T=T)


def box_distance(glo, ghi, lo, hi):
    """the kernel's lb: the per-axis gap max(lo_t - hi_g, lo_g - hi_t, 0) first, then sqrt of the dot product, fp32"""
    g = np.maximum(np.maximum(lo - ghi, glo - hi), f32(0))
    return np.sqrt(P._dot(g, g))


def survives(lb, lmax, m):
    """NOT the skip rule: a tile may be skipped only if lb - C 2^-24 (lb + Lmax) > sqrt(M), M the group's largest minimum"""
    thr = lb - MARGIN * (lb + lmax)
    return ~(thr > np.sqrt(m.max()))


def search(points, verts, faces=None, index=None):
    """cnr_point_mesh_dist_indexed -> (dist f32, face i64 (original indices), closest (nq,3) f32, squared distance f32,
    visited (groups,) tiles evaluated by each group)"""
    ix = build(verts, faces) if index is None else index
    q = np.asarray(points, f32).reshape(-1, 3)
    nq, T, F = len(q), ix["T"], ix["F"]
    qkeys = query_keys(q, ix["bbox"])
    qorder = np.argsort(qkeys, kind="stable")
    d2, face, closest = np.empty(nq, f32), np.empty(nq, np.int64), np.empty((nq, 3), f32)
    groups = -(-nq // GROUP)
    visited = np.zeros(groups, np.int64)
    for g in range(groups):
        idx = qorder[g * GROUP:(g + 1) * GROUP]
        qs = q[idx]
        glo, ghi = qs.min(0), qs.max(0)
        m = np.full(len(qs), np.inf, f32)
        mf = np.full(len(qs), 2 ** 31 - 1, np.int64)
        mr = np.zeros((len(qs), 3), f32)

        def evaluate(t):
            nonlocal m, mf, mr
            s = slice(t * TILE, min((t + 1) * TILE, F))
            dd, r = P._pairs(qs, tuple(a[s] for a in ix["rec"]))
            orig = ix["orig"][s]
            best = dd.min(1)
            j = np.where(dd == best[:, None], orig[None], 2 ** 62).argmin(1)     # the lowest original index among the tile's minima
            take = (best < m) | ((best == m) & (orig[j] < mf))                  # the minimum rule
            k = np.arange(len(qs))
            m, mf = np.where(take, best, m), np.where(take, orig[j], mf)
            mr = np.where(take[:, None], r[k, j], mr)
            visited[g] += 1
        key = qkeys[qorder[min(g * GROUP + GROUP // 2, nq - 1)]]
        seed = max(0, int(np.searchsorted(ix["first"], key, side="right")) - 1)
        evaluate(seed)
        nb, sb = -(-T // 64), seed // 64
        for step in range(2 * max(sb, nb - 1 - sb) + 1):
            off = (step + 1) >> 1
            b = sb + off if step & 1 else sb - off
            if not 0 <= b < nb:
                continue
            t = np.arange(b * 64, min(b * 64 + 64, T))
            valid = t != seed
            lb = box_distance(glo, ghi, ix["lo"][t], ix["hi"][t])
            todo = valid & survives(lb, ix["lmax"][t], m)
            while todo.any():
                j = int(np.argmax(todo))
                evaluate(int(t[j]))
                todo[:j + 1] = False
                todo &= survives(lb, ix["lmax"][t], m)
        d2[idx], face[idx], closest[idx] = m, mf, qs + mr
    return np.sqrt(d2), face, closest, d2, visited


# ---- the margin ---------------------------------------------------------------------------------------------------------------
def excess(points, verts, faces=None):
    """the worst (lb - sqrt(d2_32)) / (2^-24 (lb + L)) over all (query, face) pairs for the three bounds
    -> (per-face box, the face's tile box, group box to tile box)"""
    ix = build(verts, faces)
    tri = P.corners(verts, faces, f32)
    rec = P.face_records(tri)
    q = np.asarray(points, f32).reshape(-1, 3)
    nq, F = len(q), ix["F"]
    tile_of = np.empty(F, np.int64)
    tile_of[ix["order"]] = np.arange(F) // TILE
    qorder = np.argsort(query_keys(q, ix["bbox"]), kind="stable")
    group_of = np.empty(nq, np.int64)
    group_of[qorder] = np.arange(nq) // GROUP
    starts = np.arange(-(-nq // GROUP)) * GROUP
    glo = np.minimum.reduceat(q[qorder], starts, axis=0)[group_of]
    ghi = np.maximum.reduceat(q[qorder], starts, axis=0)[group_of]
    boxes = ((tri.min(1), tri.max(1)), (ix["lo"][tile_of], ix["hi"][tile_of]))
    L = ix["edge"].astype(np.float64)
    worst = np.full(3, -np.inf)
    step = max(1, (P.PAIRS_PER_BLOCK // 4) // F)
    for s in range(0, nq, step):
        e = slice(s, s + step)
        d = np.sqrt(P._pairs(q[e], rec)[0].astype(np.float64))
        qa = q[e, None, :]
        for k, (lo, hi, a, b) in enumerate(((*boxes[0], qa, qa), (*boxes[1], qa, qa),
                                            (*boxes[1], glo[e, None, :], ghi[e, None, :]))):
            lb = box_distance(a, b, lo[None], hi[None]).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):                # 0 / 0: a point face at distance 0
                worst[k] = max(worst[k], float(np.nanmax((lb - d) / (2.0 ** -24 * (lb + L[None])))))
    return tuple(worst)


def near_planar_scene(nq=2048, seed=21):
    """Two sheets of 2 TILE triangles each (8 x 8 quads over a unit square, the second 1.5 m along x), slightly tilted and
    coplanar within 1e-6: the first sheet's vertices have z in [-1e-6, 0), the second's in (0, 1e-6], so the top bit of the key
    (z's) separates the sheets and each fills two whole tiles.  Queries 1 mm to 1 m above them; a query's key sees x and y only
    (z is clamped to the box), so the height follows y (three decades over the sheets' width, times a factor in [0.8, 1.25]):
    the groups at low y hold queries millimetres above the sheets and skip tiles, those at high y skip nothing.  Here the
    fp32 plane distance of a pair most often falls below the box gap.  -> (q, verts, faces, sheet (F,) 0 or 1)"""
    rng = np.random.default_rng(seed)
    n = int(np.sqrt(TILE))
    g = np.stack(np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij"), -1).reshape(-1, 2) / float(n)
    k = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None]).reshape(-1)
    quad = np.concatenate([np.stack([k, k + n + 1, k + n + 2], 1), np.stack([k, k + n + 2, k + 1], 1)])
    verts, faces = [], []
    for sheet in range(2):
        xy = g + rng.uniform(-0.2, 0.2, g.shape) / n + [1.5 * sheet, 0.0]
        z = rng.uniform(1e-8, 1e-6, (len(g), 1)) * (1 if sheet else -1)
        faces.append(quad + len(g) * sheet)
        verts.append(np.concatenate([xy, z], 1))
    xy = rng.uniform([-0.2, -0.2], [2.7, 1.2], (nq, 2))
    h = 10.0 ** (-3.0 + 3.0 * (xy[:, 1:] + 0.2) / 1.4) * rng.uniform(0.8, 1.25, (nq, 1))
    q = np.concatenate([xy, np.clip(h, 1e-3, 1.0)], 1)
    return (q.astype(f32), np.concatenate(verts).astype(f32), np.concatenate(faces).astype(np.int32),
            np.repeat([0, 1], len(quad)))


def uv_sphere(n_lat=24, n_lon=48, centre=(0.3, -0.2, 0.5)):
    """a UV sphere of radius 1: 2 n_lon (n_lat - 1) faces -> (verts, faces)"""
    th = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph), np.cos(th)[:, None] * np.ones_like(ph)], -1)
    v = np.concatenate([ring.reshape(-1, 3), [[0, 0, 1.0], [0, 0, -1.0]]]) + np.asarray(centre)
    i = np.arange(n_lat - 2)[:, None] * n_lon + np.arange(n_lon)[None]
    j = np.arange(n_lat - 2)[:, None] * n_lon + (np.arange(n_lon)[None] + 1) % n_lon
    quads = np.concatenate([np.stack([i, i + n_lon, j + n_lon], -1).reshape(-1, 3), np.stack([i, j + n_lon, j], -1).reshape(-1, 3)])
    top, bot, last = len(v) - 2, len(v) - 1, (n_lat - 2) * n_lon
    k, k1 = np.arange(n_lon), (np.arange(n_lon) + 1) % n_lon
    caps = np.concatenate([np.stack([np.full(n_lon, top), k, k1], 1), np.stack([np.full(n_lon, bot), last + k1, last + k], 1)])
    return v.astype(f32), np.concatenate([quads, caps]).astype(np.int32)


def sphere_scene(nq=4096, seed=6, **kw):
    """uv_sphere with nq queries at 1.02 r: the answer lies 2 % of the radius away, most tiles much farther
    -> (q, verts, faces)"""
    v, f = uv_sphere(**kw)
    d = np.random.default_rng(seed).normal(size=(nq, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (np.asarray(kw.get("centre", (0.3, -0.2, 0.5))) + 1.02 * d).astype(f32), v, f


def two_clusters(nq=600, F=512, seed=33):
    """two clusters of F random_case faces, the second shifted by +100 on every axis; the queries lie inside the first cluster's
    box -> (q, verts, faces)"""
    _, v, f = P.random_case(8, F, seed)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    q = rng.uniform(lo, hi, (nq, 3)).astype(f32)
    return q, np.concatenate([v, v + f32(100.0)]), np.concatenate([f, f + len(v)])


# ---- sizes: cnr_pm_index_bytes(F) = align256(64 F) + align256(32 tiles); workspace = align256(4 groups) -----------------------
def index_bytes(F):
    return P.align256(64 * F) + P.align256(32 * -(-F // TILE))


def workspace_bytes(nq):
    return P.align256(4 * -(-nq // GROUP))
