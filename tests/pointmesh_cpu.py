"""numpy restatement of csrc/point_mesh.hip and the fixtures its tests share.

``closest_f32`` does the kernel's operations in the kernel's order on numpy float32 (every operation one IEEE rounding, as the
kernel's under `fp contract(off)`), ``closest_f64`` is the same algorithm in float64, ``closest_alt_f64`` an independent float64
formulation (plane projection, inside test by edge cross products, else the three segments), ``sample_faces`` the searchsorted
rule of cnr_sample_faces."""
import numpy as np

PAIRS_PER_BLOCK = 1 << 19


def corners(verts, faces=None, dtype=np.float64):
    """(F,3,3) corners of an indexed mesh, or of a soup (F*3,3) when faces is None; the fp32 values, in `dtype`"""
    v = np.asarray(verts, np.float32).astype(dtype)
    return v.reshape(-1, 3, 3) if faces is None else v[np.asarray(faces, np.int64)]


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def face_records(tri):
    """pm_record_kernel: (a, ab, ac, e00, e01, e11, unit normal) in tri's dtype.  A face whose edge vectors are exactly parallel or zero
    (ab x ac == 0 in float64 of the edges) becomes its longest edge (ab, then ac, then bc; a later one only when strictly
    longer) as a triangle with ac = 0."""
    a, b, c = tri[:, 0].copy(), tri[:, 1], tri[:, 2]
    ab, ac, bc = b - a, c - a, c - b
    e00, e01, e11, e22 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac), _dot(bc, bc)
    n = np.cross(ab.astype(np.float64), ac.astype(np.float64))          # products of fp32 values are exact in fp64
    deg = (n == 0).all(1)
    best = e00.copy()
    use_ac = deg & (e11 > best)
    best = np.where(use_ac, e11, best)
    use_bc = deg & (e22 > best)
    best = np.where(use_bc, e22, best)
    ab = np.where(use_ac[:, None], ac, ab)
    ab = np.where(use_bc[:, None], bc, ab)
    a = np.where(use_bc[:, None], b, a)
    zero = np.zeros_like(e00)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    nh = (n / np.sqrt(np.where(deg, 1.0, nn))[:, None]).astype(e00.dtype)   # the unit normal in fp64, rounded once
    return (a, ab, np.where(deg[:, None], zero[:, None], ac), np.where(deg, best, e00), np.where(deg, zero, e01),
            np.where(deg, zero, e11), nh)


def _pairs(q, rec):
    """pm_pair for every (query, face): -> (d2 (nq,F), r (nq,F,3)), r = closest - q"""
    a, ab, ac, e00, e01, e11, nh = rec
    dt = q.dtype.type
    zero, one = dt(0), dt(1)
    ap = q[:, None, :] - a[None]
    d1, d2 = _dot(ab[None], ap), _dot(ac[None], ap)
    d3, d4 = d1 - e00[None], d2 - e01[None]
    d5, d6 = d1 - e01[None], d2 - e11[None]
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    g43, g56 = d4 - d3, d5 - d6
    nv, nw, den = zero * va, zero * va, one + zero * va                 # interior: the plane distance below
    interior = np.ones(va.shape, bool)
    for cond, cv, cw, cd in (
            ((va <= 0) & (g43 >= 0) & (g56 >= 0), g56, g43, g43 + g56),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
            ((d6 >= 0) & (d5 <= d6), zero, one, one),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
            ((d3 >= 0) & (d4 <= d3), one, zero, one),
            ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
        nv, nw, den = np.where(cond, cv, nv), np.where(cond, cw, nw), np.where(cond, cd, den)
        interior &= ~cond
    bad = ~(den > 0)
    nv, nw, den = np.where(bad, zero, nv), np.where(bad, zero, nw), np.where(bad, one, den)
    with np.errstate(over="ignore", invalid="ignore"):
        inv = one / den
        v, w = nv * inv, nw * inv
        r = (v[..., None] * ab[None] + w[..., None] * ac[None]) - ap
        h = zero - _dot(nh[None], ap)                                   # interior: r = -(n . ap) n, n the unit normal
        r = np.where(interior[..., None], h[..., None] * nh[None], r)
        return _dot(r, r), r


def _closest(points, verts, faces, dtype):
    q = np.asarray(points, np.float32).reshape(-1, 3).astype(dtype)
    rec = face_records(corners(verts, faces, dtype))
    F = len(rec[0])
    nq = len(q)
    d2, face, closest = np.empty(nq, dtype), np.empty(nq, np.int64), np.empty((nq, 3), dtype)
    step = max(1, PAIRS_PER_BLOCK // F)
    for s in range(0, nq, step):
        dd, r = _pairs(q[s:s + step], rec)
        f = np.argmin(dd, axis=1)                                       # the first (lowest) index among equal minima
        k = np.arange(len(f))
        d2[s:s + step], face[s:s + step] = dd[k, f], f
        closest[s:s + step] = q[s:s + step] + r[k, f]
    return np.sqrt(d2), face, closest, d2


def closest_f32(points, verts, faces=None):
    """-> (dist f32, face i64, closest (nq,3) f32, squared distance f32): what cnr_point_mesh_dist computes, bit for bit"""
    return _closest(points, verts, faces, np.float32)


def closest_f64(points, verts, faces=None):
    """the same algorithm on the same fp32 inputs in float64"""
    return _closest(points, verts, faces, np.float64)


def _segment_d2(q, a, b):
    """squared distance of q (nq,1,3) to the segments a b (1,F,3) each, float64"""
    ab = b - a
    ll = (ab * ab).sum(-1)
    t = ((q - a) * ab).sum(-1) / np.where(ll > 0, ll, 1.0)
    t = np.clip(np.where(ll > 0, t, 0.0), 0.0, 1.0)
    r = q - (a + t[..., None] * ab)
    return (r * r).sum(-1)


def closest_alt_f64(points, verts, faces=None):
    """An independent float64 formulation -> (dist, face).  The query's projection onto the face's plane; when it lies inside
    the triangle (the three edge cross products point along the normal), the distance is |plane distance|; otherwise, and for
    a face without a normal, the minimum over the three edge segments."""
    q = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    tri = corners(verts, faces)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    dist, face = np.empty(len(q)), np.empty(len(q), np.int64)
    step = max(1, PAIRS_PER_BLOCK // len(tri))
    for s in range(0, len(q), step):
        p = q[s:s + step, None, :]
        h = ((p - a) * n).sum(-1)
        safe = np.where(nn > 0, nn, 1.0)
        proj = p - (h / safe)[..., None] * n
        inside = nn > 0
        for u, v in ((a, b), (b, c), (c, a)):
            inside = inside & ((np.cross(v - u, proj - u) * n).sum(-1) >= 0)
        seg = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, b, c)), _segment_d2(p, c, a))
        d2 = np.where(inside, h * h / safe, seg)
        f = np.argmin(d2, axis=1)
        dist[s:s + step], face[s:s + step] = np.sqrt(d2[np.arange(len(f)), f]), f
    return dist, face


def sample_faces(cum, u0):
    """cnr_sample_faces: the first f with cum[f] >= u0 * cum[-1] (side 'left'), the last face when there is none"""
    cum = np.asarray(cum, np.float64)
    return np.minimum(np.searchsorted(cum, np.asarray(u0, np.float64) * cum[-1], side="left"), len(cum) - 1)


def longest_edge(verts, faces, face):
    """the longest edge (float64) of each of the faces `face`"""
    t = corners(verts, faces)[face]
    e = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]], 1)
    return np.sqrt((e * e).sum(-1)).max(1)


def bar(d64, L, K):
    """the fp32 error bar of a distance d64 whose winning face has longest edge L: K 2^-24 (d64 + L)"""
    return K * 2.0 ** -24 * (d64 + L)


# max |closest_f32 - closest_f64| / (2^-24 (d64 + L)) over every query of BIT_CASES' random_case scenes, measured by
# test_pointmesh_host.py::test_fp32_error_constant_on_the_gpu_tests_cases (2.509, at (2048, 1)); the GPU bar is 4 K.
# (With the barycentric form r = v ab + w ac - ap in the interior region too, the same cases gave 8.7 and the large case 45:
# near a sliver, v and w carry the cancellation of va, vb, vc times the long edges.)
K_F32 = 2.51


# ---- the workspace of cnr_point_mesh_dist: align256(64 F) + chunks * align256(8 nq) --------------------------------------------
QUERIES_PER_BLOCK, FACES_PER_TILE, TARGET_WORKGROUPS = 1024, 256, 2048


def align256(x):
    return (x + 255) // 256 * 256


def chunk_count(nq, F):
    """the face chunks of the grid: whole tiles per chunk, about TARGET_WORKGROUPS workgroups over the query blocks"""
    qblocks = -(-nq // QUERIES_PER_BLOCK)
    tiles = -(-F // FACES_PER_TILE)
    want = max(1, min(tiles, -(-TARGET_WORKGROUPS // qblocks)))
    chunk_len = -(-tiles // want) * FACES_PER_TILE
    return -(-F // chunk_len)


def workspace_chunks(nq, F, nbytes):
    """the chunk count read back from cnr_point_mesh_workspace_bytes(nq, F)"""
    rest = nbytes - align256(64 * F)
    assert rest > 0 and rest % align256(8 * nq) == 0
    return rest // align256(8 * nq)


# ---- fixtures shared by test_pointmesh_host.py (which measures K on them) and test_pointmesh_gpu.py -----------------------------
BIT_CASES = ((1, 1), (1, 2), (63, 65), (64, 256), (65, 257), (2047, 255), (2048, 1), (2049, 1000), (100, 2000))
LARGE_CASE = (20000, 50000)


def random_case(nq, F, seed=None):
    """An indexed mesh of F random triangles and nq queries, coordinates in metres inside [-1, 5].  Triangle sizes are
    log-uniform from 1 mm to 1 m; one in eight is a sliver (height 1 to 10 % of its base).  Half the queries lie within 1 mm
    of a face (a random point of a random face plus a random offset), the rest anywhere in the volume.  The vertices are
    shuffled, so the indexed form and the soup `verts[faces]` read memory differently.
    -> (q (nq,3) f32, verts (3F,3) f32, faces (F,3) i32)"""
    rng = np.random.default_rng(1000003 * nq + F if seed is None else seed)
    size = 10.0 ** rng.uniform(-3.0, 0.0, F)
    centre = rng.uniform(0.0, 4.0, (F, 3))
    e = rng.normal(size=(F, 2, 3))
    e /= np.linalg.norm(e, axis=2, keepdims=True)
    sliver = rng.random(F) < 0.125
    perp = e[:, 1] - (e[:, 1] * e[:, 0]).sum(1, keepdims=True) * e[:, 0]
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    thin = rng.uniform(0.1, 0.9, (F, 1)) * e[:, 0] + rng.uniform(0.01, 0.1, (F, 1)) * perp
    e[:, 1] = np.where(sliver[:, None], thin, e[:, 1])
    a = centre - 0.33 * size[:, None] * (e[:, 0] + e[:, 1])
    tri = np.stack([a, a + size[:, None] * e[:, 0], a + size[:, None] * e[:, 1]], 1).astype(np.float32)
    perm = rng.permutation(3 * F)
    verts = np.empty((3 * F, 3), np.float32)
    verts[perm] = tri.reshape(-1, 3)
    faces = perm.reshape(F, 3).astype(np.int32)
    near = nq // 2
    f = rng.integers(0, F, near)
    bc = rng.dirichlet(np.ones(3), near)
    d = rng.normal(size=(near, 3))
    d *= (rng.uniform(0.0, 1e-3, (near, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    q_near = (tri[f].astype(np.float64) * bc[:, :, None]).sum(1) + d
    q = np.concatenate([q_near, rng.uniform(-1.0, 5.0, (nq - near, 3))])
    return q[rng.permutation(nq)].astype(np.float32), verts, faces


def soup(verts, faces):
    """the (F*3,3) soup of an indexed mesh"""
    return np.ascontiguousarray(np.asarray(verts, np.float32)[np.asarray(faces, np.int64)].reshape(-1, 3))


def grid_scene(nq=300, F=200, seed=5):
    """Every coordinate on the 2^-12 grid in [0,1): all differences, and the scene shifted by GRID_SHIFT, are exact in fp32
    -> (q, soup verts)"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 4096, (nq, 3)) / 4096.0
    c = rng.integers(0, 4096, (F, 1, 3))
    v = np.clip(c + rng.integers(-300, 301, (F, 3, 3)), 0, 4095) / 4096.0
    q[: nq // 3] = v.reshape(-1, 3)[rng.integers(0, 3 * F, nq // 3)]            # some queries on corners: distance zero
    return q.astype(np.float32), v.reshape(-1, 3).astype(np.float32)


GRID_SHIFT = np.array([64.0, -32.0, 16.0], np.float32)

# corner index triples of the unit cube's 12 triangles over CUBE_VERTS (vertex k = (k & 1, k >> 1 & 1, k >> 2 & 1))
CUBE_VERTS = np.array([[k & 1, k >> 1 & 1, k >> 2 & 1] for k in range(8)], np.float32)
CUBE_FACES = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3],
                       [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]], np.int32)


def cube_tie_queries():
    """queries on the cube's vertices, edge midpoints and face diagonals (distance 0 to several faces), and outside the edges
    and vertices at equal distance from two or more faces; all dyadic, so every squared distance is exact in fp32"""
    v = CUBE_VERTS.astype(np.float64)
    q = [v]                                                                     # vertex 0 belongs to 6 faces
    edges = [(i, j) for i in range(8) for j in range(i + 1, 8) if bin(i ^ j).count("1") == 1]
    q.append(np.array([(v[i] + v[j]) / 2 for i, j in edges]))
    q.append(np.array([[0.5, 0.5, 0.0], [0.25, 0.25, 0.0], [0.5, 0.5, 1.0], [0.0, 0.5, 0.5], [1.0, 0.25, 0.25], [0.75, 0.0, 0.75]]))
    centre = np.full(3, 0.5)
    q.append(np.array([centre + 1.5 * ((v[i] + v[j]) / 2 - centre) for i, j in edges]))      # outside an edge, on its bisector
    q.append(centre + 2.0 * (v - centre))                                       # outside a vertex, on the cube's diagonal
    return np.concatenate(q).astype(np.float32)


def degenerate_mesh(seed=9):
    """A valid random mesh with point triangles, collinear triangles (the middle corner in every position) and triangles with a
    repeated corner mixed in, all on dyadic coordinates so that the edge vectors are exactly parallel
    -> (q, verts, faces, is_degenerate (F,))"""
    rng = np.random.default_rng(seed)
    _, verts, faces = random_case(8, 40, seed)
    extra_v, extra_f = [], []
    base = len(verts)

    def add(a, b, c):
        k = base + len(extra_v)
        extra_v.extend([a, b, c])
        extra_f.append([k, k + 1, k + 2])
    for k in range(12):
        p = rng.integers(0, 512, 3) / 128.0
        d = rng.integers(-64, 65, 3) / 256.0
        d[0] = d[0] or 0.25
        kind = k % 6
        if kind == 0:
            add(p, p, p)                                                        # a point
        elif kind == 1:
            add(p, p + d, p + 3 * d)                                            # collinear, b in the middle
        elif kind == 2:
            add(p + 3 * d, p, p + d)                                            # collinear, c in the middle
        elif kind == 3:
            add(p + d, p + 3 * d, p)                                            # collinear, a in the middle
        elif kind == 4:
            add(p, p, p + d)                                                    # a == b
        else:
            add(p, p + d, p + d)                                                # b == c
    verts = np.concatenate([verts, np.array(extra_v, np.float32)])
    faces = np.concatenate([faces, np.array(extra_f, np.int32)])
    order = rng.permutation(len(faces))
    faces = np.ascontiguousarray(faces[order])
    is_deg = order >= 40
    t = corners(verts, faces)
    f = np.flatnonzero(is_deg)
    w = rng.dirichlet(np.ones(3), (len(f), 6))                                  # queries near every degenerate face
    near = (t[f][:, None] * w[..., None]).sum(2).reshape(-1, 3) + rng.normal(size=(len(f) * 6, 3)) * 0.01
    q = np.concatenate([near, rng.uniform(-1, 5, (60, 3)), t[f].reshape(-1, 3)])
    return q.astype(np.float32), verts, faces, is_deg
