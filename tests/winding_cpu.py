"""numpy restatement of csrc/winding.hip and the fixtures its tests share.

``winding_f64`` does the kernel's operations in the kernel's order on numpy float64 (every operation one IEEE rounding, as the
kernel's under `fp contract(off)`; only ``atan2`` and the rounding of ``sqrt`` may differ between the two, which is what ``bar``
allows for), ``winding_mp`` is the same formula in mpmath at 40 digits, ``winding_alt_f64`` an independent float64 form (the
spherical excess from the three dihedral angles, signed by the determinant), ``mesh_orientation`` the rule of
metrics.mesh_orientation."""
import numpy as np

import pointmesh_cpu as P
from pointmesh_cpu import (BIT_CASES, CUBE_FACES, CUBE_VERTS, GRID_SHIFT, align256, corners, cube_tie_queries,  # noqa: F401
                           degenerate_mesh, grid_scene, random_case, soup)

TWO_PI = 6.283185307179586
PAIRS_PER_BLOCK = 1 << 18

# ---- the workspace of cnr_winding_number: chunks * align256(8 nq) -----------------------------------------------------------
QUERIES_PER_BLOCK, FACES_PER_TILE, TARGET_WORKGROUPS = 512, 256, 2048


def chunk_length(nq, F):
    """faces per chunk of the grid: whole tiles, about TARGET_WORKGROUPS workgroups over the query blocks"""
    qblocks = -(-nq // QUERIES_PER_BLOCK)
    tiles = -(-F // FACES_PER_TILE)
    want = max(1, min(tiles, -(-TARGET_WORKGROUPS // qblocks)))
    return -(-tiles // want) * FACES_PER_TILE


def chunk_count(nq, F):
    return -(-F // chunk_length(nq, F))


def workspace_chunks(nq, F, nbytes):
    """the chunk count read back from cnr_winding_workspace_bytes(nq, F)"""
    assert nbytes > 0 and nbytes % align256(8 * nq) == 0
    return nbytes // align256(8 * nq)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    """each component two products and one subtraction"""
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def pair_terms(q, tri, lengths=None):
    """wn_pair for every (query, face): q (nq,3) f64, tri (F,3,3) f64 -> (t, det, den, la lb lc), (nq,F) each.
    lengths: a function (la, lb, lc) -> (la, lb, lc) applied to the three lengths before they are used (the perturbation test)"""
    A, B, C = (tri[None, :, k] - q[:, None, :] for k in range(3))
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    if lengths is not None:
        la, lb, lc = lengths(la, lb, lc)
    det = _dot(A, _cross(B, C))
    den = ((la * lb) * lc + _dot(A, B) * lc) + (_dot(B, C) * la + _dot(C, A) * lb)
    t = np.where(det == 0, 0.0, np.arctan2(det, den))
    return t, det, den, (la * lb) * lc


def _blocks(points, verts, faces):
    q = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    tri = corners(verts, faces)
    step = max(1, PAIRS_PER_BLOCK // len(tri))
    return q, tri, [slice(s, s + step) for s in range(0, len(q), step)]


def winding_f64(points, verts, faces=None, lengths=None, with_bar=False):
    """-> w (nq,) f64: what cnr_winding_number computes for this batch of queries, up to atan2 and sqrt's last bits.  Within
    a face chunk the terms are added in face order onto a sum that starts at 0, the chunks in chunk order; the chunk length is
    the grid's for (nq, F).  with_bar=True: -> (w, bar)"""
    q, tri, blocks = _blocks(points, verts, faces)
    F, L = len(tri), chunk_length(len(q), len(tri))
    w, b = np.empty(len(q)), np.empty(len(q))
    for s in blocks:
        t, det, den, lll = pair_terms(q[s], tri, lengths)
        total = None
        for p0 in range(0, F, L):
            part = np.cumsum(t[:, p0:p0 + L], axis=1)[:, -1]            # cumsum adds left to right, one rounding each
            total = part if total is None else total + part
        w[s] = total / TWO_PI
        b[s] = _bar(t, det, den, lll)
    return (w, b) if with_bar else w


def _bar(t, det, den, lll):
    nz = det != 0
    cond = np.where(nz, lll / np.where(nz, np.hypot(det, den), 1.0), 0.0)
    return 2.0 ** -52 * ((t.shape[1] + 16) * np.abs(t).sum(1) + 16 * cond.sum(1)) / (2 * np.pi)


def bar(points, verts, faces=None):
    """bar_q = 2^-52 [ (F + 16) sum_f |t_f| + 16 sum_{f: det != 0} la lb lc / hypot(det, den) ] / 2 pi, from the restatement.
    First term: F roundings of partial sums on each side, each at most 2^-53 of sum |t|, and an atan2 within 6 ulp per term
    on each side.  Second term: a perturbation of a few ulp of den or det (a sqrt that is not correctly rounded) moves t by at
    most delta / hypot(det, den), delta <= 8 2^-53 la lb lc for each."""
    return winding_f64(points, verts, faces, with_bar=True)[1]


def ulp_lengths(seed):
    """a `lengths` argument of pair_terms that moves each of the three lengths by a random -1, 0 or +1 ulp"""
    rng = np.random.default_rng(seed)

    def move(*ls):
        out = []
        for x in ls:
            k = rng.integers(-1, 2, x.shape)
            out.append(np.where(k > 0, np.nextafter(x, np.inf), np.where(k < 0, np.nextafter(x, -np.inf), x)))
        return out
    return move


# ---- the same formula at 40 digits ------------------------------------------------------------------------------------------
def winding_mp(points, verts, faces=None):
    """the formula of pair_terms in mpmath at 40 digits, the sum at 40 digits too -> (nq,) f64 (rounded once at the end)"""
    import mpmath
    q = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    tri = corners(verts, faces)
    with mpmath.workprec(140):
        mpf = np.frompyfunc(mpmath.mpf, 1, 1)
        sqrt = np.frompyfunc(mpmath.sqrt, 1, 1)
        atan2 = np.frompyfunc(lambda y, x: mpmath.mpf(0) if y == 0 else mpmath.atan2(y, x), 2, 1)
        T = mpf(tri)
        out = np.empty(len(q))
        for i in range(len(q)):
            A, B, C = (T[:, k] - mpf(q[i])[None, :] for k in range(3))
            la, lb, lc = sqrt(_dot(A, A)), sqrt(_dot(B, B)), sqrt(_dot(C, C))
            det = _dot(A, _cross(B, C))
            den = ((la * lb) * lc + _dot(A, B) * lc) + (_dot(B, C) * la + _dot(C, A) * lb)
            out[i] = float(mpmath.fsum(atan2(det, den)) / (2 * mpmath.pi))
    return out


# ---- an independent float64 form ----------------------------------------------------------------------------------------------
def _angle(u, v):
    """the angle between the vectors u and v, in [0, pi]"""
    c = np.cross(u, v)
    return np.arctan2(np.sqrt((c * c).sum(-1)), (u * v).sum(-1))


def winding_alt_f64(points, verts, faces=None):
    """Girard: the solid angle of a face is the spherical excess alpha + beta + gamma - pi of the triangle its corners' directions
    span on the unit sphere, the three angles being those between the planes through q and two corners; signed by the
    determinant of the directions.  A face seen edge on or with a corner at q (a plane normal vanishes, or det == 0) counts 0."""
    q, tri, blocks = _blocks(points, verts, faces)
    w = np.empty(len(q))
    for s in blocks:
        d = tri[None] - q[s, None, None, :]                              # (n,F,3,3)
        ln = np.sqrt((d * d).sum(-1, keepdims=True))
        u = d / np.where(ln > 0, ln, 1.0)
        a, b, c = u[:, :, 0], u[:, :, 1], u[:, :, 2]
        nab, nbc, nca = np.cross(a, b), np.cross(b, c), np.cross(c, a)
        excess = (_angle(nab, -nca) + _angle(nbc, -nab) + _angle(nca, -nbc)) - np.pi
        det = (d[:, :, 2] * np.cross(d[:, :, 0], d[:, :, 1])).sum(-1)
        flat = (det == 0) | (ln[..., 0] == 0).any(-1)
        for n in (nab, nbc, nca):
            flat |= (n == 0).all(-1)
        w[s] = np.where(flat, 0.0, np.sign(det) * excess).sum(1) / (4 * np.pi)
    return w


# ---- orientation -------------------------------------------------------------------------------------------------------------
def signed_volume(verts, faces=None):
    """sum_f (a - c0) . ((b - c0) x (c - c0)) in float64, c0 the centre of the vertices' box (six times the enclosed volume of
    a closed, outward mesh)"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    c0 = 0.5 * (v.min(0) + v.max(0))
    t = corners(verts, faces) - c0
    return float((t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum())


def mesh_orientation(verts, faces=None):
    return 1 if signed_volume(verts, faces) >= 0 else -1


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def flipped(faces):
    """the same faces with the opposite orientation"""
    return np.ascontiguousarray(np.asarray(faces)[:, ::-1])


def uv_sphere(segments=32, rings=16):
    """the unit sphere about the origin: `rings` bands of latitude, `segments` of longitude, a fan at either pole;
    2 segments (rings - 1) faces (960), normals outward -> (verts (V,3) f32, faces (F,3) i32)"""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                     np.repeat(np.cos(th)[:, None], segments, 1)], -1).reshape(-1, 3)
    verts = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]).astype(np.float32)
    south = len(verts) - 1
    faces = []
    for j in range(segments):
        k = (j + 1) % segments
        faces.append([0, 1 + j, 1 + k])
        for r in range(rings - 2):
            a, b, c, d = 1 + r * segments + j, 1 + (r + 1) * segments + j, 1 + (r + 1) * segments + k, 1 + r * segments + k
            faces += [[a, b, c], [a, c, d]]
        faces.append([south, 1 + (rings - 2) * segments + k, 1 + (rings - 2) * segments + j])
    return verts, np.array(faces, np.int32)


def open_sphere():
    """uv_sphere without its cap: the faces whose centroid has z <= 0.5"""
    verts, faces = uv_sphere()
    keep = verts.astype(np.float64)[faces].mean(1)[:, 2] <= 0.5
    return verts, np.ascontiguousarray(faces[keep])


def inside_queries():
    return np.random.default_rng(0).uniform(-1.3, 1.3, (3000, 3)).astype(np.float32)


def cube_expected():
    """the closed-form winding number of the unit cube at cube_tie_queries(): 8 vertices 1/8, 12 edge midpoints 1/4, 6 points on
    faces 1/2, 20 outside points 0"""
    return np.concatenate([np.full(8, 0.125), np.full(12, 0.25), np.full(6, 0.5), np.zeros(20)])


def concentric_cubes(delta=2.0 ** -5):
    """the unit cube, outward, and the cube [-delta, 1 + delta]^3 with its faces flipped -> ((va, fa), (vb, fb))"""
    vb = (CUBE_VERTS.astype(np.float64) * (1 + 2 * delta) - delta).astype(np.float32)
    return (CUBE_VERTS, CUBE_FACES), (vb, flipped(CUBE_FACES))


def iou_points():
    return (np.random.default_rng(1).random((20000, 3)) * 1.25 - 0.125).astype(np.float32)


def rotated_box():
    """an oriented box as metrics.oriented_bounds returns it -> (transform (4,4), extents (3,)): unequal extents, turned by 30
    degrees about z and then 20 about x, its centre at (0.7, -0.4, 1.1); the transform moves that centre to the origin and the
    box's edges onto the axes"""
    cz, sz, cx, sx = np.cos(np.pi / 6), np.sin(np.pi / 6), np.cos(np.pi / 9), np.sin(np.pi / 9)
    R = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.array([0.7, -0.4, 1.1])
    return T, np.array([1.0, 0.6, 0.35])


def box_draw(lo, hi, N, seed):
    """volume_iou's points in an axis-aligned box: default_rng(seed).random((N,3)) scaled in float64, rounded to fp32 once"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + np.random.default_rng(seed).random((int(N), 3)) * (hi - lo)).astype(np.float32)
