"""numpy restatement of csrc/metric.hip and the metric formulas of metric/metrics.py: area-weighted sampling from the same
uniforms (np.cumsum + np.searchsorted, the reflected barycentric point in fp64), clipping to a box of six planes (the same
Sutherland-Hodgman in fp64, fan triangulation, (face, fan) order), and the distances by scipy's cKDTree in float64."""
import numpy as np
from scipy.spatial import cKDTree


def triangles(verts, faces=None):
    """(F,3,3) f64 corners of an indexed mesh, or of a soup when faces is None"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    return v.reshape(-1, 3, 3) if faces is None else v[np.asarray(faces, np.int64)]


def face_areas(tri):
    c = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return 0.5 * np.sqrt((c * c).sum(1))


def sample_surface(tri, u):
    """-> (face index (n,), points (n,3) f32, cum (F,)) for uniforms u (n,3) f64"""
    cum = np.cumsum(face_areas(tri))
    face = np.minimum(np.searchsorted(cum, u[:, 0] * cum[-1], side="left"), len(tri) - 1)
    ab = u[:, 1:].copy()
    flip = ab.sum(1) > 1.0
    ab[flip] = np.abs(ab[flip] - 1.0)
    t = tri[face]
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    pts = e1 * ab[:, :1] + e2 * ab[:, 1:] + t[:, 0]
    return face, pts.astype(np.float32), cum


def _clip_polygon(P, planes, seen):
    """seen: a one-element list holding the smallest |dist| evaluated so far, over the original and intermediate vertices"""
    for h in planes:
        d = (P - h[:3]) @ h[3:]
        seen[0] = min(seen[0], float(np.abs(d).min()))
        if (d >= 0).all():
            continue
        Q = []
        n = len(P)
        for i in range(n):
            j = (i + 1) % n
            if d[i] >= 0:
                Q.append(P[i])
            if (d[i] >= 0) != (d[j] >= 0):
                t = d[i] / (d[i] - d[j])
                Q.append(P[i] + (P[j] - P[i]) * t)
        P = np.array(Q).reshape(-1, 3)
        if len(P) == 0:
            break
    return P if len(P) >= 3 else P[:0]


def clip_box_info(tri, planes):
    """-> (triangles (T,3,3) f64, triangles per face (F,), the smallest |(x - o) . n| evaluated): the triangles' parts inside all
    six planes (origin, inward normal rows), fan-triangulated from the polygon's first vertex, in (face, fan) order.  The
    smallest |dist| runs over every vertex, original or intermediate, at every plane it was tested against: while it is far
    above the rounding of a dist, every kept / dropped decision is the same in any fp64 evaluation."""
    planes = np.asarray(planes, np.float64)
    tri = np.asarray(tri, np.float64)
    d = ((tri[:, :, None, :] - planes[None, None, :, :3]) * planes[None, None, :, 3:]).sum(-1)
    inside = (d >= 0).all((1, 2))
    seen = [float(np.abs(d[inside]).min()) if inside.any() else np.inf]
    out, counts = [], np.zeros(len(tri), np.int64)
    for f in range(len(tri)):
        if inside[f]:
            out.append(tri[f][None])
            counts[f] = 1
            continue
        P = _clip_polygon(tri[f], planes, seen)
        if len(P):
            out.append(np.stack([np.stack([P[0], P[k], P[k + 1]]) for k in range(1, len(P) - 1)]))
            counts[f] = len(P) - 2
    return (np.concatenate(out, 0) if out else np.zeros((0, 3, 3))), counts, seen[0]


def clip_box(tri, planes):
    """-> (T,3,3) f64: clip_box_info's triangles"""
    return clip_box_info(tri, planes)[0]


def nn_dist(q, p):
    return cKDTree(np.asarray(p, np.float64)).query(np.asarray(q, np.float64))[0]


def accuracy(gt, rec):
    return float(np.mean(nn_dist(rec, gt)))


def completion(gt, rec):
    return float(np.mean(nn_dist(gt, rec)))


def accuracy_ratio(gt, rec, dist_th=0.01):
    return float(np.mean((nn_dist(rec, gt) < dist_th).astype(np.float64)))


def completion_ratio(gt, rec, dist_th=0.01):
    return float(np.mean((nn_dist(gt, rec) < dist_th).astype(np.float64)))


def chamfer(gt, rec):
    return (completion(gt, rec) + accuracy(gt, rec)) / 2.0


# ---- fixtures shared by test_metrics_host.py (which proves their conditions from the restatement) and test_metrics_gpu.py -------
def random_box(rng, centre, ext):
    """a randomly rotated box -> (transform (4,4) moving the box to the origin, extents (3,))"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, -q @ np.asarray(centre)
    return T, np.asarray(ext, np.float64)


CLIP_SOUP_FACES = (1, 63, 64, 65, 255, 256, 257, 1000)       # a wave (64) and a block (256) that end inside the face list


def clip_soup_cases():
    """general position: random soups (F*3,3) f32 of CLIP_SOUP_FACES faces, each with a random rotated box that cuts it
    -> [(F, verts, transform, extents)]"""
    rng = np.random.default_rng(21)
    out = []
    for F in CLIP_SOUP_FACES:
        v = (rng.normal(size=(3 * F, 3)) * 0.5).astype(np.float32)
        if F == 1:                                            # a single face has to cross the box: one corner inside, two far out
            v = np.array([[0.05, -0.02, 0.03], [1.3, 0.4, -0.2], [-0.3, 1.1, 0.6]], np.float32)
        T, ext = random_box(rng, rng.normal(size=3) * 0.05, (0.7, 0.8, 0.9))
        out.append((F, v, T, ext))
    return out


UNIT_BOX = (np.eye(4), np.ones(3))                            # planes at +-0.5 with axis normals


def hexagon_triangle(r=0.66, turn=0.0, lift=(0.0, 0.0, 0.0)):
    """A triangle that the unit cube clips to 9 vertices (7 fan triangles).  The plane x + y + z = 0 cuts the cube in a regular
    hexagon with corners at the permutations of (1/2, -1/2, 0), circumradius sqrt(1/2) = 0.707 and inradius 0.612; a triangle
    in that plane with inradius r between the two, its edges facing alternate corners, cuts those three corners off and keeps
    the other three.  `turn` (radians, about the plane's normal) and `lift` (added to the corners) move it off the symmetric
    position, so that nothing lies exactly on a cube face."""
    c = np.array([[0.5, -0.5, 0.0], [0.0, 0.5, -0.5], [-0.5, 0.0, 0.5]])
    d = c / np.linalg.norm(c, axis=1, keepdims=True)
    n = np.ones(3) / np.sqrt(3.0)
    tri = -2.0 * r * d
    tri = tri * np.cos(turn) + np.cross(n, tri) * np.sin(turn)
    return tri + np.asarray(lift, np.float64).reshape(-1, 3)


def fan_soup():
    """a soup (F*3,3) f32 against UNIT_BOX whose faces clip to every triangle count from 0 to 7: corners from N(0, 1) give 0 to
    6, hexagon_triangle gives 7; shuffled, so that neighbouring lanes carry different counts"""
    rng = np.random.default_rng(33)
    tris = [rng.normal(size=(2041, 3, 3))]
    for k in range(8):
        tris.append(hexagon_triangle(0.64 + 0.005 * k, 0.01 * (k - 3.5), rng.normal(size=(3, 3)) * 2e-3)[None])
    tris = np.concatenate(tris)
    return tris[rng.permutation(len(tris))].reshape(-1, 3).astype(np.float32)


def on_plane_soup():
    """Triangles with corners at multiples of 1/8 against UNIT_BOX, so every dist is exact and `>=` alone decides; every edge
    that crosses a plane does so at a dyadic parameter, so the intersections are exact too.  The triangle counts are what
    Sutherland-Hodgman with `>=` gives by hand: a corner or an edge that only touches the box survives as zero-area triangles.
    -> (verts (F*3,3) f32, triangles per face)"""
    t = [
        ([[0.5, -0.25, -0.25], [0.5, 0.25, -0.25], [0.5, 0.0, 0.25]], 1),            # lying in the face x = 1/2: kept whole
        ([[-0.5, -0.25, 0.125], [-0.5, 0.25, 0.125], [-0.75, 0.0, 0.125]], 2),       # an edge in x = -1/2, the third corner outside:
                                                                                     # the edge twice over, two zero-area triangles
        ([[-0.5, -0.25, 0.125], [-0.5, 0.25, 0.125], [-0.25, 0.0, 0.125]], 1),       # the same edge, the third corner inside
        ([[0.5, 0.125, 0.0], [0.75, 0.25, 0.125], [0.75, 0.0, -0.125]], 1),          # one corner touches x = 1/2 from outside: that
                                                                                     # corner three times, a zero-area triangle
        ([[0.125, 0.5, 0.5], [0.375, 0.75, 0.75], [-0.125, 0.75, 0.625]], 1),        # a corner on the box edge y = z = 1/2, from outside
        ([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [0.25, 0.5, 0.25]], 1),               # a corner on the box corner, the rest inside
        ([[-0.5, -0.5, -0.5], [-0.75, -0.5, -0.25], [-0.75, -0.25, -0.5]], 1),       # touches the box corner from outside
        ([[0.25, 0.0, 0.0], [0.75, 0.0, 0.0], [0.25, 0.25, 0.0]], 2),                # crosses x = 1/2 at t = 1/2 on both edges
        ([[0.0, 0.5, 0.25], [0.0, 0.25, 0.0], [0.0, 0.75, 0.0]], 2),                 # a corner on y = 1/2, one edge crosses there
        ([[0.0, 0.0, 0.5], [0.25, 0.0, 0.5], [0.0, 0.25, 0.75]], 2),                 # an edge in z = 1/2, the third corner outside
    ]
    verts = np.array([c for c, _ in t], np.float64).reshape(-1, 3)
    assert np.array_equal(verts * 8, np.round(verts * 8))
    return verts.astype(np.float32), np.array([k for _, k in t], np.int64)


def dyadic_sampling_fixture():
    """Right triangles in planes z = const with power-of-two legs along x and y, zero-area faces at the start, in the middle
    and at the end, areas that add to a power of two: every area, every prefix, u0 * total and every sampled point are exact
    in fp64 in any evaluation order, fused or not.  u0 runs over 0, every prefix boundary / total, the values one ulp below
    and above each, and 1 - 2^-53; (a, b) over dyadic pairs that include a + b == 1 (not reflected) and a + b == 1 + 2^-52
    (reflected).  -> (verts (F*3,3) f32 soup, u (n,3) f64)"""
    legs = [(0, 0), (2, 2), (-2, 1), (0, 4), (0, 0), (1, 0), (1, 1), (-1, -0.5), (0.5, 1), (4, -2), (0, 0)]
    areas = [0.5 * abs(a * b) for a, b in legs]
    assert sum(areas) == 8.0
    verts = []
    for k, (a, b) in enumerate(legs):
        o = np.array([k - 3.0, 0.0, 0.25 * k])                 # y from 0: b may carry last-place bits
        verts += [o, o + [a, 0, 0], o + [0, b, 0]]
    u = _dyadic_uniforms(np.cumsum(areas))
    return np.array(verts, np.float32), u


def dyadic_single_face():
    """F = 1: one right triangle of area 2 -> (verts (3,3) f32, u)"""
    return np.array([[1, 0, 3], [3, 0, 3], [1, 2, 3]], np.float32), _dyadic_uniforms(np.array([2.0]))


def _dyadic_uniforms(cum):
    total = cum[-1]
    u0 = [0.0, 1.0 - 2.0 ** -53, 0.5, 0.3125]
    for c in np.unique(cum):
        for v in (c / total, np.nextafter(c / total, -1.0), np.nextafter(c / total, 2.0)):
            if 0.0 <= v < 1.0:
                u0.append(float(v))
    ab = [(0.0, 0.0), (0.25, 0.5), (0.5, 0.5), (0.25, 0.75), (1.0, 0.0), (0.5, 0.5 + 2.0 ** -52),
          (0.75, 0.75), (0.875, 0.125 + 2.0 ** -52), (0.0, 1.0 - 2.0 ** -53), (0.625, 0.0)]
    return np.array([[x, a, b] for x in u0 for a, b in ab], np.float64)


SAMPLING_SEED = 4


def sampling_near_boundaries(tri, u):
    """the samples whose u0 * total lies within 1e-12 (relative to the total) of the prefix boundary on either side of their
    face: there a last-place difference in the prefix could pick the neighbouring face -> (face, points, cum, near mask)"""
    face, pts, cum = sample_surface(tri, u)
    target = u[:, 0] * cum[-1]
    near = np.abs(cum[np.minimum(face, len(cum) - 1)] - target) < 1e-12 * cum[-1]
    near |= np.abs(cum[np.maximum(face - 1, 0)] - target) < 1e-12 * cum[-1]
    return face, pts, cum, near


def sampling_random_inputs():
    """the random part of the sampling comparison -> (soup vertices (300,3), its faces (500,3), three (20000,3) uniform draws:
    one per mesh of the comparison, the soup last)"""
    rng = np.random.default_rng(SAMPLING_SEED)
    v = rng.normal(size=(300, 3)) * 2 + 4
    f = rng.integers(0, 300, (500, 3))
    return v, f, [rng.random((20000, 3)) for _ in range(3)]
