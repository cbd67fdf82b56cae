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


def _clip_polygon(P, planes):
    for h in planes:
        d = (P - h[:3]) @ h[3:]
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


def clip_box(tri, planes):
    """-> (T,3,3) f64: the triangles' parts inside all six planes (origin, inward normal rows), fan-triangulated"""
    planes = np.asarray(planes, np.float64)
    d = np.einsum("fkc,pc->fkp", tri, planes[:, 3:]) - (planes[:, :3] * planes[:, 3:]).sum(1)
    inside = (d >= 0).all((1, 2))
    out = []
    for f in range(len(tri)):
        if inside[f]:
            out.append(tri[f][None])
            continue
        P = _clip_polygon(tri[f], planes)
        if len(P):
            out.append(np.stack([np.stack([P[0], P[k], P[k + 1]]) for k in range(1, len(P) - 1)]))
    return np.concatenate(out, 0) if out else np.zeros((0, 3, 3))


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
