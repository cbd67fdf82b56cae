"""TEST INFRASTRUCTURE: the scene view pipeline restated in numpy from its formulas (include/cnr_hip.h, cnr_view_*), every
function parametrised by `dtype`: float64 is the truth, float32 the yardstick of modular_cases.check -- the same
restatement in the kernels' own precision, its sums written in the kernels' order of operations.

    segments(T_wc, dirs, to_box, zmin, zmax, dtype)        slab test per (pixel, entity), (entity, pixel) order, pix_segs
    points(T_wc, dirs, to_field, seg, S, dtype)            uniform midpoints and their positions in the field frames
    composite(sigma, color, z, pix_segs, seg_entity, entity_inst, thr, dtype)   the merged per-pixel alpha composite
    box_affine(centre, R, half) / rot(axis, angle) / pinhole_dirs(W, H, f, cx, cy)   scene builders for the tests
"""
import numpy as np

KMAX = 8


def rot(axis, angle):
    """Rodrigues rotation matrix (float64)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def box_affine(centre, R, half):
    """to_box (3,4) float64 of the box {centre + R (half * u), u in [-1,1]^3}: diag(1/half) R^T [I | -centre]"""
    A = np.diag(1.0 / np.asarray(half, np.float64)) @ np.asarray(R, np.float64).T
    return np.concatenate([A, -(A @ np.asarray(centre, np.float64))[:, None]], 1)


def pinhole_dirs(W, H, f, cx, cy):
    """(W*H, 3) float32 directions ((w - cx) / f, (h - cy) / f, 1), pixel index w * H + h (cnr_camera_rays)"""
    w, h = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="ij")
    d = np.stack([(w - np.float32(cx)) / np.float32(f), (h - np.float32(cy)) / np.float32(f), np.ones_like(w)], -1)
    return d.reshape(-1, 3).astype(np.float32)


def _affine(A, x, with_t=True):
    """rows of A (3,4) applied to points x (...,3), summed left to right"""
    out = [A[k, 0] * x[..., 0] + A[k, 1] * x[..., 1] + A[k, 2] * x[..., 2] + (A[k, 3] if with_t else 0) for k in range(3)]
    return np.stack(out, -1)


def slab(T_wc, dirs, to_box, zmin, zmax, dtype):
    """-> hit (E,P) bool, zn (E,P), zf (E,P) in `dtype`"""
    T, d, A = np.asarray(T_wc, dtype), np.asarray(dirs, dtype), np.asarray(to_box, dtype)
    R = np.concatenate([T[:3, :3], np.zeros((3, 1), dtype)], 1)
    dw = _affine(R, d, with_t=False)                                  # (P,3) world directions
    E, P = A.shape[0], d.shape[0]
    hit, zn, zf = np.zeros((E, P), bool), np.zeros((E, P), dtype), np.zeros((E, P), dtype)
    one = dtype(1.0)
    for e in range(E):
        o = _affine(A[e], T[:3, 3])                                   # (3,)
        db = _affine(A[e], dw, with_t=False)                          # (P,3)
        near, far, ok = np.full(P, zmin, dtype), np.full(P, zmax, dtype), np.ones(P, bool)
        for k in range(3):
            zero = db[:, k] == 0
            ok &= ~zero | (abs(o[k]) <= one)
            safe = np.where(zero, one, db[:, k])
            t1, t2 = (-one - o[k]) / safe, (one - o[k]) / safe
            near = np.where(zero, near, np.maximum(near, np.minimum(t1, t2)))
            far = np.where(zero, far, np.minimum(far, np.maximum(t1, t2)))
        hit[e], zn[e], zf[e] = ok & (far > near), near, far
    return hit, zn, zf


def segments(T_wc, dirs, to_box, zmin, zmax, dtype, hit=None):
    """cnr_view_segments_count / _emit.  `hit`: take this hit set (E,P) instead of the own one (to compare z of one precision
    on the hit set of the other)."""
    own, zn, zf = slab(T_wc, dirs, to_box, dtype(zmin), dtype(zmax), dtype)
    hit = own if hit is None else hit
    E, P = hit.shape
    ent, pix = np.nonzero(hit)                                        # row-major: (entity, pixel) order
    N = len(ent)
    seg_z = np.stack([zn[ent, pix], zf[ent, pix]], -1).astype(dtype).reshape(N, 2)
    entity_offset = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.int64)
    pix_segs = np.full((P, KMAX), -1, np.int32)
    overflow = 0
    for p in range(P):
        s = np.nonzero(pix == p)[0]                                   # ascending segment index = entity order
        if len(s) > KMAX:
            overflow += 1
            keep = np.sort(s[np.argsort(seg_z[s, 0], kind="stable")[:KMAX]])     # nearest by z_near, ties: the earlier entity
            s = keep
        pix_segs[p, :len(s)] = s
    return dict(hit=hit, seg_pixel=pix.astype(np.int32), seg_entity=ent.astype(np.int32), seg_z=seg_z,
                entity_offset=entity_offset, pix_segs=pix_segs, overflow=overflow, N=N)


def points(T_wc, dirs, to_field, seg_pixel, seg_entity, seg_z, S, dtype):
    """cnr_view_points -> z (N,S), pts (N,S,3)"""
    T, d, F, sz = np.asarray(T_wc, dtype), np.asarray(dirs, dtype), np.asarray(to_field, dtype), np.asarray(seg_z, dtype)
    i = np.arange(S, dtype=dtype)[None, :]
    zn, zf = sz[:, :1], sz[:, 1:]
    z = zn + (i + dtype(0.5)) * (zf - zn) / dtype(S)
    c = z[..., None] * d[seg_pixel][:, None, :]                       # camera-frame points (N,S,3)
    w = _affine(T[:3], c)
    Fe = F[seg_entity]                                                # (N,3,4)
    pts = np.stack([Fe[:, None, k, 0] * w[..., 0] + Fe[:, None, k, 1] * w[..., 1] + Fe[:, None, k, 2] * w[..., 2] + Fe[:, None, k, 3]
                    for k in range(3)], -1)
    return z.astype(dtype), pts.astype(dtype)


def composite(sigma, color, z, pix_segs, seg_entity, entity_inst, thr, dtype):
    """cnr_view_composite: per pixel the samples of its segments ordered by (z, position in the pix_segs row, sample index)."""
    sigma, color, z = np.asarray(sigma, dtype), np.asarray(color, dtype), np.asarray(z, dtype)
    P, S = pix_segs.shape[0], sigma.shape[1] if sigma.ndim == 2 else 0
    out = dict(rgb=np.zeros((P, 3), dtype), depth=np.zeros(P, dtype), opacity=np.zeros(P, dtype), var=np.zeros(P, dtype),
               mass=np.zeros((P, KMAX), dtype), instance=np.full(P, -1, np.int32))
    one, eps = dtype(1.0), dtype(1e-10)
    for p in range(P):
        segs = [int(s) for s in pix_segs[p] if s >= 0]
        if not segs:
            continue
        K = len(segs)
        zz = np.concatenate([z[s] for s in segs])
        kk = np.repeat(np.arange(K), S)
        ii = np.tile(np.arange(S), K)
        order = np.lexsort((ii, kk, zz))                              # last key first: z, then segment, then sample
        with np.errstate(over="ignore"):                            # exp(200) = inf in float32: occupancy 0, as in the kernel
            occ = one / (one + np.exp(-np.concatenate([sigma[s] for s in segs])))
        col = np.concatenate([color[s] for s in segs])
        occ, col, zz, kk = occ[order], col[order], zz[order], kk[order]
        free = one - occ + eps
        T = np.concatenate([[one], np.cumprod(free)[:-1]]).astype(dtype)
        term = (occ * T).astype(dtype)
        depth = (term * zz).sum(dtype=dtype)
        out["rgb"][p] = (term[:, None] * col).sum(0, dtype=dtype)
        out["depth"][p], out["opacity"][p] = depth, term.sum(dtype=dtype)
        out["var"][p] = (term * (zz - depth) ** 2).sum(dtype=dtype)
        mass = np.array([term[kk == k].sum(dtype=dtype) for k in range(K)], dtype)
        out["mass"][p, :K] = mass
        if out["opacity"][p] >= dtype(thr):
            out["instance"][p] = entity_inst[seg_entity[segs[int(np.argmax(mass))]]]     # argmax: the first maximum
    return out
