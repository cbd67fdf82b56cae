"""numpy restatement of the mesh rasteriser (csrc/raster.hip, cnr_amd/raster.py): every pixel against every
face in fp64, with the parenthesisation of include/cnr_hip.h, so that the kernels' face, label and depth images can be held to
it bit for bit; attributes, visibility, mesh culling and depth L1 restated the same way; and a brute-force Moeller-Trumbore
intersection in the world frame that shares none of those formulas, which the restatement itself is held to."""
import numpy as np


def pinhole_dirs(W, H, fx, fy, cx, cy):
    """the cameraInfo cache rows (W*H,3) float32, pixel (w,h) at row w H + h: ((w - cx) / fx, (h - cy) / fy, 1) in fp32"""
    d = np.ones((W, H, 3), np.float32)
    d[:, :, 0] = ((np.arange(W).astype(np.float32) - np.float32(cx)) / np.float32(fx))[:, None]
    d[:, :, 1] = ((np.arange(H).astype(np.float32) - np.float32(cy)) / np.float32(fy))[None, :]
    return d.reshape(-1, 3)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def face_records(verts, faces, T_cw):
    """-> n (F,3,3) = (n0, n1, n2), det (F,) of the fp32 verts under the fp64 world-to-camera matrix"""
    p = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]      # (F,3,3)
    T = np.asarray(T_cw, np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    v = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], -1)   # (F, corner, xyz)
    n = np.stack([_cross(v[:, 1], v[:, 2]), _cross(v[:, 2], v[:, 0]), _cross(v[:, 0], v[:, 1])], 1)
    det = (v[:, 0, 0] * n[:, 0, 0] + v[:, 0, 1] * n[:, 0, 1]) + v[:, 0, 2] * n[:, 0, 2]
    return n, det


def _edges(n, dirs):
    """e (P,F,3), S (P,F) for the records n (F,3,3) and the rays dirs (P,3) float32"""
    dx, dy = dirs[:, 0].astype(np.float64)[:, None, None], dirs[:, 1].astype(np.float64)[:, None, None]
    e = (n[None, :, :, 0] * dx + n[None, :, :, 1] * dy) + n[None, :, :, 2]
    return e, (e[..., 0] + e[..., 1]) + e[..., 2]


def rasterize(verts, faces, T_cw, dirs, W, H, zmin, zmax, cull_backfaces=False, face_ids=None, block=256):
    """No binning: -> dict(face (W,H) i32, -1 for none; t (W,H) f64, inf for none; depth (W,H) f32 = float32(t), 0 for none;
    bary (W,H,2) f64 = b1, b2 of the winner; margin (W,H) f64 = the smallest min_i |e_i| / |S| met among the faces whose plane
    the ray hits in front (s S > 0), inf when there is none).  ``face_ids``: test these faces only (ascending indices into
    ``faces``; the images still hold indices into ``faces``)."""
    faces = np.asarray(faces, np.int64)
    ids = np.arange(len(faces)) if face_ids is None else np.asarray(face_ids, np.int64)
    assert (np.diff(ids) > 0).all()
    P = W * H
    best_t, best_f = np.full(P, np.inf), np.full(P, -1, np.int64)
    best_b, margin = np.zeros((P, 2)), np.full(P, np.inf)
    rows = np.arange(P)
    with np.errstate(all="ignore"):
        for a in range(0, len(ids), block):
            sub = ids[a:a + block]
            n, det = face_records(verts, faces[sub], T_cw)
            s = np.where(det > 0, 1.0, -1.0)
            e, S = _edges(n, dirs)
            t = det[None] / S
            front = (s[None] * S > 0) & (det != 0)[None]
            cov = front & (s[None, :, None] * e >= 0).all(-1) & (t >= zmin) & (t <= zmax)
            if cull_backfaces:
                cov &= (det > 0)[None]
            m = np.where(front, np.abs(e).min(-1) / np.abs(S), np.inf)
            margin = np.minimum(margin, m.min(1, initial=np.inf))
            tc = np.where(cov, t, np.inf)
            j = tc.argmin(1)                    # the first of equal minima: the lowest face index of the block
            tj = tc[rows, j]
            upd = tj < best_t                   # strict: earlier blocks hold lower indices
            best_t[upd], best_f[upd] = tj[upd], sub[j[upd]]
            best_b[upd] = np.stack([e[rows, j, 1] / S[rows, j], e[rows, j, 2] / S[rows, j]], -1)[upd]
    hit = best_f >= 0
    depth = np.where(hit, best_t, 0.0).astype(np.float32)
    return dict(face=best_f.astype(np.int32).reshape(W, H), t=best_t.reshape(W, H), depth=depth.reshape(W, H),
                bary=best_b.reshape(W, H, 2), margin=margin.reshape(W, H))


def moller_trumbore(verts, faces, T_wc, dirs, W, H, zmin, zmax, block=256):
    """Brute force in the world frame: ray o + tt D, o the camera centre, D = R_wc d, against p0 + u e1 + v e2.  D's camera-frame
    z is 1, so tt is the z-depth.  -> face (W,H) i32, t (W,H) f64 (inf for none): nearest hit, lowest index among equals"""
    T = np.asarray(T_wc, np.float64)
    p = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    o, D = T[:3, 3], dirs.astype(np.float64) @ T[:3, :3].T                       # (P,3)
    P = W * H
    best_t, best_f = np.full(P, np.inf), np.full(P, -1, np.int64)
    rows = np.arange(P)
    with np.errstate(all="ignore"):
        for a in range(0, len(p), block):
            q = p[a:a + block]
            e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
            pvec = np.cross(D[:, None], e2[None])                                  # (P,F,3)
            det = (pvec * e1[None]).sum(-1)
            tvec = o[None] - q[:, 0]                                               # (F,3)
            u = (pvec * tvec[None]).sum(-1) / det
            qvec = np.cross(tvec, e1)                                              # (F,3)
            v = (D[:, None] * qvec[None]).sum(-1) / det
            tt = (e2 * qvec).sum(-1)[None] / det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt >= zmin) & (tt <= zmax)
            tc = np.where(ok, tt, np.inf)
            j = tc.argmin(1)
            tj = tc[rows, j]
            upd = tj < best_t
            best_t[upd], best_f[upd] = tj[upd], a + j[upd]
    return best_f.astype(np.int32).reshape(W, H), best_t.reshape(W, H)


def _unit(g):
    with np.errstate(all="ignore"):
        ln = np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])
        ok = (ln > 0) & np.isfinite(ln)
        return np.where(ok[..., None], g / np.where(ok, ln, 1.0)[..., None], 0.0)


def attributes(verts, faces, colors, normals, face_label, T_cw, dirs, face_img, normal="face"):
    """from the face image (W,H): -> rgb (W,H,3) f64, instance (W,H) i32, normal (W,H,3) f64, as cnr_raster_attributes"""
    W, H = face_img.shape
    faces = np.asarray(faces, np.int64)
    f = face_img.reshape(-1).astype(np.int64)
    hit = f >= 0
    fi = np.where(hit, f, 0)
    n, _ = face_records(verts, faces, T_cw)
    dx, dy = dirs[:, 0].astype(np.float64), dirs[:, 1].astype(np.float64)
    nn = n[fi]                                                                    # (P,3,3)
    with np.errstate(all="ignore"):
        e = (nn[:, :, 0] * dx[:, None] + nn[:, :, 1] * dy[:, None]) + nn[:, :, 2]
        S = (e[:, 0] + e[:, 1]) + e[:, 2]
        b = e / S[:, None]
    idx = faces[fi]                                                               # (P,3)
    col = np.asarray(colors, np.float32).astype(np.float64)[idx]                   # (P,3,3)
    rgb = (b[:, 0, None] * col[:, 0] + b[:, 1, None] * col[:, 1]) + b[:, 2, None] * col[:, 2]
    if normal == "vertex":
        nv = np.asarray(normals, np.float32).astype(np.float64)[idx]
        g = (b[:, 0, None] * nv[:, 0] + b[:, 1, None] * nv[:, 1]) + b[:, 2, None] * nv[:, 2]
    else:
        p = np.asarray(verts, np.float32).astype(np.float64)[idx]
        g = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        T = np.asarray(T_cw, np.float64)
        dw = np.stack([(T[0, k] * dx + T[1, k] * dy) + T[2, k] for k in range(3)], -1)
        flip = (g[:, 0] * dw[:, 0] + g[:, 1] * dw[:, 1]) + g[:, 2] * dw[:, 2] > 0
        g = np.where(flip[:, None], -g, g)
    nrm = _unit(g)
    inst = np.where(hit, np.asarray(face_label, np.int64)[fi], -1).astype(np.int32)
    return (np.where(hit[:, None], rgb, 0.0).reshape(W, H, 3), inst.reshape(W, H), np.where(hit[:, None], nrm, 0.0).reshape(W, H, 3))


def visible(face_imgs, depth_imgs, F, depth_obs=None, tol=0.0):
    """face_imgs (V,W,H) i32, depth_imgs (V,W,H) f32 -> seen bool (F,), count i32 (F,) = the views in which the face won a
    pixel; with depth_obs (V,W,H) f32 only pixels with depth_obs > 0 and float64(depth) <= float64(depth_obs) + tol count"""
    seen, count = np.zeros(F, bool), np.zeros(F, np.int32)
    for v in range(len(face_imgs)):
        ok = face_imgs[v] >= 0
        if depth_obs is not None:
            ok &= (depth_obs[v] > 0) & (depth_imgs[v].astype(np.float64) <= depth_obs[v].astype(np.float64) + float(tol))
        won = np.unique(face_imgs[v][ok])
        seen[won] = True
        count[won] += 1
    return seen, count


def cull_mesh(verts, faces, colors, normals, keep):
    """the kept faces with compacted vertices (old order kept): -> verts, faces, colors, normals"""
    keep = np.asarray(keep)
    keep = np.nonzero(keep)[0] if keep.dtype == np.bool_ else keep.astype(np.int64)
    new_index, used, out_faces = {}, [], []
    kept = [tuple(int(i) for i in faces[k]) for k in keep]
    for i in sorted({i for fc in kept for i in fc}):
        new_index[i] = len(used)
        used.append(i)
    for fc in kept:
        out_faces.append([new_index[i] for i in fc])
    used = np.array(used, np.int64)
    return (np.asarray(verts)[used], np.array(out_faces, np.int64).reshape(-1, 3), np.asarray(colors)[used], np.asarray(normals)[used])


def depth_l1(d_rec, d_gt):
    """depth images of any equal shape, 0 = nothing hit -> dict(l1, both, only_rec, only_gt, neither)"""
    a, b = np.asarray(d_rec, np.float32), np.asarray(d_gt, np.float32)
    ha, hb = a > 0, b > 0
    both = ha & hb
    nb = int(both.sum())
    l1 = float(np.abs(a.astype(np.float64) - b.astype(np.float64))[both].sum() / nb) if nb else float("nan")
    return dict(l1=l1, both=nb, only_rec=int((ha & ~hb).sum()), only_gt=int((~ha & hb).sum()), neither=int((~ha & ~hb).sum()))


# ---- fixtures shared by the host and the GPU tests ---------------------------------------------------------------------------
W0, H0 = 50, 37
SOUP_CAM = dict(W=W0, H=H0, fx=40.0, fy=40.0, cx=24.5, cy=18.0, zmin=0.1, zmax=10.0)


def soup(seed=11, n=120):
    """random triangles around the camera: centres in [-1.5,1.5] x [-1,1] x [-0.5,6], corner noise sigma 0.5, rounded to fp32;
    some cross the camera plane, some lie behind it.  -> verts (3n,3) f32, faces (n,3) i64"""
    rng = np.random.default_rng(seed)
    c = rng.uniform([-1.5, -1.0, -0.5], [1.5, 1.0, 6.0], (n, 3))
    v = (c[:, None] + rng.normal(0.0, 0.5, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * n).reshape(n, 3)


def random_rigid(seed=5):
    """a random rigid T_wc (4,4) float64"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-2.0, 2.0, 3)
    return T


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """T_wc (4,4) of a camera at ``eye`` whose optical axis (+z) goes to ``target``, x right, y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T


def ring_poses(n, radius, height, target=(0.5, 0.5, 0.5)):
    """n poses on a circle of ``radius`` around ``target`` at ``height`` above it, looking at it"""
    t = np.asarray(target, np.float64)
    return np.stack([look_at(t + [radius * np.cos(a), radius * np.sin(a), height], t)
                     for a in 2 * np.pi * np.arange(n) / n])


def sphere_volume(D, radius, center=0.5):
    """(D,D,D) float32 occupancy-like volume, > 0.5 inside the sphere of ``radius`` around ``center`` in [0,1]^3 units"""
    g = np.linspace(0.0, 1.0, D)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    r = np.sqrt((x - center) ** 2 + (y - center) ** 2 + (z - center) ** 2)
    return (0.5 + (radius - r)).astype(np.float32)


DYADIC_CAM = dict(W=32, H=24, fx=32.0, fy=32.0, cx=16.0, cy=12.0, zmin=0.5, zmax=8.0)


def dyadic_point(w, h, z):
    """the camera-frame point that pixel (w, h) of DYADIC_CAM sees at depth z: exact in fp32 for dyadic z and integer w, h"""
    return [(w - 16.0) / 32.0 * z, (h - 12.0) / 32.0 * z, z]
