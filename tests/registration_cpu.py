"""TEST INFRASTRUCTURE: numpy / scipy restatement of csrc/pointcloud.hip and of the registration path built on it (DESIGN.md
§3.9): unprojection, open3d's voxel down-sample, point-to-point ICP with a cKDTree, the default solver's scheme and
align_poses' bookkeeping.  Everything is fp64; clouds are kept as the fp32 values the product stores."""
import numpy as np
from scipy.spatial import cKDTree

DEPTH_TRUNC = 8.0


# ---- unprojection and down-sampling ------------------------------------------------------------------------------------
def unproject(sample, inst_id, fx, fy, cx, cy, T_WC=None):
    """one frame of sample_dict -> (kept flat indices in the (W,H) arrays' memory order, points (n,3) f64, colors (n,3) f64)"""
    depth, mask, image = sample["depth"], sample["obj_mask"], sample["image"]
    W, H = depth.shape
    keep = (mask == inst_id) & (depth > 0) & (depth <= np.float32(DEPTH_TRUNC))
    idx = np.flatnonzero(keep.reshape(-1))
    u, v, z = (idx // H).astype(np.float64), (idx % H).astype(np.float64), depth.reshape(-1)[idx].astype(np.float64)
    cam = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z, np.ones_like(z)], 1)
    T = np.asarray(sample["T"] if T_WC is None else T_WC, np.float64)
    return idx, (cam @ T.T)[:, :3], image.reshape(-1, 3)[idx].astype(np.float64) / 255.0


def voxel_down_sample(points, colors, voxel):
    """points (n,3) fp32 values -> (means (m,3) f64, colour means or None, keys (m,) i64, counts), voxels ascending in (ix, iy, iz)"""
    p = np.asarray(points, np.float32).astype(np.float64)
    mn = p.min(0) - voxel / 2
    ijk = np.floor((p - mn) / voxel).astype(np.int64)
    keys = (ijk[:, 0] << 42) | (ijk[:, 1] << 21) | ijk[:, 2]
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    heads = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    counts = np.diff(np.r_[heads, len(sk)])
    # one call, so a million voxels take half a second.  reduceat adds a run's rows one after another in input order (the sort is
    # stable); a[run].sum(0) may group them otherwise, so the two agree to rounding (a few 2^-53 relative), not bit for bit
    mean =lambda a: np.add.reduceat(a[order], heads, axis=0) / counts[:, None]
    return mean(p), None if colors is None else mean(np.asarray(colors, np.float32).astype(np.float64)), sk[heads], counts


class CpuCloud:
    """host stand-in of utils.PointCloud: fp32 values, fp64 arithmetic, cKDTree distances"""

    def __init__(self, points, colors=None):
        self.p32 = np.asarray(points, np.float32).reshape(-1, 3)
        self.c32 = None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)

    @property
    def points(self):
        return self.p32.astype(np.float64)

    def voxel_down_sample(self, v):
        p, c, _, _ = voxel_down_sample(self.p32, self.c32, v)
        return CpuCloud(p, c)

    def compute_point_cloud_distance(self, other):
        return cKDTree(other.points).query(self.points)[0]


# ---- ICP ---------------------------------------------------------------------------------------------------------------
def transform32(T, src):
    """f32(T . src) as cnr_icp_step defines the transformed source"""
    s = np.asarray(src, np.float32).astype(np.float64)
    return (s @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def icp_sums(src, tgt, T, index, dist, max_corr):
    """the 17 sums from given correspondences -> (sums, sums of the absolute values of the terms)"""
    a = transform32(T, src).astype(np.float64)
    b = np.asarray(tgt, np.float32).astype(np.float64)[index]
    keep = np.asarray(dist, np.float32) < np.float32(max_corr)
    a, b, d = a[keep], b[keep], np.asarray(dist, np.float32)[keep].astype(np.float64)
    terms = np.concatenate([np.ones((len(a), 1)), (d * d)[:, None], a, b, (a[:, :, None] * b[:, None, :]).reshape(-1, 9)], 1)
    return terms.sum(0), np.abs(terms).sum(0)


def kabsch(sums):
    """R = V diag(1, 1, det(V U^T)) U^T of H = sum (a - ca)(b - cb)^T = U S V^T, t = cb - R ca -> (4,4)"""
    n, ca, cb = sums[0], sums[2:5] / sums[0], sums[5:8] / sums[0]
    H = sums[8:17].reshape(3, 3) - n * np.outer(ca, cb)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ np.diag([1.0, 1.0, np.linalg.det(Vt.T @ U.T)]) @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cb - R @ ca
    return T


def icp(src, tgt, T0, max_corr, max_iteration=100):
    """open3d's point-to-point loop from one start, all fp64 -> (T, fitness, rmse, updates)"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    tree, T, prev = cKDTree(tgt), np.array(T0, np.float64), None
    for it in range(max_iteration + 1):
        a = src @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(a)
        keep = d < max_corr
        n = int(keep.sum())
        fitness, rmse = n / len(src), (np.sqrt((d[keep] ** 2).sum() / n) if n else 0.0)
        if prev is not None and abs(fitness - prev[0]) < 1e-6 and abs(rmse - prev[1]) < 1e-6:
            break
        prev = (fitness, rmse)
        if n < 3 or it == max_iteration:
            break
        a, b = a[keep], tgt[j[keep]]
        s = np.concatenate([[n, 0.0], a.sum(0), b.sum(0), (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1)])
        T = kabsch(s) @ T
    return T, fitness, rmse, it


def rigid_fit(a, b):
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cb - R @ ca
    return T


class IcpSolverCpu:
    """the default solver's scheme (category_registration.IcpSolver) for templates that are rigid copies of the first"""

    def __init__(self, voxel_size=0.02, max_corr=0.10, max_iteration=100, get_bound=None):
        self.voxel_size, self.max_corr, self.max_iteration, self.get_bound = voxel_size, max_corr, max_iteration, get_bound

    def _frame(self, cloud):
        box = self.get_bound(cloud)
        F = np.eye(4)
        F[:3, :3], F[:3, 3] = box.R, box.center
        return F

    def __call__(self, source, templates):
        import torch
        src = np.asarray(source, np.float64)[0].T
        tm = np.asarray(templates, np.float64).transpose(0, 2, 1)
        src_ds, tgt_ds = CpuCloud(src).voxel_down_sample(self.voxel_size), CpuCloud(tm[0]).voxel_down_sample(self.voxel_size)
        F_s, F_0 = self._frame(src_ds), self._frame(tgt_ds)
        out = []
        for k in range(len(tm)):
            st = max(1, tm.shape[1] // 512)
            S = rigid_fit(tm[0][::st], tm[k][::st]) if k else np.eye(4)
            Q = np.eye(4)
            Q[:3, :3] = S[:3, :3].T
            T, _, _, _ = icp(src_ds.points, tgt_ds.points, F_0 @ Q @ np.linalg.inv(F_s), self.max_corr, self.max_iteration)
            out.append(S @ T)
        out = np.stack(out)
        return torch.from_numpy(out[:, :3, :3].copy()), torch.from_numpy(out[:, :3, 3:].copy())


# ---- align_poses' bookkeeping ------------------------------------------------------------------------------------------
def align_poses_cpu(inst_dict, bbox3d_dict, count_dict, pe_dict, fc_dict, solver, U, multi_init_pose=True, eta1=0.06, eta2=0.15,
                    eta3=0.12, add=100):
    """the bookkeeping of align_poses on CpuCloud entries; U = the product's utils module (host functions only)"""
    moved = (inst_dict, count_dict, bbox3d_dict, pe_dict, fc_dict)
    chamfers = {}
    while bbox3d_dict:
        for cls in list(bbox3d_dict.keys()):
            ids = list(bbox3d_dict[cls].keys())
            counts = [count_dict[cls][i] for i in count_dict[cls].keys()]
            rep_idx = int(np.argmax(counts)) if len(counts) > 1 else 0
            rep = ids[rep_idx]
            tmpl = inst_dict[cls][rep]["pcs"]
            inst_dict[cls][rep]["T_obj"], inst_dict[cls][rep]["bbox3D"] = U.get_pose_from_pointcloud(tmpl, inst_id=rep)
            others = [i for k, i in enumerate(ids) if k != rep_idx]
            if others:
                T_t = inst_dict[cls][rep]["T_obj"].copy()
                s_t = np.linalg.det(T_t[:3, :3]) ** (1 / 3)
                T_t[:3, :3] /= s_t
                syms = U.get_possible_transform_from_bbox() if multi_init_pose else [np.eye(4)]
                tp = tmpl.points
                templates = np.stack([U.transform_pointcloud(tp, S) for S in syms]).transpose(0, 2, 1)
                for i in others:
                    sp = inst_dict[cls][i]["pcs"].points
                    s_s = np.max(sp.max(0) - sp.min(0)) / 2
                    R, t = solver(sp.T[None], templates)
                    cands = []
                    for k, S in enumerate(syms):
                        T = np.eye(4)
                        T[:3, :3], T[:3, 3:] = np.asarray(R[k]), np.asarray(t[k])
                        T = np.linalg.inv(S) @ T
                        cands.append((cKDTree(tp).query(U.transform_pointcloud(sp, T))[0].mean() / s_s, T))
                    k = int(np.argmin([c[0] for c in cands]))
                    ch, T_rel = cands[k]
                    chamfers.setdefault(cls, {})[i] = ch
                    if ch > eta2:
                        sub = True
                    elif ch < eta1:
                        sub = False
                    else:
                        opp = cKDTree(U.transform_pointcloud(sp, T_rel)).query(tp)[0].mean() / s_t
                        sub = bool(opp > eta3)
                    if sub:
                        for d in moved:
                            d.setdefault(cls + add, {})[i] = d[cls].pop(i)
                    else:
                        inst_dict[cls][i]["T_obj"] = np.linalg.inv(T_rel) @ T_t
                        U.get_obb(inst_dict[cls][i])
            bbox3d_dict.pop(cls)
    return chamfers


# ---- synthetic shapes and classes (seeded; the GPU tests and tools/time_registration.py share them) -----------------------------------------------------------------------------------------
def _boxes_surface(rng, boxes, n):
    """n points on the surfaces of axis-aligned boxes [(lo, hi)], area-weighted"""
    faces = []
    for lo, hi in boxes:
        lo, hi = np.asarray(lo, float), np.asarray(hi, float)
        for ax in range(3):
            o = [a for a in range(3) if a != ax]
            area = (hi[o[0]] - lo[o[0]]) * (hi[o[1]] - lo[o[1]])
            faces += [(lo, hi, ax, lo[ax], area), (lo, hi, ax, hi[ax], area)]
    w = np.array([f[4] for f in faces])
    pick = rng.choice(len(faces), n, p=w / w.sum())
    pts = np.empty((n, 3))
    for k, f in enumerate(pick):
        lo, hi, ax, v, _ = faces[f]
        pts[k] = lo + rng.random(3) * (hi - lo)
        pts[k, ax] = v
    return pts


def chair(rng, n):
    """an asymmetric chair: seat, back, one armrest, four legs of two lengths' worth of detail"""
    return _boxes_surface(rng, [((0, 0, 0.40), (0.50, 0.45, 0.46)), ((0, 0, 0.46), (0.05, 0.45, 0.95)),
                                ((0.05, 0, 0.46), (0.40, 0.04, 0.66)), ((0, 0, 0), (0.05, 0.05, 0.40)),
                                ((0.45, 0, 0), (0.50, 0.05, 0.40)), ((0, 0.40, 0), (0.05, 0.45, 0.40)),
                                ((0.45, 0.40, 0), (0.50, 0.45, 0.40))], n)


def pole(rng, n):
    return _boxes_surface(rng, [((0, 0, 0), (0.08, 0.08, 1.9)), ((0, 0, 1.9), (0.6, 0.08, 1.98))], n)


def _pose(rng, k):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = rng.random(3) * 4 - 2 + [3.0 * k, 0, 0]
    return T


def _partial(rng, pts, keep=0.75, noise=0.002):
    """drop the points lowest along a random direction (the side turned away), add noise"""
    d = rng.standard_normal(3)
    s = pts @ (d / np.linalg.norm(d))
    out = pts[s >= np.quantile(s, 1 - keep)]
    return out + noise * rng.standard_normal(out.shape)


def solver_case(seed=31):
    """class 7: four posed, partial (75 %), noisy (2 mm) chairs (the first is complete: the representative) and a pole
    -> (clouds {id: (n,3)}, poses {id: (4,4)}, counts)"""
    rng = np.random.default_rng(seed)
    clouds, poses = {}, {}
    for k, oid in enumerate((11, 12, 13, 14)):
        poses[oid] = _pose(rng, k)
        local = chair(rng, 9000 + 500 * k)
        local = local + 0.002 * rng.standard_normal(local.shape) if k == 0 else _partial(rng, local)
        clouds[oid] = local @ poses[oid][:3, :3].T + poses[oid][:3, 3]
    poses[15] = _pose(rng, 5)
    clouds[15] = pole(rng, 7000) @ poses[15][:3, :3].T + poses[15][:3, 3]
    return clouds, poses, {11: 900, 12: 500, 13: 400, 14: 300, 15: 200}


def pose_errors(inst_dict, poses, cls=7, rep=11):
    """per aligned copy: (rotation error in degrees, translation error in metres) of T_obj against the known pose.
    T_obj = inv(T_rel) T_obj_rep with T_rel: copy -> representative, so the expected T_obj is P_i inv(P_rep) T_obj_rep."""
    T_rep = inst_dict[cls][rep]["T_obj"].copy()
    T_rep[:3, :3] /= np.linalg.det(T_rep[:3, :3]) ** (1 / 3)
    out = {}
    for oid, info in inst_dict[cls].items():
        if oid == rep:
            continue
        want = poses[oid] @ np.linalg.inv(poses[rep]) @ T_rep
        got = info["T_obj"].copy()
        got[:3, :3] /= np.linalg.det(got[:3, :3]) ** (1 / 3)
        c = (np.trace(got[:3, :3].T @ want[:3, :3]) - 1) / 2
        out[oid] = (float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(got[:3, 3] - want[:3, 3])))
    return out


def build_dicts(clouds, counts, cloud_type, cls=7):
    inst = {cls: {oid: {"pcs": cloud_type(p), "frame_info": []} for oid, p in clouds.items()}}
    cnt = {cls: dict(counts)}
    bbox = {cls: {oid: "bbox-%d" % oid for oid in clouds}}
    pe = {cls: {oid: "pe-%d" % oid for oid in clouds}}
    fc = {cls: {oid: "fc-%d" % oid for oid in clouds}}
    return inst, bbox, cnt, pe, fc
