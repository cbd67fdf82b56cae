"""TEST INFRASTRUCTURE: numpy fp64 restatement of csrc/fpfh.hip ("FPFH mode") and of FpfhTeaserSolver: the
hybrid neighbour search, the normals (cyclic Jacobi, the orientation rule), SPFH / FPFH operation by operation, the sequential
fp32 nearest neighbour in descriptor space, mutual correspondences, and the solver on teaser_cpu / registration_cpu for the
stages it inherits.  Also the seeded cases the host and GPU tests share."""
import math

import numpy as np

import registration_cpu as RC
import teaser_cpu as TC

NB, NF = 11, 33
JACOBI_SWEEPS = 8


# ---- hybrid search -----------------------------------------------------------------------------------------------------
def hybrid_search(points, radius, max_nn):
    """points: fp32 values.  -> (idx (n,max_nn) i32 padded -1, d2 (n,max_nn) f64 padded 0, count (n,) i32): per point the points
    with d2 = (dx dx + dy dy) + dz dz < radius radius (fp64 from the f32 coordinates), by (d2, index) ascending, the first max_nn.
    Brute force over all pairs: the cells of the kernel only pre-select."""
    p = np.asarray(points, np.float32).astype(np.float64)
    n = len(p)
    idx = np.full((n, max_nn), -1, np.int32)
    d2o = np.zeros((n, max_nn))
    count = np.zeros(n, np.int32)
    r2 = float(radius) * float(radius)
    for i in range(n):
        d = p[i] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = np.flatnonzero(d2 < r2)
        order = inside[np.lexsort((inside, d2[inside]))][:max_nn]
        count[i] = len(order)
        idx[i, :len(order)] = order
        d2o[i, :len(order)] = d2[order]
    return idx, d2o, count


def centroid(points):
    """the fp64 mean of the fp32 values, summed one after the other"""
    p = np.asarray(points, np.float32).astype(np.float64)
    return np.cumsum(p, axis=0)[-1] / float(len(p))


# ---- normals -----------------------------------------------------------------------------------------------------------
def _rotate(A, V, p, q, r):
    """one Jacobi rotation on (p, q) of the stacked symmetric matrices A (n,3,3) (only a_pp, a_qq, a_pq = A[:,p,q], a_rp =
    A[:,min,max] are kept up to date, as the kernel keeps six numbers) and of V (n,3,3), where a_pq != 0"""
    key = lambda a, b: (min(a, b), max(a, b))
    app, aqq, apq = A[:, p, p].copy(), A[:, q, q].copy(), A[:, p, q].copy()
    arp, arq = A[(slice(None),) + key(r, p)].copy(), A[(slice(None),) + key(r, q)].copy()
    on = apq != 0.0
    safe = np.where(on, apq, 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        theta = (aqq - app) / (2.0 * safe)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    tp = t * apq
    A[:, p, p] = np.where(on, app - tp, app)
    A[:, q, q] = np.where(on, aqq + tp, aqq)
    A[:, p, q] = np.where(on, 0.0, apq)
    A[(slice(None),) + key(r, p)] = np.where(on, c * arp - s * arq, arp)
    A[(slice(None),) + key(r, q)] = np.where(on, s * arp + c * arq, arq)
    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
    V[:, :, p] = np.where(on[:, None], c[:, None] * vp - s[:, None] * vq, vp)
    V[:, :, q] = np.where(on[:, None], s[:, None] * vp + c[:, None] * vq, vq)


def jacobi_eigen(A0, sweeps=JACOBI_SWEEPS):
    """stacked symmetric (n,3,3) -> (diagonal (n,3) after the sweeps, V (n,3,3) with the eigenvectors in its columns)"""
    A = np.array(A0, np.float64)
    V = np.tile(np.eye(3), (len(A), 1, 1))
    for _ in range(sweeps):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), V


def covariances(points, idx, count):
    """-> (cov (n,3,3) of each list, sequential in list order; rows with fewer than 3 neighbours hold the identity)"""
    p = np.asarray(points, np.float32).astype(np.float64)
    n, K = idx.shape
    cov = np.tile(np.eye(3), (n, 1, 1))
    for i in range(n):
        k = int(count[i])
        if k < 3:
            continue
        q = p[idx[i, :k]]
        mean = np.cumsum(q, axis=0)[-1] / float(k)
        d = q - mean
        for a in range(3):
            for b in range(a, 3):
                cov[i, a, b] = cov[i, b, a] = np.cumsum(d[:, a] * d[:, b])[-1] / float(k)
    return cov


def estimate_normals(points, idx, count, c=None, return_eigen=False, return_raw=False):
    """-> normals (n,3) f64 [, eigenvalues ascending (n,3) of the restatement's Jacobi] [, the unit eigenvectors before the
    orientation rule]"""
    p = np.asarray(points, np.float32).astype(np.float64)
    c = centroid(points) if c is None else np.asarray(c, np.float64)
    lam, V = jacobi_eigen(covariances(points, idx, count))
    pick = np.zeros(len(p), np.int64)
    low = lam[:, 0].copy()
    for a in (1, 2):
        better = lam[:, a] < low
        pick[better], low[better] = a, lam[better, a]
    e = V[np.arange(len(p)), :, pick]
    length = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    nrm = e / length[:, None]
    raw = nrm.copy()
    d = p - c
    dot = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]
    big = nrm[:, 0].copy()
    for a in (1, 2):
        more = np.abs(nrm[:, a]) > np.abs(big)
        big[more] = nrm[more, a]
    flip = (dot < 0.0) | ((dot == 0.0) & (big < 0.0))
    nrm[flip] = -nrm[flip]
    nrm[np.asarray(count) < 3] = (0.0, 0.0, 1.0)
    out = (nrm,) + ((np.sort(lam, axis=1),) if return_eigen else ()) + ((raw,) if return_raw else ())
    return out if len(out) > 1 else nrm


def largest_component(v):
    """per row the component of largest magnitude, the first of equals"""
    big = v[:, 0].copy()
    for a in (1, 2):
        more = np.abs(v[:, a]) > np.abs(big)
        big[more] = v[more, a]
    return big


def tie_rule_rows(raw, count, each=4):
    """rows for the dot == 0 rule: the first `each` full rows whose raw eigenvector has a negative largest component (the rule
    must flip them) and the first `each` with a positive one (it must not).  With the centroid set to point i itself, p_i - c
    is exactly 0 and so is the dot product, whatever the normal."""
    big = largest_component(raw)
    full = np.asarray(count) >= 3
    return np.flatnonzero(full & (big < 0))[:each].tolist(), np.flatnonzero(full & (big > 0))[:each].tolist()


# ---- SPFH and FPFH -----------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pair_features(p1, n1, p2, n2):
    """stacked pairs -> (the three scaled features x (m,3) whose floor, clamped to [0, 10], is the bin; swap margin | |a1| - |a2| |
    (m,), inf where the pair has d == 0)"""
    p1, n1, p2, n2 = (np.asarray(a, np.float64) for a in (p1, n1, p2, n2))
    dp = p2 - p1
    d = np.sqrt(_dot(dp, dp))
    live = d != 0.0
    ds = np.where(live, d, 1.0)
    a1, a2 = _dot(n1, dp) / ds, _dot(n2, dp) / ds
    swap = np.abs(a1) < np.abs(a2)
    s1 = np.where(swap[:, None], n2, n1)
    s2 = np.where(swap[:, None], n1, n2)
    dp = np.where(swap[:, None], -dp, dp)
    f2 = np.where(swap, -a2, a1)
    v = _cross(dp, s1)
    vn = np.sqrt(_dot(v, v))
    live &= vn != 0.0
    v = v / np.where(vn != 0.0, vn, 1.0)[:, None]
    w = _cross(s1, v)
    f1 = _dot(v, s2)
    f0 = np.arctan2(_dot(w, s2), _dot(s1, s2))
    f = np.where(live[:, None], np.stack([f0, f1, f2], 1), 0.0)
    x = np.stack([(11.0 * (f[:, 0] + np.pi)) / (2.0 * np.pi), (11.0 * (f[:, 1] + 1.0)) * 0.5, (11.0 * (f[:, 2] + 1.0)) * 0.5], 1)
    return x, np.where(d != 0.0, np.abs(np.abs(a1) - np.abs(a2)), np.inf)


def bins_of(x):
    return np.clip(np.floor(x), 0.0, 10.0).astype(np.int64)


def spfh(points, normals, idx, count, return_margins=False, exact_rows=()):
    """-> spfh (n,33) f64 [, the smallest distance of a scaled feature to a bin edge (an integer in 1..10: beyond those floor and
    clamp cannot change the bin) over all pairs, the smallest swap margin; the rows in exact_rows, whose arithmetic is exact by
    construction, are left out of both]"""
    p = np.asarray(points, np.float32).astype(np.float64)
    nrm = np.asarray(normals, np.float64)
    n, K = idx.shape
    out = np.zeros((n, NF))
    edge, swap = np.inf, np.inf
    for i in range(n):
        k = int(count[i])
        if k <= 1:
            continue
        nb = idx[i, 1:k]
        x, margin = pair_features(np.repeat(p[i:i + 1], k - 1, 0), np.repeat(nrm[i:i + 1], k - 1, 0), p[nb], nrm[nb])
        b = bins_of(x)
        hist = np.zeros(NF, np.int64)
        for a in range(3):
            np.add.at(hist, a * NB + b[:, a], 1)
        out[i] = hist.astype(np.float64) * (100.0 / float(k - 1))
        if i not in exact_rows:
            edge = min(edge, float(np.abs(x[:, :, None] - np.arange(1.0, 11.0)[None, None, :]).min()))
            swap = min(swap, float(margin.min()))
    return (out, edge, swap) if return_margins else out


def fpfh(spfh_rows, idx, d2, count):
    spf = np.asarray(spfh_rows, np.float64)
    n, K = idx.shape
    out = np.zeros((n, NF))
    for i in range(n):
        k = int(count[i])
        if k <= 1:
            continue
        acc, total = np.zeros(NF), np.zeros(3)
        for s in range(1, k):
            if d2[i, s] == 0.0:
                continue
            val = spf[idx[i, s]] / d2[i, s]
            acc += val
            for g in range(3):                       # sum[g] takes its 11 values one after the other, after the earlier neighbours'
                for j in range(g * NB, (g + 1) * NB):
                    total[g] += val[j]
        for g in range(3):
            if total[g] != 0.0:
                acc[g * NB:(g + 1) * NB] = acc[g * NB:(g + 1) * NB] * (100.0 / total[g])
        out[i] = acc + spf[i]
    return out


def extract_fpfh(points, voxel_size, return_parts=False):
    """helpers.extract_fpfh on fp32 values: normals at 2 voxel / 30, FPFH at 5 voxel / 100 -> (n,33) f64"""
    idx_n, _, cnt_n = hybrid_search(points, 2.0 * voxel_size, 30)
    nrm = estimate_normals(points, idx_n, cnt_n)
    idx, d2, cnt = hybrid_search(points, 5.0 * voxel_size, 100)
    s = spfh(points, nrm, idx, cnt)
    f = fpfh(s, idx, d2, cnt)
    return (f, nrm, s, (idx, d2, cnt)) if return_parts else f


# ---- descriptor nearest neighbour ----------------------------------------------------------------------------------------
def feature_nn(q, p):
    """-> (index (nq,) i32: the lowest row of p with the least sequential fp32 sum of squared differences, that sum (nq,) f32)"""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    index = np.zeros(len(q), np.int32)
    dist = np.zeros(len(q), np.float32)
    for i in range(len(q)):
        s = np.zeros(len(p), np.float32)
        for j in range(q.shape[1]):
            d = q[i, j] - p[:, j]
            s = s + d * d
        index[i] = int(np.argmin(s))                  # the first of equals
        dist[i] = s[index[i]]
    return index, dist


def mutual_correspondences(f0, f1, mutual_filter=True):
    """helpers.find_correspondences on the f32-rounded descriptors -> (idx0, idx1) int64, idx0 ascending"""
    nn01, _ = feature_nn(f0, f1)
    i0 = np.arange(len(nn01), dtype=np.int64)
    if not mutual_filter:
        return i0, nn01.astype(np.int64)
    nn10, _ = feature_nn(f1, f0)
    keep = nn10[nn01] == i0
    return i0[keep], nn01[keep].astype(np.int64)


# ---- the solver --------------------------------------------------------------------------------------------------------
class FpfhTeaserSolverCpu:
    """FpfhTeaserSolver on CpuCloud's down-sampling, the restated descriptors, teaser_cpu's graph / clique / rotation /
    translation and registration_cpu.icp"""

    def __init__(self, voxel_size=0.05, noise_bound=None, max_correspondences=10000, cbar2=1.0, seed=0, icp_max_iteration=100):
        self.voxel_size, self.noise_bound = voxel_size, (voxel_size if noise_bound is None else noise_bound)
        self.max_correspondences, self.cbar2, self.seed, self.icp_max_iteration = max_correspondences, cbar2, seed, icp_max_iteration

    def solve_one(self, src, tmpl):
        s = RC.CpuCloud(src).voxel_down_sample(self.voxel_size)
        t = RC.CpuCloud(tmpl).voxel_down_sample(self.voxel_size)
        i0, i1 = mutual_correspondences(extract_fpfh(s.p32, self.voxel_size), extract_fpfh(t.p32, self.voxel_size))
        if len(i0) > self.max_correspondences:
            keep = np.sort(np.random.default_rng(self.seed).choice(len(i0), self.max_correspondences, replace=False))
            i0, i1 = i0[keep], i1[keep]
        if len(i0) == 0:
            raise ValueError("no mutual correspondences")
        pairs = np.stack([i0, i1], 1)
        A, B = s.points[i0], t.points[i1]
        clique = TC.max_clique(TC.graph(A, B, self.noise_bound, self.cbar2))
        T0, _ = TC.solve_pose(A[clique], B[clique], self.noise_bound, self.cbar2)
        T, _, _, _ = RC.icp(s.points, t.points, T0, self.noise_bound, self.icp_max_iteration)
        self.last = dict(pairs=pairs, clique=clique, T0=T0, n_src=len(s.p32), n_tgt=len(t.p32), source=s.points, target=t.points)
        return T

    def __call__(self, source, templates):
        import torch
        src = np.asarray(source, np.float64)[0].T
        tm = np.asarray(templates, np.float64).transpose(0, 2, 1)
        T = self.solve_one(src, tm[0])
        st = max(1, tm.shape[1] // 512)
        out = np.stack([(RC.rigid_fit(tm[0][::st], tm[k][::st]) if k else np.eye(4)) @ T for k in range(len(tm))])
        return torch.from_numpy(out[:, :3, :3].copy()), torch.from_numpy(out[:, :3, 3:].copy())


# ---- seeded cases ------------------------------------------------------------------------------------------------------
def jittered_cloud(seed, n, box=1.0):
    """n points uniform in a cube, fp32: free of exact ties"""
    return (np.random.default_rng(seed).random((n, 3)) * box - box / 2).astype(np.float32)


def lattice_cloud(m=5):
    """the integer lattice {-m//2 .. }^3 scaled by 2^-4, both sides of 0 on every axis: every distance is exact, many d2 are equal
    (order falls to the index) and with radius 2^-4 k the lattice points at distance exactly radius test the strict <"""
    g = np.arange(m) - m // 2
    return (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) / 16.0).astype(np.float32)


def search_cases(capacity):
    """name -> (points f32, radius, max_nn) for the hybrid search.  `capacity`: the kernel's per-wave buffer."""
    rng = np.random.default_rng(77)
    out = {}
    for n in (1, 63, 65, 257):
        out["n%d" % n] = (jittered_cloud(100 + n, n), 0.3, 30)
    lat = lattice_cloud(5)                                     # 125 points, spacing 1/16
    out["lattice"] = (lat, 2.0 / 16.0, 30)                      # 33 lattice points lie within or at 2/16: 6 of them exactly at it
    out["lattice_nn128"] = (lat, 3.0 / 16.0, 128)
    mixed = np.concatenate([jittered_cloud(5, 200, 0.4), jittered_cloud(6, 40, 2.0) + np.float32(3.0),
                            np.array([[9.0, -9.0, 9.0]], np.float32)])       # a dense part, a sparse part, an isolated point
    mixed = np.concatenate([mixed, mixed[[3, 3, 17, 240]]])    # duplicated points (the isolated one too)
    for max_nn in (1, 30, 100, 128):
        out["mixed_nn%d" % max_nn] = (mixed, 0.15, max_nn)
    clump = np.concatenate([(rng.random((capacity + 150, 3)) * 0.05).astype(np.float32), jittered_cloud(8, 60, 1.0)])
    out["clump"] = (clump[rng.permutation(len(clump))], 0.2, 100)
    return out


def surface(seed, nx=25, ny=24, spacing=0.0355, n_bumps=40):
    """A plate of gentle random bumps (Gaussians 5 to 9 cm wide, 1.5 to 3.5 cm high or deep) on a jittered hexagonal grid, the
    points about 3.6 cm apart: farther than the diagonal of a 2 cm voxel, so every point stays alone in its voxel under any
    pose, and nearer than the 4 cm of the normals' search, so every point has its ring of six.  Flat boxes give FPFH nothing
    to tell the points of a face apart by, and the spaced random points of teaser_cpu.registration_case have no surface,
    hence no normals that survive 2 mm of noise: this sibling is the class of the end-to-end tests.  -> (n,3) f64"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    x = (i + 0.5 * (j % 2)) * spacing + (rng.random(i.shape) - 0.5) * 0.02 * spacing
    y = j * spacing * math.sqrt(3.0) / 2.0 + (rng.random(i.shape) - 0.5) * 0.02 * spacing
    z = np.zeros_like(x)
    for _ in range(n_bumps):
        cx, cy = rng.random() * nx * spacing, rng.random() * ny * spacing * 0.87
        w, h = 0.05 + 0.04 * rng.random(), (0.015 + 0.02 * rng.random()) * rng.choice([-1.0, 1.0])
        z = z + h * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * w * w))
    return np.stack([x, y, z], -1).reshape(-1, 3)


def other_surface(seed, n=18, spacing=0.04):
    """another shape for align_poses to split off: a long half cylinder"""
    rng = np.random.default_rng(seed)
    a, h = np.meshgrid(np.linspace(0.0, np.pi, 8), np.arange(4 * n) * spacing, indexing="ij")
    a = a + (rng.random(a.shape) - 0.5) * 0.05
    return np.stack([0.1 * np.cos(a), 0.1 * np.sin(a), h], -1).reshape(-1, 3)


E2E_VOXEL = 0.02          # 2 cm voxels: points 3 cm apart stay alone in theirs; normals within 4 cm, descriptors within 10 cm


def e2e_case(seed=51, n_outliers=12, noise=0.002):
    """class 7: the surface (11, the representative), two posed copies (12, 13) with 2 mm noise and unrelated points, and
    another shape (15).  -> (clouds {id: (n,3)}, poses {id: (4,4)}, counts)"""
    rng = np.random.default_rng(seed)
    local = surface(seed)
    clouds, poses = {}, {}
    for k, oid in enumerate((11, 12, 13)):
        poses[oid] = RC._pose(rng, k)
        pts = local
        if k:
            far = TC.spaced_points(rng, n_outliers, local.min(0) - 0.2, local.max(0) + 0.2, 0.06)
            pts = np.concatenate([local + noise * rng.standard_normal(local.shape), far])[rng.permutation(len(local) + n_outliers)]
        clouds[oid] = pts @ poses[oid][:3, :3].T + poses[oid][:3, 3]
    poses[15] = RC._pose(rng, 5)
    clouds[15] = other_surface(seed + 1) @ poses[15][:3, :3].T + poses[15][:3, 3]
    return clouds, poses, {11: 900, 12: 500, 13: 400, 15: 200}


def normals_cases():
    """name -> (points f32, radius, max_nn).  `aniso`: a lattice with spacings 1/16, 1/8, 1/4, symmetric about the origin: the
    centroid is exactly 0, the points with x = 0 have n.(p - c) exactly 0 wherever the normal is the x axis, and every sum is
    exact.  `sparse` has rows with fewer than 3 neighbours."""
    g = np.arange(5) - 2
    aniso = (np.stack(np.meshgrid(g / 16.0, g / 8.0, g / 4.0, indexing="ij"), -1).reshape(-1, 3)).astype(np.float32)
    return {"jitter_300": (jittered_cloud(21, 300, 1.0), 0.25, 30), "surface": (surface(51).astype(np.float32), 0.04, 30),
            "aniso": (aniso, 0.3, 30), "sparse": (jittered_cloud(22, 40, 2.0), 0.35, 30)}


def eigen_gap(lam):
    """(l1 - l0) / l2 of ascending eigenvalues (0 where l2 is 0)"""
    return np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0, lam[:, 2], 1.0), 0.0)


def angles(a, b):
    """angle in radians between unit vectors, up to sign, from the cross product (accurate near 0)"""
    return np.arcsin(np.clip(np.linalg.norm(np.cross(a, b), axis=1), 0.0, 1.0))


def descriptor_case(seed=32, n=260):
    """A jittered cloud plus the special rows of the SPFH / FPFH tests -> (points f32, radius, max_nn, special: name -> index).
    isolated: no neighbour but itself (k = 1); dup: a copy of point 0 (a pair with d == 0); along_a / along_b: two points alone
    together, one straight above the other: both keep the rule's normal (0, 0, 1), so dp is parallel to it and |v| == 0."""
    cand = jittered_cloud(seed, 4 * n, 0.6)                  # thinned to 4 cm apart: two points 1 cm apart share their whole
    keep = []                                               # neighbourhood, hence their normal to the last bit, and |a1| = |a2|
    for i in range(len(cand)):
        if all(np.linalg.norm(cand[i].astype(np.float64) - cand[j]) >= 0.04 for j in keep):
            keep.append(i)
    p = cand[keep[:n]]
    n = len(p)
    extra = np.array([[9.0, 9.0, 9.0], p[0], [5.0, 5.0, 5.0], [5.0, 5.0, 5.0625]], np.float32)
    return np.concatenate([p, extra]), 0.2, 40, dict(isolated=n, dup=n + 1, along_a=n + 2, along_b=n + 3)


def chair_correspondence_figures(copies=(12, 13, 14), voxel=0.05):
    """DESIGN.md 3.9's figures on registration_cpu.solver_case (the chairs of the all-pairs finding) at the FPFH defaults, voxel
    0.05 m and noise bound = voxel: per copy (mutual correspondences, those true within 2 noise_bound, those within 2 cm).
    `python tests/fpfh_cpu.py` prints them (about half a minute)."""
    clouds, poses, _ = RC.solver_case()
    t = RC.CpuCloud(clouds[11]).voxel_down_sample(voxel)
    ft = extract_fpfh(t.p32, voxel)
    out = {}
    for oid in copies:
        s = RC.CpuCloud(clouds[oid]).voxel_down_sample(voxel)
        i0, i1 = mutual_correspondences(extract_fpfh(s.p32, voxel), ft)
        want = poses[11] @ np.linalg.inv(poses[oid])
        err = np.linalg.norm(s.points[i0] @ want[:3, :3].T + want[:3, 3] - t.points[i1], axis=1)
        out[oid] = (len(i0), int((err < 2 * voxel).sum()), int((err < 0.02).sum()))
    return out


if __name__ == "__main__":
    print("chair case, FPFH mode: copy -> (correspondences, true within 2 noise_bound, true within 2 cm)", chair_correspondence_figures())
