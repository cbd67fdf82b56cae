"""TEST INFRASTRUCTURE: numpy restatement of the TEASER-style solver (category_registration.TeaserSolver).
fp64 throughout, except the graph's comparison, which repeats the kernel's fp32 expression operation by operation.  Dense
boolean graph, exact maximum clique by Bron-Kerbosch with pivoting (small N), GNC-TLS rotation, adaptive voting, and the
whole solver on the restated clouds and ICP of registration_cpu.  Also the seeded planted cases the tests share."""
import math

import numpy as np

import registration_cpu as RC


# ---- graph -------------------------------------------------------------------------------------------------------------
def threshold32(noise_bound=0.01, cbar2=1.0):
    return np.float32(2.0 * noise_bound * math.sqrt(cbar2))


def pair_norms32(P):
    """(N,N) fp32: sqrt((dx dx + dy dy) + dz dz) of P_i - P_j, every operation rounded to fp32"""
    P = np.asarray(P, np.float32)
    d = P[:, None, :] - P[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def graph(A, B, noise_bound=0.01, cbar2=1.0):
    """dense boolean adjacency of the compatibility graph"""
    diff = np.abs(pair_norms32(B) - pair_norms32(A))
    adj = diff <= threshold32(noise_bound, cbar2)
    np.fill_diagonal(adj, False)
    return adj


def threshold_margin(A, B, noise_bound=0.01, cbar2=1.0):
    """how far the nearest pair stays from the threshold, in ulps of fp32 at the distance scale (the larger of the two norms
    and the threshold): the graph may be compared bit for bit when this is large"""
    na, nb = pair_norms32(A).astype(np.float64), pair_norms32(B).astype(np.float64)
    thr = float(threshold32(noise_bound, cbar2))
    gap = np.abs(np.abs(nb - na) - thr)
    scale = np.maximum(np.maximum(na, nb), thr)
    ulp = np.spacing(scale.astype(np.float32)).astype(np.float64)
    np.fill_diagonal(gap, np.inf)
    return float((gap / ulp).min())


def pack(adj):
    """dense boolean -> (N, ceil(N/64)) uint64 bitset rows, bit j & 63 of word j >> 6"""
    N = len(adj)
    W = (N + 63) // 64
    padded = np.zeros((N, W * 64), np.uint8)
    padded[:, :N] = adj
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(N, W)


def unpack(words, N):
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint8).reshape(len(words), -1)
    return np.unpackbits(w, axis=1, bitorder="little")[:, :N].astype(bool)


# ---- maximum clique ----------------------------------------------------------------------------------------------------
def search_order(adj):
    """ascending degree, ties by index"""
    return np.argsort(adj.sum(1), kind="stable")


def max_clique(adj):
    """the maximum clique that is lexicographically smallest in positions of search_order(adj) -> vertices in that order.
    Bron-Kerbosch with a pivot of most candidates; branches that cannot reach the best size so far are cut (equal sizes are
    kept for the lexicographic choice); a greedy pass gives the first bound."""
    adj = np.asarray(adj, bool)
    N = len(adj)
    order = search_order(adj)
    sub = adj[np.ix_(order, order)]
    nb = [int.from_bytes(np.packbits(row, bitorder="little").tobytes(), "little") for row in sub]

    def bits(x):
        out = []
        while x:
            low = x & -x
            out.append(low.bit_length() - 1)
            x ^= low
        return out

    state = {"size": 1, "best": None}
    for v in range(N):                                   # greedy: the lowest later neighbour each time
        P, n = nb[v] >> (v + 1) << (v + 1), 1
        while P:
            u = (P & -P).bit_length() - 1
            P &= nb[u]
            n += 1
        state["size"] = max(state["size"], n)

    def bk(R, P, X):
        if not P and not X:
            key = sorted(R)
            if len(R) > state["size"] or (len(R) == state["size"] and (state["best"] is None or key < state["best"])):
                state["size"], state["best"] = len(R), key
            return
        if len(R) + bin(P).count("1") < state["size"]:
            return
        pivot = max(bits(P | X), key=lambda u: bin(P & nb[u]).count("1"))
        for v in bits(P & ~nb[pivot]):
            bk(R + [v], P & nb[v], X & nb[v])
            P &= ~(1 << v)
            X |= 1 << v

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), N + 100))
    bk([], (1 << N) - 1, 0)
    return order[np.array(state["best"], np.int64)]


def is_clique(adj, members):
    m = np.asarray(members)
    s = np.asarray(adj)[np.ix_(m, m)]
    return len(set(m.tolist())) == len(m) and bool((s | np.eye(len(m), dtype=bool)).all())


# ---- rotation and translation ------------------------------------------------------------------------------------------
def fit_rotation(a, b, w):
    H = np.einsum("k,ki,kj->ij", w, a, b)
    U, _, Vt = np.linalg.svd(H)
    D = np.eye(3)
    D[2, 2] = np.linalg.det(Vt.T @ U.T)
    return Vt.T @ D @ U.T


def gnc_tls(a, b, bound, factor=1.4, max_iterations=100, cost_threshold=1e-12):
    """-> (R, iterations)"""
    w, mu, last = np.ones(len(a)), None, np.inf
    R = np.eye(3)
    for it in range(1, max_iterations + 1):
        R = fit_rotation(a, b, w)
        r2 = np.square(b - a @ R.T).sum(1)
        if mu is None:
            mu = 1.0 / (2.0 * r2.max() / bound - 1.0)
            if mu <= 0:
                return R, it
        cost = float(w @ r2)
        for k, r in enumerate(r2):
            if r >= (mu + 1) / mu * bound:
                w[k] = 0.0
            elif r <= mu / (mu + 1) * bound:
                w[k] = 1.0
            else:
                w[k] = math.sqrt(bound * mu * (mu + 1) / r) - mu
        mu *= factor
        if abs(cost - last) < cost_threshold:
            return R, it
        last = cost
    return R, max_iterations


def vote(x, bound, cbar2=1.0):
    """the scalar TLS estimate by a sweep over the sorted interval ends"""
    x = np.asarray(x, np.float64)
    half = bound * math.sqrt(cbar2)
    events = sorted([(v - half, 0, k) for k, v in enumerate(x)] + [(v + half, 1, k) for k, v in enumerate(x)])
    inside, best = set(), (np.inf, 0.0)
    for _, leaving, k in events:
        inside.remove(k) if leaving else inside.add(k)
        if inside:
            sel = x[sorted(inside)]
            t = sel.mean()
            cost = np.square(sel - t).sum() / bound ** 2 + cbar2 * (len(x) - len(sel))
            if cost < best[0]:
                best = (cost, float(t))
    return best[1]


def chain(a, b):
    """translation-invariant measurements of consecutive members, the last with the first"""
    K = len(a)
    nxt = (np.arange(K) + 1) % K
    k = K if K > 2 else K - 1
    return (a[nxt] - a)[:k], (b[nxt] - b)[:k]


def solve_pose(a, b, noise_bound=0.01, cbar2=1.0, factor=1.4, max_iterations=100, cost_threshold=1e-12):
    ta, tb = chain(a, b)
    R, its = gnc_tls(ta, tb, (2 * noise_bound) ** 2 * cbar2, factor, max_iterations, cost_threshold) if len(ta) else (np.eye(3), 0)
    d = b - a @ R.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, [vote(d[:, k], noise_bound, cbar2) for k in range(3)]
    return T, its


def pairs_for(n_s, n_t, max_correspondences, seed):
    total = n_s * n_t
    flat = np.sort(np.random.default_rng(seed).choice(total, max_correspondences, replace=False)) if total > max_correspondences \
        else np.arange(total)
    return np.stack([flat // n_t, flat % n_t], 1)


class TeaserSolverCpu:
    """the whole solver on CpuCloud's down-sampling and registration_cpu.icp; templates are solved against the first and moved
    by the rigid fits between the copies, as TeaserSolver does for rigid copies"""

    def __init__(self, voxel_size=0.1, noise_bound=0.01, max_correspondences=10000, cbar2=1.0, seed=0, icp_max_iteration=100):
        self.voxel_size, self.noise_bound, self.max_correspondences, self.cbar2 = voxel_size, noise_bound, max_correspondences, cbar2
        self.seed, self.icp_max_iteration = seed, icp_max_iteration

    def solve_one(self, src, tmpl):
        s = RC.CpuCloud(src).voxel_down_sample(self.voxel_size).points
        t = RC.CpuCloud(tmpl).voxel_down_sample(self.voxel_size).points
        pairs = pairs_for(len(s), len(t), self.max_correspondences, self.seed)
        A, B = s[pairs[:, 0]], t[pairs[:, 1]]
        clique = max_clique(graph(A, B, self.noise_bound, self.cbar2))
        T0, _ = solve_pose(A[clique], B[clique], self.noise_bound, self.cbar2)
        T, _, _, _ = RC.icp(s, t, T0, self.noise_bound, self.icp_max_iteration)
        self.last = dict(pairs=pairs, clique=clique, T0=T0)
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
def spaced_points(rng, n, lo, hi, gap):
    """n points uniform in the box [lo, hi], each at least `gap` from the others"""
    pts = []
    while len(pts) < n:
        p = lo + rng.random(3) * (np.asarray(hi) - lo)
        if all(np.linalg.norm(p - q) >= gap for q in pts):
            pts.append(p)
    return np.array(pts)


def planted_case(seed, n_template=60, n_keep=60, n_outliers=20, max_correspondences=2500, noise=0.002, gap=0.06):
    """A template of n_template spaced points in a 1 m x 0.8 m x 0.6 m box; the source is n_keep of them under a random pose with
    `noise` Gaussian noise per axis, plus n_outliers unrelated spaced points; all-to-all pairs sub-sampled to max_correspondences.
    -> dict(A, B (N,3) f32, inliers (N,) bool: the true correspondences, pose (4,4) template -> source, source, template)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.zeros(3), np.array([1.0, 0.8, 0.6])
    tmpl = spaced_points(rng, n_template, lo, hi, gap)
    kept = rng.permutation(n_template)[:n_keep]
    P = RC._pose(rng, 0)
    src_in = tmpl[kept] @ P[:3, :3].T + P[:3, 3] + noise * rng.standard_normal((n_keep, 3))
    out_local = spaced_points(rng, n_outliers, lo, hi, gap).reshape(-1, 3)
    src = np.concatenate([src_in, out_local @ P[:3, :3].T + P[:3, 3]])
    order = rng.permutation(len(src))
    src, true_of = src[order], np.r_[kept, -np.ones(n_outliers, np.int64)][order]
    pairs = pairs_for(len(src), n_template, max_correspondences, seed)
    A, B = src[pairs[:, 0]].astype(np.float32), tmpl[pairs[:, 1]].astype(np.float32)
    return dict(A=A, B=B, inliers=true_of[pairs[:, 0]] == pairs[:, 1], pose=P, source=src, template=tmpl, pairs=pairs)


def random_graph(seed, N, density):
    rng = np.random.default_rng(seed)
    up = np.triu(rng.random((N, N)) < density, 1)
    return up | up.T


def guarded(A, B, ulps=32.0, noise_bound=0.01, cbar2=1.0):
    """the correspondences left after dropping one end of every pair that lies within `ulps` of the threshold"""
    na, nb = pair_norms32(A).astype(np.float64), pair_norms32(B).astype(np.float64)
    thr = float(threshold32(noise_bound, cbar2))
    near = np.abs(np.abs(nb - na) - thr) < ulps * np.spacing(np.maximum(np.maximum(na, nb), thr).astype(np.float32))
    np.fill_diagonal(near, False)
    keep = np.ones(len(A), bool)
    for i, j in zip(*np.nonzero(np.triu(near))):
        if keep[i] and keep[j]:
            keep[j] = False
    return A[keep], B[keep], keep


def graph_cases():
    """the graph cases the GPU test compares bit for bit (tests/test_teaser_host.py guards each): name -> (A, B).  Planted cases
    with the few vertices of near-threshold pairs dropped; sizes 1, 65, about 1000 and about 2500."""
    out = {}
    for name, kw in (("planted_2500", dict(seed=3)), ("planted_1000", dict(seed=4, max_correspondences=1000)),
                     ("n65", dict(seed=5, n_template=13, n_keep=4, n_outliers=1, max_correspondences=10 ** 9))):
        c = planted_case(**kw)
        out[name] = guarded(c["A"], c["B"])[:2]
    c = planted_case(seed=6, n_template=5, n_keep=1, n_outliers=0, max_correspondences=1)
    out["n1"] = (c["A"], c["B"])
    return out


# ---- a class for align_poses: partial, noisy copies of a sparse template with unrelated points, and another shape ---------
REG_VOXEL, REG_MAX_CORR = 0.02, 2500          # the solver arguments of the case: 2 cm voxels keep points 6 cm apart separate


def registration_case(seed=41, n_template=100, keep=0.5, n_outliers=5, noise=0.002):
    """class 7: the template (11, complete, the representative), three copies (12, 13, 14) that keep the half of its points
    highest along a random direction, with 2 mm noise and n_outliers unrelated points, and another shape (15); all posed.
    -> (clouds {id: (n,3)}, poses {id: (4,4)}, counts) as registration_cpu.solver_case gives them"""
    rng = np.random.default_rng(seed)
    lo, hi = np.zeros(3), np.array([1.0, 0.8, 0.6])
    local = spaced_points(rng, n_template, lo, hi, 0.06)
    clouds, poses = {}, {}
    for k, oid in enumerate((11, 12, 13, 14)):
        poses[oid] = RC._pose(rng, k)
        pts = local
        if k:
            d = rng.standard_normal(3)
            s = local @ (d / np.linalg.norm(d))
            part = local[s >= np.quantile(s, 1 - keep)]
            pts = np.concatenate([part + noise * rng.standard_normal(part.shape), spaced_points(rng, n_outliers, lo, hi, 0.06)])
        clouds[oid] = pts @ poses[oid][:3, :3].T + poses[oid][:3, 3]
    poses[15] = RC._pose(rng, 5)
    clouds[15] = spaced_points(rng, 60, np.zeros(3), np.array([0.15, 0.15, 2.0]), 0.06) @ poses[15][:3, :3].T + poses[15][:3, 3]
    return clouds, poses, {11: 900, 12: 500, 13: 400, 14: 300, 15: 200}
