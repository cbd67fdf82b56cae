"""TEST INFRASTRUCTURE: numpy restatement of the TEASER-style solver (category_registration.TeaserSolver).
fp64 throughout, except the graph's comparison, which repeats the kernel's fp32 expression operation by operation.  Dense
boolean graph, exact maximum clique by Bron-Kerbosch with pivoting (small N), GNC-TLS rotation, adaptive voting, and the
whole solver on the restated clouds and ICP of registration_cpu.  Also the seeded planted cases the tests share."""
import json
import math
import os

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


def pair_norms32_contracted(P):
    """pair_norms32 as a compiler that contracts would evaluate it: sqrt(fma(dz, dz, fma(dx, dx, dy dy))).  The products of two
    fp32 numbers are exact in fp64; each sum is taken in fp64 and rounded once to fp32 (the fp64 sum's own rounding, 2^-29
    of an fp32 ulp, moves that only in a tie)."""
    P = np.asarray(P, np.float32)
    d = P[:, None, :] - P[None, :, :]
    return _norm32_contracted(d)


def _norm32_contracted(d):
    d64 = d.astype(np.float64)
    s = (d64[..., 0] * d64[..., 0] + (d[..., 1] * d[..., 1]).astype(np.float64)).astype(np.float32)
    s = (d64[..., 2] * d64[..., 2] + s.astype(np.float64)).astype(np.float32)
    return np.sqrt(s)


def _norm32(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def graph_contracted(A, B, noise_bound=0.01, cbar2=1.0):
    """graph() with the two multiply-adds of each norm fused.  NOT what cnr_teaser_graph promises: it exists to prove that a
    test case can tell the two apart."""
    diff = np.abs(pair_norms32_contracted(B) - pair_norms32_contracted(A))
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


def max_clique(adj, order=None):
    """the maximum clique that is lexicographically smallest in positions of `order` (default search_order(adj)) -> vertices
    in that order.  Bron-Kerbosch with a pivot of most candidates; branches that cannot reach the best size so far are cut
    (equal sizes are kept for the lexicographic choice); a greedy pass gives the first bound."""
    adj = np.asarray(adj, bool)
    N = len(adj)
    order = search_order(adj) if order is None else np.asarray(order, np.int64)
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


def search_trace(adj, KL=8, budget=1 << 20, order=None):
    """A plain-Python replay of cnr_clique_search's own search (csrc/teaser.hip: greedy_root, dfs_root in MODE_SIZE), not of
    Bron-Kerbosch: relabel by search_order, the greedy pass seeds `best`, then every root in ascending order with the
    l + |P| <= best prune, the untried candidates of levels 1..KL on a stack and every deeper level rebuilt on the way back
    from level KL's set, the rows of R[KL..l) and the bits above R[l] (a rebuild costs l - KL steps).  A root stops once it
    has spent `budget` steps.  Roots run one after the other here and each sees the others' `best` at once.  That is ONE legal
    timing: on the GPU the roots run side by side, `best` arrives later, less is pruned, and a run may spend MORE steps (in
    all and on one root) than this replay; the final size is the same whenever no root runs out of budget.
    -> dict(greedy_size, size, steps, max_root_steps, deepest_level, rebuilds, roots_out_of_budget)"""
    adj = np.asarray(adj, bool)
    N = len(adj)
    order = search_order(adj) if order is None else np.asarray(order, np.int64)
    sub = adj[np.ix_(order, order)]
    nb = [int.from_bytes(np.packbits(row, bitorder="little").tobytes(), "little") for row in sub]
    best = 1
    for v in range(N):
        P, n = nb[v] >> (v + 1) << (v + 1), 1
        while P:
            P &= nb[(P & -P).bit_length() - 1]
            n += 1
        best = max(best, n)
    out = dict(greedy_size=best, size=best, steps=0, max_root_steps=0, deepest_level=1, rebuilds=0, roots_out_of_budget=0)
    for v in range(N):
        cur, l, steps = nb[v] >> (v + 1) << (v + 1), 1, 0
        stack, R = [0] * (KL + 1), {0: v}
        while True:
            cnt = bin(cur).count("1")
            if cnt == 0 or l + cnt <= best:
                l -= 1
                if l == 0:
                    break
                if l <= KL:
                    cur = stack[l]
                else:
                    cur = stack[KL]
                    for t in range(KL, l):
                        cur &= nb[R[t]]
                    cur = cur >> (R[l] + 1) << (R[l] + 1)
                    steps += l - KL
                    out["rebuilds"] += 1
            else:
                u = (cur & -cur).bit_length() - 1
                cur &= ~(1 << u)
                if l <= KL:
                    stack[l] = cur
                R[l] = u
                cur &= nb[u]
                l += 1
                steps += 1
                out["deepest_level"] = max(out["deepest_level"], l)
                best = max(best, l)
            if steps >= budget:
                out["roots_out_of_budget"] += 1
                break
        out["steps"] += steps
        out["max_root_steps"] = max(out["max_root_steps"], steps)
    out["size"] = best
    return out


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


# ---- cases that reach the search's deep levels, its wider instantiations and the graph's threshold -------------------------
GOLDEN_CLIQUES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "teaser_cliques.json")
KL_OF_WORDS = lambda W: 4 if W > 128 else 8          # csrc/teaser.hip Levels<WPL>::KL: the candidate sets kept in LDS


def dense_graph_cases():
    """name -> adjacency.  Dense random graphs: the search goes far below level KL = 8 and backtracks there thousands of times,
    the greedy pass falls short, and several maximum cliques leave the choice to the lexicographic rule."""
    return {"dense_96": random_graph(22, 96, 0.8), "dense_120": random_graph(21, 120, 0.7)}


def embedded_case(seed, N, n_block, p_block):
    """A sparse background (every vertex linked to 3 random others) with the dense random_graph(seed + 1, n_block, p_block)
    laid over n_block random vertices: a search as deep as the block's at a width only a large N reaches."""
    rng = np.random.default_rng(seed)
    adj = np.zeros((N, N), bool)
    i, j = np.repeat(np.arange(N), 3), rng.integers(0, N, 3 * N)
    keep = i != j
    adj[i[keep], j[keep]] = adj[j[keep], i[keep]] = True
    pos = rng.permutation(N)[:n_block]
    adj[np.ix_(pos, pos)] |= random_graph(seed + 1, n_block, p_block)
    return adj


EMBEDDED = {"embedded_4200": (31, 4200, 90, 0.7), "embedded_8300": (32, 8300, 80, 0.6)}          # 66 and 130 row words


def embedded_cases():
    return {name: embedded_case(*a) for name, a in EMBEDDED.items()}


# search_trace() of the dense cases at KL = 8 and of the embedded cases at their width's KL, default budget, as measured on the
# CPU (tests/test_teaser_host.py repeats it and compares): what the GPU tests print their own step counts beside
SEARCH_TRACE_RECORD = {
    "dense_96": dict(greedy_size=16, size=20, steps=2218385, max_root_steps=177732, deepest_level=20, rebuilds=21328, roots_out_of_budget=0),
    "dense_120": dict(greedy_size=13, size=16, steps=570334, max_root_steps=34227, deepest_level=16, rebuilds=79, roots_out_of_budget=0),
    "embedded_4200": dict(greedy_size=12, size=14, steps=104933, max_root_steps=7221, deepest_level=14, rebuilds=221, roots_out_of_budget=0),
    "embedded_8300": dict(greedy_size=10, size=12, steps=12739, max_root_steps=902, deepest_level=12, rebuilds=256, roots_out_of_budget=0),
}


def expected_cliques():
    """name -> max_clique(adj) of the dense and embedded cases as recorded in tests/golden/teaser_cliques.json (Bron-Kerbosch
    takes 3 to 20 s each: tests/test_teaser_host.py repeats it and compares; the GPU tests read the record).
    `python tests/teaser_cpu.py` rewrites the record."""
    with open(GOLDEN_CLIQUES) as f:
        return {k: np.array(v, np.int64) for k, v in json.load(f).items()}


def positioned_case(N, positions, decoy=None):
    """For direct calls with order = identity: a K-clique on the vertices `positions` and a (K-1)-clique, the decoy, on
    `decoy` (default: the lowest K-1 odd indices that are no member), every other vertex isolated.  The maximum clique is
    `positions` by construction.  -> dict(N, members, decoy (ascending int64), words (N, ceil(N/64)) uint64 packed as pack()
    does, deg (N,) int32); the rows are packed directly, since a dense N = 16 379 matrix is 268 MB."""
    members = np.array(sorted(positions), np.int64)
    K = len(members)
    if decoy is None:
        decoy = [v for v in range(1, 4 * K, 2) if v not in set(members.tolist())][:K - 1]
    decoy = np.array(sorted(decoy), np.int64)
    assert len(set(members.tolist())) == K and len(decoy) == K - 1 and not set(members.tolist()) & set(decoy.tolist())
    assert 0 <= min(members.min(), decoy.min()) and max(members.max(), decoy.max()) < N
    words = np.zeros((N, (N + 63) // 64), np.uint64)
    deg = np.zeros(N, np.int32)
    for group in (members, decoy):
        for a in group:
            for b in group:
                if a != b:
                    words[a, b >> 6] |= np.uint64(1) << np.uint64(b & 63)
            deg[a] = len(group) - 1
    return dict(N=N, members=members, decoy=decoy, words=words, deg=deg)


def positioned_cases():
    """N no multiple of 64, one per instantiation of the search (66, 130 and 256 row words).  The members straddle bit 63/64
    (words 0/1), words 63/64 (the first and second word of a lane), 127/128, 191/192 (where N reaches them), and end in the
    last, partial word -- on its last bit."""
    out = {}
    for N in (4161, 8257, 16384 - 5):
        last = (N - 1) >> 6 << 6
        pos = [40, 63, 64] + [b + k for b in (4096, 8192, 12288) if b < last for k in (-1, 0)] + sorted({last, N - 1})
        out["positioned_%d" % N] = positioned_case(N, pos)
    return out


LATTICE_NOISE_BOUND = 0.0625          # threshold exactly 0.125


def lattice_case(N=1500, seed=5):
    """A = integers in [0, 64) / 64; B = A with one axis moved by k / 64, k in [-8, 8].  Every difference and every sum of
    squares is a multiple of 1/64 or 1/4096 below 2^24 of them, hence exact in fp32, and whenever both sums are perfect squares
    | |b_i - b_j| - |a_i - a_j| | is an exact multiple of 1/64: pairs sit EXACTLY at the threshold 0.125, where <= and < differ.
    -> (A, B) f32; the noise bound is LATTICE_NOISE_BOUND"""
    rng = np.random.default_rng(seed)
    A = (rng.integers(0, 64, (N, 3)) / 64).astype(np.float32)
    B = A.copy()
    B[np.arange(N), rng.integers(0, 3, N)] += (rng.integers(-8, 9, N) / 64).astype(np.float32)
    return A, B


def contraction_case(n_pairs=256, seed=17, scale=1.5, noise_bound=0.01):
    """Correspondences on which graph() and graph_contracted() disagree, found by search: B = fp32(scale A), so a pair's
    | |b_i - b_j| - |a_i - a_j| | is (scale - 1) |a_i - a_j| up to rounding; candidate pairs (2k, 2k + 1) are drawn at the
    distance thr / (scale - 1) in a random direction, where the rounding of the coordinates spreads the difference over some
    tens of ulp around the threshold, and the first n_pairs pairs whose edge the contracted evaluation flips are kept (all in a
    0.5 m box: the other pairs lie anywhere and seldom near the threshold).  -> (A, B) f32, N = 2 n_pairs"""
    rng = np.random.default_rng(seed)
    thr = threshold32(noise_bound)
    dist = float(thr) / (scale - 1.0)
    found_p, found_q = [], []
    while sum(len(x) for x in found_p) < n_pairs:
        p = rng.random((1 << 16, 3)) * 0.5
        u = rng.standard_normal((1 << 16, 3))
        q = p + dist * u / np.linalg.norm(u, axis=1, keepdims=True)
        p, q = p.astype(np.float32), q.astype(np.float32)
        bp, bq = (np.float32(scale) * p), (np.float32(scale) * q)
        plain = np.abs(_norm32(bq - bp) - _norm32(q - p)) <= thr
        fused = np.abs(_norm32_contracted(bq - bp) - _norm32_contracted(q - p)) <= thr
        found_p.append(p[plain != fused])
        found_q.append(q[plain != fused])
    p, q = np.concatenate(found_p)[:n_pairs], np.concatenate(found_q)[:n_pairs]
    A = np.empty((2 * n_pairs, 3), np.float32)
    A[0::2], A[1::2] = p, q
    return A, np.float32(scale) * A


def threshold_cases():
    """name -> (A, B, noise_bound): graph cases compared bit for bit WITHOUT the guard of graph_cases(): the lattice case has
    pairs exactly at the threshold, the contraction case pairs that a fused multiply-add flips, and the planted case of 4161
    correspondences (66 row words: no multiple of the graph kernel's 4 waves, a last word of one bit) is a natural input."""
    c = planted_case(12, max_correspondences=4161, n_template=80, n_keep=80)
    return {"lattice": lattice_case() + (LATTICE_NOISE_BOUND,), "contraction": contraction_case() + (0.01,),
            "planted_4161": (c["A"], c["B"], 0.01)}


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


if __name__ == "__main__":      # rewrites tests/golden/teaser_cliques.json (about a minute of Bron-Kerbosch)
    record = {name: [int(v) for v in max_clique(adj)] for name, adj in {**dense_graph_cases(), **embedded_cases()}.items()}
    with open(GOLDEN_CLIQUES, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print({k: len(v) for k, v in record.items()})
