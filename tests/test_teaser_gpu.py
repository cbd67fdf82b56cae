"""GPU: the TEASER-style solver (csrc/teaser.hip, category_registration.TeaserSolver) against the restatement
tests/teaser_cpu.py: the graph bit for bit on the guarded cases and on unguarded ones (pairs exactly at the threshold, pairs a
fused multiply-add flips), the clique on graphs small enough for Bron-Kerbosch -- among them dense ones that rebuild deep
levels thousands of times and embedded or positioned ones for the two wider instantiations of the search -- and on the planted
construction at N = 10 000, the budget at every scale, the max_degree and order guards by direct calls, align_poses end to
end, and rigid-copy templates.  tests/test_teaser_host.py proves by the restatement alone that each case can fail for its reason."""
import time

import numpy as np
import pytest
import torch

import registration_cpu as RC
import teaser_cpu as TC

pytestmark = pytest.mark.gpu
ETA1, ETA2, ETA3 = 0.06, 0.15, 0.12

# Measured with the fp64 restatement (teaser_cpu.TeaserSolverCpu(voxel 0.02, noise bound 0.01, 2500 correspondences) under
# registration_cpu.align_poses_cpu) on teaser_cpu.registration_case(41), 2026-10-17, `python tests/test_teaser_gpu.py`: per
# copy (rotation degrees, translation metres) and the normalised one-sided chamfer distances the eta rule saw.
RESTATEMENT_ERRORS = {12: (0.12066950169926616, 0.0007324473318671346), 13: (0.07834972282625795, 0.00025247986218847215),
                      14: (0.09614347524642863, 0.0004944592194280635)}
RESTATEMENT_CHAMFER = {12: 0.024031344618568658, 13: 0.026508661863545547, 14: 0.02429868435039522, 15: 0.3491705397401282}
# registration_cpu.IcpSolverCpu(0.02, 0.10) on the same inputs, same run (no assertion): 12 (0.699 deg, 4.2 mm), 14 (0.953 deg,
# 3.8 mm); copy 13 is not aligned (chamfer 0.169 > eta2) and leaves the class.


@pytest.fixture(scope="module")
def CR():
    import cnr_amd
    return cnr_amd.category_registration


def _dev_graph(adj_bool, dev):
    words = TC.pack(adj_bool)
    return (torch.from_numpy(words.view(np.int64)).to(dev).contiguous(),
            torch.from_numpy(adj_bool.sum(1).astype(np.int32)).to(dev))


def _host_adj(adj, N):
    return TC.unpack(adj.cpu().numpy().view(np.uint64), N)


@pytest.mark.parametrize("name", ["planted_2500", "planted_1000", "n65", "n1"])
def test_graph_equals_the_restatement_bit_for_bit_gpu(dev, CR, name):
    A, B = TC.graph_cases()[name]
    want = TC.graph(A, B)
    dA, dB = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    adj, deg = CR.compatibility_graph(dA, dB)
    assert np.array_equal(adj.cpu().numpy().view(np.uint64), TC.pack(want))          # the padding bits too
    assert np.array_equal(deg.cpu().numpy(), want.sum(1))
    adj2, deg2 = CR.compatibility_graph(dA, dB)
    assert torch.equal(adj, adj2) and torch.equal(deg, deg2)


def _check_against_restatement(CR, dev, adj_bool, want=None):
    want = TC.max_clique(adj_bool) if want is None else want
    adj, deg = _dev_graph(adj_bool, dev)
    got, info = CR.max_clique(adj, deg)
    print("clique", len(got), "restatement", len(want), info)
    assert info["exact"] and info["size"] == len(got) == len(want)
    assert TC.is_clique(adj_bool, got)
    assert np.array_equal(got, want)
    assert np.array_equal(CR.clique_order(deg).cpu().numpy(), TC.search_order(adj_bool))
    again, info2 = CR.max_clique(adj, deg)
    assert np.array_equal(got, again) and info2["size"] == info["size"] and info2["exact"]
    return got, info


def test_clique_on_the_planted_case_gpu(dev, CR):
    c = TC.planted_case(3)
    got, _ = _check_against_restatement(CR, dev, TC.graph(c["A"], c["B"]))
    assert c["inliers"][got].all() and len(got) == int(c["inliers"].sum())


@pytest.mark.parametrize("seed,N,density", [(1, 1000, 0.06), (2, 200, 0.3), (7, 2500, 0.06), (8, 130, 0.3), (9, 1, 0.3)])
def test_clique_on_random_graphs_gpu(dev, CR, seed, N, density):
    _check_against_restatement(CR, dev, TC.random_graph(seed, N, density))


def test_clique_at_ten_thousand_correspondences_gpu(dev, CR):
    """the planted construction at the reference's size: 160 template points, 60 kept + 20 unrelated, 12 800 pairs -> 10 000"""
    c = TC.planted_case(11, n_template=160, max_correspondences=10000)
    assert len(c["A"]) == 10000
    adj, deg = CR.compatibility_graph(torch.from_numpy(c["A"]).to(dev), torch.from_numpy(c["B"]).to(dev))
    torch.cuda.synchronize()
    t = time.perf_counter()
    got, info = CR.max_clique(adj, deg)
    ms = (time.perf_counter() - t) * 1e3
    own = _host_adj(adj, 10000)
    print("N 10000: edges", int(own.sum()) // 2, "max degree", int(deg.max()), "clique", len(got), "planted", int(c["inliers"].sum()),
          info, "%.1f ms" % ms)
    assert (own == own.T).all() and TC.is_clique(own, got)
    assert len(got) >= int(c["inliers"].sum())
    assert info["exact"] and info["roots_out_of_budget"] == 0


def test_a_tiny_budget_ends_promptly_and_inexact_gpu(dev, CR):
    c = TC.planted_case(3)
    adj_bool = TC.graph(c["A"], c["B"])
    adj, deg = _dev_graph(adj_bool, dev)
    torch.cuda.synchronize()
    t = time.perf_counter()
    got, info = CR.max_clique(adj, deg, search_budget=2)
    seconds = time.perf_counter() - t
    print("budget 2:", info, "%.3f s" % seconds)
    assert not info["exact"] and info["roots_out_of_budget"] > 0 and info["max_root_steps"] <= 2 + 2500
    assert len(got) >= 1 and TC.is_clique(adj_bool, got)
    assert seconds < 5.0


# ---- deep levels, the wider instantiations, the budget and the guards ----------------------------------------------------------
SENTINEL = -77


def _print_steps(name, info):
    print(name, "GPU steps", info["steps"], "find_steps", info["find_steps"], "max_root_steps", info["max_root_steps"],
          "| search_trace (one root after the other)", TC.SEARCH_TRACE_RECORD[name])


@pytest.mark.parametrize("name", ["dense_96", "dense_120"])
def test_clique_on_dense_graphs_that_rebuild_deep_levels_gpu(dev, CR, name):
    """levels far beyond KL = 8 with thousands of backtracks there (dfs_root's rebuild branch), several maximum cliques"""
    got, info = _check_against_restatement(CR, dev, TC.dense_graph_cases()[name], TC.expected_cliques()[name])
    _print_steps(name, info)
    assert info["roots_out_of_budget"] == 0 and info["flags"] == 0
    assert info["greedy_size"] == TC.SEARCH_TRACE_RECORD[name]["greedy_size"] < info["size"]          # the greedy pass has no timing


@pytest.mark.parametrize("name", ["embedded_4200", "embedded_8300"])
def test_clique_in_the_wide_instantiations_gpu(dev, CR, name):
    """66 and 130 row words: two and four words per lane (KL = 8 and 4), with rebuilds, against the exact answer"""
    got, info = _check_against_restatement(CR, dev, TC.embedded_case(*TC.EMBEDDED[name]), TC.expected_cliques()[name])
    _print_steps(name, info)
    assert info["roots_out_of_budget"] == 0 and info["flags"] == 0


def _direct_search(dev, words, order, max_degree, budget, alloc_degree=None):
    """cnr_clique_search itself -> (clique_out whole, info as max_clique names it); buffers sized for alloc_degree, clique_out
    filled with SENTINEL"""
    import cnr_amd
    _C, N = cnr_amd._C, len(words)
    alloc = max_degree if alloc_degree is None else alloc_degree
    adj = torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(dev).contiguous()
    order = torch.from_numpy(np.asarray(order, np.int32)).to(dev)
    ws = torch.zeros(int(_C.load().cnr_clique_workspace_bytes(N, alloc)), device=dev, dtype=torch.uint8)
    out = torch.full((alloc + 1,), SENTINEL, device=dev, dtype=torch.int32)
    info = torch.zeros(8, device=dev, dtype=torch.int64)
    _C.call("cnr_clique_search", adj, order, N, int(max_degree), int(budget), ws, out, info)
    keys = ("size", "exact", "steps", "find_steps", "max_root_steps", "roots_out_of_budget", "greedy_size", "flags")
    return out.cpu().numpy().astype(np.int64), dict(zip(keys, (int(x) for x in info.cpu())))


@pytest.mark.parametrize("name", ["positioned_4161", "positioned_8257", "positioned_16379"])
def test_clique_members_across_word_boundaries_gpu(dev, CR, name):
    """identity order: the members sit on bits 63/64, words 63/64, 127/128, 191/192 and the last bit of the last, partial word"""
    c = TC.positioned_cases()[name]
    K = len(c["members"])
    out, info = _direct_search(dev, c["words"], np.arange(c["N"]), K - 1, CR.DEFAULT_SEARCH_BUDGET)
    print(name, info, out)
    assert info["size"] == K and info["exact"] == 1 and info["flags"] == 0 and info["roots_out_of_budget"] == 0
    assert np.array_equal(out[:K], c["members"]) and (out[K:] == SENTINEL).all()
    assert info["greedy_size"] == K


def test_budget_sweep_never_reports_a_wrong_exact_answer_gpu(dev, CR):
    """dense_96 at budgets from 1 to the default: always a clique between the greedy and the true size, a root's steps within
    budget + cap, and whatever is called exact IS the restatement's clique.  (Inexact results may differ run to run: which
    roots run out depends on when `best` arrives; so nothing is asserted about them between runs.)"""
    adj_bool, want = TC.dense_graph_cases()["dense_96"], TC.expected_cliques()["dense_96"]
    adj, deg = _dev_graph(adj_bool, dev)
    cap = int(adj_bool.sum(1).max()) + 1
    for budget in (1, 8, 64, 512, 4096, 32768, None):
        got, info = CR.max_clique(adj, deg, search_budget=budget)
        print("budget", budget, info)
        b = CR.DEFAULT_SEARCH_BUDGET if budget is None else budget
        assert TC.is_clique(adj_bool, got) and info["size"] == len(got)
        assert info["greedy_size"] <= info["size"] <= len(want)
        assert info["greedy_size"] == TC.SEARCH_TRACE_RECORD["dense_96"]["greedy_size"]
        assert info["max_root_steps"] <= b + cap
        if info["exact"]:
            assert np.array_equal(got, want) and info["roots_out_of_budget"] == 0, budget
        if budget == 1:
            assert not info["exact"] and info["roots_out_of_budget"] > 0
        if budget is None:
            assert info["exact"] and info["roots_out_of_budget"] == 0


def test_an_understated_max_degree_is_caught_gpu(dev, CR):
    """A 40-clique laid over a sparse graph, searched with half the true maximum degree stated: fewer levels than the clique
    has.  The buffers are sized for the TRUE degree, so a broken guard writes into owned memory and shows on the sentinel."""
    adj_bool = TC.random_graph(5, 150, 0.1)
    members = np.random.default_rng(50).permutation(150)[:40]
    adj_bool[np.ix_(members, members)] = ~np.eye(40, dtype=bool)
    true_max = int(adj_bool.sum(1).max())
    stated = true_max // 2
    assert stated + 1 < 40 <= true_max + 1
    out, info = _direct_search(dev, TC.pack(adj_bool), TC.search_order(adj_bool), stated, CR.DEFAULT_SEARCH_BUDGET, alloc_degree=true_max)
    print("true max degree", true_max, "stated", stated, info)
    assert info["flags"] & 1 and info["exact"] == 0
    assert 1 <= info["size"] <= stated + 1
    assert (out[info["size"]:] == SENTINEL).all()
    assert TC.is_clique(adj_bool, out[:info["size"]])


def test_order_entries_outside_the_range_read_as_isolated_vertices_gpu(dev, CR):
    """Two members of the maximum clique lose their entry of `order` (-1 and N): their positions have no edge, the answer is the
    restatement's on the graph without those two vertices, in positions of the same order."""
    adj_bool = TC.random_graph(2, 200, 0.3)
    N, order, first = 200, TC.search_order(adj_bool), TC.max_clique(adj_bool)
    gone = first[[0, -1]]
    cleared = adj_bool.copy()
    cleared[gone, :] = cleared[:, gone] = False
    want = TC.max_clique(cleared, order=order)
    assert len(want) > 1 and not set(want.tolist()) & set(gone.tolist())
    broken = order.copy()
    broken[np.flatnonzero(order == gone[0])], broken[np.flatnonzero(order == gone[1])] = -1, N
    max_degree = int(adj_bool.sum(1).max())
    out, info = _direct_search(dev, TC.pack(adj_bool), broken, max_degree, CR.DEFAULT_SEARCH_BUDGET)
    print(info, out[:info["size"]], "restatement", want, "with every vertex", first)
    assert info["size"] == len(want) and info["exact"] == 1 and info["flags"] == 0
    assert np.array_equal(out[:len(want)], want) and (out[len(want):] == SENTINEL).all()


@pytest.mark.parametrize("name", ["lattice", "contraction", "planted_4161"])
def test_unguarded_graph_equals_the_restatement_bit_for_bit_gpu(dev, CR, name):
    """No vertex dropped: pairs exactly at the threshold (<= against <), pairs that a fused multiply-add flips, and a natural
    input of 66 row words.  The header promises single correctly rounded fp32 operations in a fixed order; that is compared."""
    A, B, noise_bound = TC.threshold_cases()[name]
    want = TC.graph(A, B, noise_bound)
    adj, deg = CR.compatibility_graph(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), noise_bound=noise_bound)
    got = _host_adj(adj, len(A))
    if not np.array_equal(got, want):
        thr = TC.threshold32(noise_bound)
        na, nb, ca, cb = TC.pair_norms32(A), TC.pair_norms32(B), TC.pair_norms32_contracted(A), TC.pair_norms32_contracted(B)
        ulps = lambda x, y: (np.float64(np.abs(np.float32(y - x))) - np.float64(thr)) / np.float64(np.spacing(thr))
        for i, j in list(zip(*np.nonzero(np.triu(got != want))))[:20]:
            print("pair", i, j, "GPU", got[i, j], "restatement", want[i, j], "| chain: |a|", na[i, j], "|b|", nb[i, j], "difference - thr",
                  ulps(na[i, j], nb[i, j]), "ulp | contracted: |a|", ca[i, j], "|b|", cb[i, j], "difference - thr", ulps(ca[i, j], cb[i, j]), "ulp")
    assert np.array_equal(adj.cpu().numpy().view(np.uint64), TC.pack(want))          # the padding bits too
    assert np.array_equal(deg.cpu().numpy(), want.sum(1))


def _solver(CR, **kw):
    return CR.TeaserSolver(voxel_size=TC.REG_VOXEL, max_correspondences=TC.REG_MAX_CORR, **kw)


def test_teaser_solver_aligns_partial_copies_through_align_poses_gpu(dev, CR):
    """Bound: 2 x the fp64 restatement's own errors on the same inputs (fp32 distances move the ICP's fixed point)."""
    import cnr_amd
    clouds, poses, counts = TC.registration_case()
    inst, bbox, cnt, pe, fc = RC.build_dicts(clouds, counts, lambda p: cnr_amd.utils.PointCloud(p, device=dev))
    solver = _solver(CR)
    info = CR.align_poses(inst, bbox, cnt, pe, fc, name="replica", eta1=ETA1, eta2=ETA2, eta3=ETA3, device=str(dev), solver=solver)
    print("chamfer", info["chamfer"], "last_info", {k: v for k, v in solver.last_info.items() if k not in ("groups", "clique")})
    for v in RESTATEMENT_CHAMFER.values():
        assert v < 0.75 * ETA1 or v > 1.25 * ETA2
    assert list(inst.keys()) == [7, 107] and list(inst[107].keys()) == [15] and list(inst[7].keys()) == [11, 12, 13, 14]
    errs = RC.pose_errors(inst, poses)
    print("pose errors (degrees, metres)", errs)
    for oid, (rot, tr) in errs.items():
        ref_rot, ref_tr = RESTATEMENT_ERRORS[oid]
        assert rot <= 2 * ref_rot and tr <= 2 * ref_tr, (oid, rot, tr, ref_rot, ref_tr)
    li = solver.last_info
    assert li["graph_builds"] == 1 and li["rigid_copies"] and li["exact"] and li["N"] == TC.REG_MAX_CORR
    assert set(("N", "edges", "clique_size", "exact", "gnc_iterations", "icp_state")) <= set(li)


def test_rigid_copy_templates_equal_one_by_one_solves_gpu(dev, CR):
    """24 rigid copies of the template in one call (one graph, one clique) against 24 calls with one template each.  In each
    the ICP ends on fixed pairs, where one more update moves fitness and rmse by less than 1e-6: the poses agree to 1e-5 (metres,
    and radians over a cloud of about 1 m), ten times that tolerance."""
    import cnr_amd
    clouds, poses, _ = TC.registration_case()
    S = cnr_amd.utils.get_possible_transform_from_bbox()
    assert len(S) == 24
    src = torch.from_numpy(clouds[12].T[None].copy()).to(dev)
    tmpl = np.stack([cnr_amd.utils.transform_pointcloud(clouds[11], Sk).T for Sk in S])
    solver = _solver(CR)
    R, t = solver(src, torch.from_numpy(tmpl).to(dev))
    assert solver.last_info["graph_builds"] == 1 and solver.last_info["rigid_copies"]
    assert R.shape == (24, 3, 3) and t.shape == (24, 3, 1)
    worst = 0.0
    for k in range(24):
        one = _solver(CR)
        Rk, tk = one(src, torch.from_numpy(tmpl[k:k + 1].copy()).to(dev))
        assert one.last_info["graph_builds"] == 1
        worst = max(worst, float((Rk[0] - R[k]).abs().max()), float((tk[0] - t[k]).abs().max()))
    print("largest difference", worst)
    assert worst <= 1e-5


def test_templates_that_are_no_copies_are_solved_one_by_one_gpu(dev, CR):
    clouds, poses, _ = TC.registration_case()
    src = torch.from_numpy(clouds[12].T[None].copy()).to(dev)
    other = clouds[11] * [1.0, 1.0, 1.05]                      # stretched: no rigid copy
    solver = _solver(CR)
    R, t = solver(src, torch.from_numpy(np.stack([clouds[11].T, other.T])).to(dev))
    assert solver.last_info["graph_builds"] == 2 and not solver.last_info["rigid_copies"] and R.shape == (2, 3, 3)


if __name__ == "__main__":      # the CPU measurement behind RESTATEMENT_ERRORS / RESTATEMENT_CHAMFER and the IcpSolver note
    import cnr_amd
    for name, solver in (("TeaserSolverCpu", TC.TeaserSolverCpu(TC.REG_VOXEL, 0.01, TC.REG_MAX_CORR)),
                         ("IcpSolverCpu", RC.IcpSolverCpu(0.02, 0.10, get_bound=cnr_amd.utils.get_bound))):
        clouds, poses, counts = TC.registration_case()
        inst, bbox, cnt, pe, fc = RC.build_dicts(clouds, counts, RC.CpuCloud)
        ch = RC.align_poses_cpu(inst, bbox, cnt, pe, fc, solver, cnr_amd.utils, eta1=ETA1, eta2=ETA2, eta3=ETA3)
        print(name, "classes", {c: list(d.keys()) for c, d in inst.items()})
        print(" RESTATEMENT_ERRORS =", RC.pose_errors(inst, poses))
        print(" RESTATEMENT_CHAMFER =", ch)
