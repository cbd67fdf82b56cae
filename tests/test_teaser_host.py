"""CPU: the TEASER-style solver's host side.  The guard that lets tests/test_teaser_gpu.py compare the graph
bit for bit, the planted case on the restatement alone, GNC-TLS and the voting (product and restatement) under gross outliers,
and the public signatures with their ABI rows."""
import inspect
import math

import numpy as np
import pytest

import teaser_cpu as TC
from test_abi import assert_row_matches, declared_functions, declared_int64_returns

SIGMA = 0.002          # the planted cases' noise per axis


@pytest.fixture(scope="module")
def CR():
    import cnr_amd
    return cnr_amd.category_registration


def test_graph_cases_have_no_pair_at_the_threshold():
    """Every graph case of the GPU test: no pair's | |b_i - b_j| - |a_i - a_j| | lies within 8 ulp (of the larger norm) of the
    threshold, by the restatement alone.  A correctly rounded fp32 evaluation in any order differs by a few ulp at most, so
    the adjacency may be compared bit for bit."""
    cases = TC.graph_cases()
    sizes = sorted(len(A) for A, _ in cases.values())
    assert sizes[0] == 1 and any(n % 64 for n in sizes[1:]) and sizes[-1] > 2000
    for name, (A, B) in cases.items():
        margin = TC.threshold_margin(A, B)
        print(name, len(A), "margin", margin, "ulp")
        assert margin >= 8.0, (name, margin)


def test_planted_clique_is_the_inlier_set_with_a_margin():
    """60 template points kept, posed, 2 mm noise, 20 unrelated points, 4800 pairs sub-sampled to 2500.  The exact maximum clique
    holds true correspondences only -- all that survived the sub-sampling -- and is at least 10 vertices larger than the largest
    clique among the other vertices."""
    c = TC.planted_case(3)
    assert len(c["A"]) == 2500
    adj = TC.graph(c["A"], c["B"])
    clique = TC.max_clique(adj)
    assert TC.is_clique(adj, clique)
    assert c["inliers"][clique].all() and len(clique) == int(c["inliers"].sum())
    others = np.flatnonzero(~c["inliers"])
    rival = TC.max_clique(adj[np.ix_(others, others)])
    print("clique", len(clique), "largest clique among non-inliers", len(rival))
    assert len(clique) - len(rival) >= 10


def _corrupted_clique(seed=3, share=0.3):
    c = TC.planted_case(seed)
    members = np.flatnonzero(c["inliers"])
    a, b = c["A"][members].astype(np.float64), c["B"][members].astype(np.float64)
    rng = np.random.default_rng(seed + 100)
    bad = rng.permutation(len(a))[:int(round(share * len(a)))]
    b[bad] = rng.random((len(bad), 3)) * [1.0, 0.8, 0.6] + [0.5, -0.4, 0.3]          # gross: tens of centimetres off
    good = np.ones(len(a), bool)
    good[bad] = False
    return a, b, good, np.linalg.inv(c["pose"])


def _pose_bounds(a, good):
    """What 2 mm noise allows.  A chain measurement a_(k+1) - a_k of two clean members carries noise sigma sqrt(2) per axis.
    The least-squares rotation about an axis has the variance 2 sigma^2 / sum |a_perp|^2, and on average 2/3 of a measurement's
    squared length is perpendicular to the axis; three axes, five standard deviations.  The translation is the mean of the clean
    b - R a: sigma / sqrt(n) per axis (three axes, five standard deviations), plus the rotation's error times the distance of
    the points from the origin."""
    nxt = (np.arange(len(a)) + 1) % len(a)
    clean = good & good[nxt]
    lever = float(((a[nxt] - a)[clean] ** 2).sum()) * 2.0 / 3.0
    rot = 5.0 * math.sqrt(3.0) * math.sqrt(2.0) * SIGMA / math.sqrt(lever)
    tr = 5.0 * math.sqrt(3.0) * SIGMA / math.sqrt(int(good.sum())) + rot * float(np.linalg.norm(a, axis=1).max())
    return rot, tr


def _angle(R, R_true):
    return math.acos(min(1.0, max(-1.0, (np.trace(R.T @ R_true) - 1.0) / 2.0)))


def test_rotation_and_translation_survive_gross_outliers(CR):
    a, b, good, T_true = _corrupted_clique()
    assert 0.29 < 1 - good.mean() < 0.31
    rot_bound, tr_bound = _pose_bounds(a, good)
    print("bounds: rotation %.3g rad, translation %.3g m" % (rot_bound, tr_bound))
    ta, tb = TC.chain(a, b)
    bound = (2 * 0.01) ** 2
    R_ref, its_ref = TC.gnc_tls(ta, tb, bound)
    R, its, w = CR.gnc_tls_rotation(ta, tb, bound)
    t_ref = np.array([TC.vote((b - a @ R_ref.T)[:, k], 0.01) for k in range(3)])
    t = CR.tls_translation(a, b, R, 0.01, 1.0)
    for name, (Rk, tk, n) in {"restatement": (R_ref, t_ref, its_ref), "product": (R, t, its)}.items():
        err = (_angle(Rk, T_true[:3, :3]), float(np.linalg.norm(tk - T_true[:3, 3])))
        print(name, "rotation error %.3g rad, translation error %.3g m, %d iterations" % (err + (n,)))
        assert err[0] <= rot_bound and err[1] <= tr_bound, (name, err)
        assert 1 < n <= 100
    assert np.allclose(R, R_ref, atol=1e-12) and np.allclose(t, t_ref, atol=1e-12) and its == its_ref
    nxt = (np.arange(len(a)) + 1) % len(a)
    assert (w[~(good & good[nxt])] < 0.5).all() and (w[good & good[nxt]] > 0.5).all()          # the weights name the outliers


def test_voting_picks_the_largest_consensus(CR):
    x = np.r_[0.300, 0.302, 0.297, 0.301, 0.299, 0.9, -0.4, 0.52, 0.53]
    t, inside = CR.tls_scalar(x, 0.01)
    assert abs(t - x[:5].mean()) < 1e-15 and inside.tolist() == [True] * 5 + [False] * 4
    assert abs(TC.vote(x, 0.01) - t) < 1e-15


def test_signatures_and_defaults(CR):
    p = inspect.signature(CR.TeaserSolver.__init__).parameters
    want = dict(voxel_size=0.1, noise_bound=0.01, max_correspondences=10000, cbar2=1.0, gnc_factor=1.4, rotation_max_iterations=100,
                rotation_cost_threshold=1e-12, icp_max_iteration=100, seed=0, search_budget=None, icp_max_corr=None)
    assert {k: v.default for k, v in p.items() if k != "self"} == want
    assert list(inspect.signature(CR.TeaserSolver.__call__).parameters) == ["self", "source", "templates"]
    defaults = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults(CR.teaser_correspondences) == dict(voxel_size=0.1, max_correspondences=10000, rng=None, device=None)
    assert defaults(CR.compatibility_graph) == dict(noise_bound=0.01, cbar2=1.0)
    assert defaults(CR.max_clique) == dict(search_budget=None)
    assert defaults(CR.gnc_tls_rotation) == dict(gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12)
    assert defaults(CR.tls_translation) == dict(noise_bound=0.01, cbar2=1.0)
    assert CR.compatibility_threshold() == float(TC.threshold32()) and CR.DEFAULT_SEARCH_BUDGET >= 1
    assert inspect.signature(CR.align_poses).parameters["solver"].default is None          # the default solver stays IcpSolver


def test_abi_rows_of_the_new_symbols():
    import cnr_amd
    fns, sig = declared_functions(), cnr_amd._C.SIGNATURES
    for name, n_args in (("cnr_teaser_graph", 7), ("cnr_clique_workspace_bytes", 2), ("cnr_clique_search", 9)):
        assert name in fns and name in sig and len(fns[name]) == len(sig[name]) == n_args, name
        assert_row_matches(name, sig[name], fns[name])
    assert "cnr_clique_workspace_bytes" in cnr_amd._C._RESTYPE64 and "cnr_clique_workspace_bytes" in declared_int64_returns()
    lib = cnr_amd._C.load()
    assert lib.cnr_teaser_graph(None, None, 4, 0.02, None, None, None) == -1
    assert lib.cnr_clique_search(None, None, 4, 3, 10, None, None, None, None) == -1
    assert lib.cnr_clique_workspace_bytes(0, 0) < 0 and lib.cnr_clique_workspace_bytes(cnr_amd.category_registration.TEASER_MAX_N + 1, 5) < 0
    assert lib.cnr_clique_workspace_bytes(1, 0) > 0 and lib.cnr_clique_workspace_bytes(10000, 1800) > 10000 * 157 * 8


# ---- the cases of tests/test_teaser_gpu.py that pin the search's deep levels, its wider instantiations and the graph's threshold:
# each can fail for the reason it exists, by the restatement alone (conditions, not measurements) ------------------------------
def _budget(CR):
    return CR.DEFAULT_SEARCH_BUDGET


@pytest.mark.parametrize("name,min_rebuilds", [("dense_96", 1000), ("dense_120", 50)])
def test_dense_cases_rebuild_deep_levels_and_outrun_the_greedy_pass(CR, name, min_rebuilds):
    adj = TC.dense_graph_cases()[name]
    KL = TC.KL_OF_WORDS((len(adj) + 63) // 64)
    assert KL == 8
    tr = TC.search_trace(adj, KL, _budget(CR))
    print(name, tr)
    assert tr == TC.SEARCH_TRACE_RECORD[name]
    assert tr["rebuilds"] >= min_rebuilds and tr["deepest_level"] >= KL + 4 and tr["roots_out_of_budget"] == 0
    assert tr["max_root_steps"] <= _budget(CR) // 4          # headroom for the GPU's later `best`
    want = TC.max_clique(adj)
    assert TC.is_clique(adj, want) and tr["greedy_size"] < tr["size"] == len(want)
    assert np.array_equal(want, TC.expected_cliques()[name])          # the record the GPU test reads


@pytest.mark.parametrize("name,words,KL", [("embedded_4200", range(65, 129), 8), ("embedded_8300", range(129, 257), 4)])
def test_embedded_cases_reach_the_wide_instantiations_with_rebuilds(CR, name, words, KL):
    adj = TC.embedded_cases()[name]
    W = (len(adj) + 63) // 64
    assert W in words and TC.KL_OF_WORDS(W) == KL and len(adj) % 64
    tr = TC.search_trace(adj, KL, _budget(CR))
    print(name, tr)
    assert tr == TC.SEARCH_TRACE_RECORD[name]
    assert tr["rebuilds"] >= 10 and tr["roots_out_of_budget"] == 0 and tr["max_root_steps"] <= _budget(CR) // 4
    want = TC.max_clique(adj)
    assert TC.is_clique(adj, want) and tr["size"] == len(want)
    assert np.array_equal(want, TC.expected_cliques()[name])


def test_positioned_cases_straddle_the_word_boundaries():
    cases = TC.positioned_cases()
    assert sorted(c["N"] for c in cases.values()) == [4161, 8257, 16379]
    for name, c in cases.items():
        N, m = c["N"], set(c["members"].tolist())
        W = (N + 63) // 64
        assert N % 64 and c["words"].shape == (N, W)
        assert {63, 64} <= m                                                   # bit 63 of word 0, bit 0 of word 1
        for w in (64, 128, 192):                                               # the lane's next word
            if w < W - 1:
                assert {64 * w - 1, 64 * w} <= m, (name, w)
        assert N - 1 in m and (N - 1) >> 6 == W - 1 and N < 64 * W             # the last bit of the last, partial word
        assert max(m) >> 12 == (W - 1) // 64                                   # a member in the lane's last word index
        # the answer, by construction and by Bron-Kerbosch on the vertices that have an edge at all
        live = np.flatnonzero(c["deg"] > 0)
        assert set(live.tolist()) == m | set(c["decoy"].tolist())
        sub = TC.unpack(c["words"][live], N)[:, live]
        assert (sub == sub.T).all() and np.array_equal(sub.sum(1), c["deg"][live])
        got = live[TC.max_clique(sub, order=np.arange(len(live)))]
        assert np.array_equal(got, c["members"]) and len(c["decoy"]) == len(got) - 1
        assert c["decoy"].max() < 64 and c["decoy"].min() < c["members"].min()          # what a search blind beyond word 0 finds first


def test_lattice_case_has_pairs_exactly_at_the_threshold():
    A, B = TC.lattice_case()
    thr = TC.threshold32(TC.LATTICE_NOISE_BOUND)
    assert float(thr) == 0.125 and len(A) == 1500
    diff = np.abs(TC.pair_norms32(B) - TC.pair_norms32(A))
    at = np.triu(diff == thr, 1)
    print("pairs exactly at the threshold", int(at.sum()))
    assert int(at.sum()) >= 16                                                 # <= and < differ on them
    le = diff <= thr
    np.fill_diagonal(le, False)
    assert np.array_equal(le, TC.graph(A, B, TC.LATTICE_NOISE_BOUND))


def test_contraction_case_tells_a_fused_multiply_add_from_the_promised_chain():
    A, B = TC.contraction_case()
    assert len(A) <= 2048
    plain, fused = TC.graph(A, B), TC.graph_contracted(A, B)
    differ = int(np.triu(plain != fused, 1).sum())
    print("N", len(A), "edges", int(plain.sum()) // 2, "edges a contracted evaluation flips", differ)
    assert differ >= 16
