"""No GPU: the sampler's restatement (tests/sampler_cpu.py) against things independent of it -- the published Philox4x32-10
known answers, the counter layout's own disjointness (and the overlap beyond S = 256 that cnr_sample_rays refuses), the moments
of the Box-Muller draws -- and the conditions the case builder promises tests/test_sampler_gpu.py."""
import numpy as np
import pytest
import torch

import modular_cases as M
import sampler_cpu as SC

F32, F64 = torch.float32, torch.float64


# ---- Philox4x32-10: the Random123 known answers ------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = SC.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and tuple(int(v) for v in got.reshape(-1)) == want
    # ... and through the sampler's packing: seed = key, (ctr_lo, ctr_hi) = the counter, low word first
    got = SC.philox4(key[0] | key[1] << 32, ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32)
    assert tuple(int(v) for v in got.reshape(-1)) == want


def test_philox_is_vectorised_and_u01_is_a_24_bit_grid():
    lo = np.arange(5, dtype=np.uint64)[:, None] + (np.uint64(1) << np.uint64(40))
    hi = np.arange(3, dtype=np.uint64)[None, :]
    w = SC.philox4(2 ** 40 + 3, lo, hi)
    assert w.shape == (5, 3, 4)
    for i in range(5):
        for j in range(3):
            assert np.array_equal(w[i, j], SC.philox4(2 ** 40 + 3, int(lo[i, 0]), int(hi[0, j]))[0])
    u = SC.u01(np.array([0, 255, 256, 0xFFFFFFFF], dtype=np.uint64))
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)


# ---- the counter layout -----------------------------------------------------------------------------------------------------
def _counter_sets(offset, blocks, steps=(0, 1, 2, 7), rays=(0, 1, 5, 2 ** 20), lanes=(0, 1, 63)):
    """-> {(step, block): set of uniform counters}, {step: set of Gaussian counters}"""
    uni, gau = {}, {}
    for t in steps:
        for b in range(blocks):
            lo, hi_g, hi_u = SC.counters(offset, t, np.array(rays)[:, None], np.array(lanes)[None, :], b)
            uni[(t, b)] = {(int(l), int(hi_u[0])) for l in lo.reshape(-1)}
            gau[t] = {(int(l), int(hi_g[0])) for l in lo.reshape(-1)}
    return uni, gau


@pytest.mark.parametrize("offset", [0, 2 ** 32 + 5, 2 ** 64 - 6])
def test_counters_of_up_to_256_columns_are_distinct(offset):
    steps = (0, 1, 2, 3, 7, 8)
    uni, gau = _counter_sets(offset, SC.MAX_IN_KERNEL_S // 64, steps=steps)
    sets = list(uni.values()) + list(gau.values())
    assert all(len(s) == 4 * 3 for s in sets)                             # (ray, lane) -> low word is one to one
    assert len(set().union(*sets)) == sum(len(s) for s in sets)           # pairwise distinct, Gaussians included
    assert len(sets) == len(steps) * 4 + len(steps)


def test_a_fifth_column_block_is_the_next_steps_first():
    """S = 257: block 4 of step t reads the words of block 0 of step t + 1 -- why in-kernel draws stop at S = 256"""
    blocks = (257 + 63) // 64
    assert blocks == 5
    uni, _ = _counter_sets(0, blocks, steps=(0, 1, 2))
    assert uni[(0, 4)] == uni[(1, 0)] and uni[(1, 4)] == uni[(2, 0)]
    assert uni[(0, 3)].isdisjoint(uni[(1, 0)])
    w4 = SC.draw_words(9, 0, 0, 3, np.arange(64), 4)[1]
    w0 = SC.draw_words(9, 0, 1, 3, np.arange(64), 0)[1]
    assert np.array_equal(w4, w0)


def test_rng_index():
    assert SC.ray_indices(2, 3).tolist() == [0, 1, 2, 3, 4, 5]
    # rank 1 of 2 over the classes, the rays 32 .. 63 of 96: local class c is global class 1 + 2 c
    got = SC.ray_indices(2, 32, (1, 2, 96, 32)).reshape(2, 32)
    assert got[0].tolist() == list(range(96 + 32, 96 + 64)) and got[1].tolist() == list(range(3 * 96 + 32, 3 * 96 + 64))
    assert SC.ray_indices(1, 2, (0, 0, 7, 0)).tolist() == [0, 1]


# ---- Box-Muller ---------------------------------------------------------------------------------------------------------
def test_gauss_moments_and_tolerance():
    n = 2 ** 16
    words = SC.philox4(9, np.arange(n // 2, dtype=np.uint64), SC.GAUSS_HI_XOR)
    assert words.shape == (n // 2, 4)
    assert int((SC.u01(words[:, [0, 2]]) == 0).sum()) == 0                # no used word has u0 == 0
    g = SC.gauss(words, SC.EPS).reshape(-1)
    sd = float(np.float32(SC.EPS) / np.float32(3.0))
    assert g.shape == (n,) and g.dtype == np.float64
    mean, var = g.mean(), g.var()
    print(f"gauss: mean / se {mean / (sd / np.sqrt(n)):.2f}, (var - sd^2) / se {(var - sd * sd) / (sd * sd * np.sqrt(2.0 / n)):.2f}")
    assert abs(mean) <= 4 * sd / np.sqrt(n)
    assert abs(var - sd * sd) <= 4 * sd * sd * np.sqrt(2.0 / n)
    # float32, every operation rounded on its own, is the same draw to a few ulps of sd-sized values
    g32 = SC.gauss(words, SC.EPS, np.float32).reshape(-1)
    assert g32.dtype == np.float32 and float(np.abs(g32 - g).max()) < 1e-6 * sd * 10
    # the bar is the first-order move of 64 grid steps: moving u1 by 64 steps moves g by about that much
    tol = SC.gauss_tol(words, SC.EPS)
    assert tol.shape == (n // 2, 2) and bool(np.isfinite(tol).all()) and float(tol.min()) > 0
    moved = words.copy()
    moved[:, 1] = np.where(words[:, 1] < 0xF0000000, words[:, 1] + np.uint32(64 << 8), words[:, 1])
    dg = np.abs(SC.gauss(moved, SC.EPS)[:, 0] - SC.gauss(words, SC.EPS)[:, 0])
    assert bool((dg <= tol[:, 0] * 1.001 + 1e-12).all())
    print(f"gauss_tol: median {np.median(tol):.3e}, max {tol.max():.3e}, sd {sd:.3e}: a structural error is ~{sd / np.median(tol):.0f}x the bar")
    assert np.median(tol) < sd * 1e-3


# ---- the case builder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,R,n1,n2,world,min_bound", SC.RECORDED_CASES)
def test_case_builder_and_yardstick_floor(C, R, n1, n2, world, min_bound):
    seen = {}
    for rot in SC.recorded_rots(R):
        case = SC.build_case(C, R, n1, n2, min_bound, rot=rot)
        assert all(t.dtype == (torch.uint8 if k == "rgbs" else F32) for k, t in case._asdict().items())
        assert case.u.shape == (C, R, n1 + n2) and case.g.shape == (C, R, n2) and case.T.shape == (C, R, 4, 4)
        assert float(case.u.min()) >= 0.0 and float(case.u.max()) < 1.0
        # sim(3): A A^T = s^2 I with s in [0.5, 2], bottom row (0, 0, 0, 1)
        A = case.T[..., :3, :3].double()
        s2 = (A @ A.transpose(-1, -2)).diagonal(dim1=-2, dim2=-1).mean(-1)
        assert float(((A @ A.transpose(-1, -2)) - s2[..., None, None] * torch.eye(3, dtype=F64)).abs().max()) < 1e-5
        assert 0.25 <= float(s2.min()) and float(s2.max()) <= 4.0 and bool((torch.linalg.det(A) > 0).all())
        assert bool((case.T[..., 3, :] == torch.tensor([0.0, 0.0, 0.0, 1.0])).all())
        b = SC.branches(case, min_bound)
        for k, m in b.items():
            seen[k] = seen.get(k, 0) + int(m.sum())
        if R >= 5:
            wave = (torch.arange(C * R) % 4).view(C, R)
            for c in range(C):
                assert all(bool(m[c].any()) for m in b.values()), "every class holds every branch"
                assert bool((case.depth[c] == min_bound).any())
                assert bool((case.depth[c] == float(np.nextafter(np.float32(min_bound), np.float32(np.inf)))).any())
            assert all(bool((wave[m] != 0).any()) for m in b.values()), "no branch sits only in a block's first wave"
            assert {int(v) for v in case.rgbs[..., 3][~b["invalid"]]} == {0, 1, 2}
        # the yardstick: the float32 oracle inside check()'s rule against the float64 one, group by group, and the floor
        # 2^-22 max|want| no smaller than one ulp of the largest value (what one contracted multiply-add can differ by)
        want = SC.expected(case, n1, n2, SC.EPS, SC.STOP_EPS, min_bound, world, F64)
        ref = SC.expected(case, n1, n2, SC.EPS, SC.STOP_EPS, min_bound, world, F32)
        assert want["z"].dtype == F64 and ref["z"].dtype == F32 and want["z"].shape == (C, R, n1 + n2)
        assert torch.equal(want["labels"], ref["labels"]) and torch.equal(want["depth_mask"], ref["depth_mask"])
        assert torch.equal(want["depth_mask"].bool(), ~b["invalid"])
        SC.check_groups(ref, want, ref, case, n1, min_bound, f"yardstick {C}x{R} ({n1},{n2}) rot {rot}")
        for name, (mask, cols) in SC.groups(case, n1, min_bound).items():
            w = want["z"][mask][:, cols]
            if w.numel():
                scale = float(w.abs().max())
                e_r = float((ref["z"][mask][:, cols].double() - w).abs().max())
                ulp = float(np.spacing(np.float32(scale))) if scale > 0 else 0.0   # (one row of depth 0: z is exactly 0 throughout)
                print(f"  {name} z: e_r {e_r:.3e}, floor {M.FLOOR * scale:.3e}, ulp of the largest value {ulp:.3e}")
                assert M.FACTOR * e_r + M.FLOOR * scale >= ulp
    assert all(seen[k] > 0 for k in ("invalid", "this", "other")), seen


def test_tiny_depth_rows():
    case = SC.build_case(2, 37, 1, 9, 0.0, tiny=True)
    b = SC.branches(case, 0.0)
    for c in range(2):
        assert bool((case.depth[c][b["this"][c]] == SC.TINY_DEPTH).any())
