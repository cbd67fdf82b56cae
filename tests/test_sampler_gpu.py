"""GPU: the depth-guided ray sampler (csrc/sample_common.h through cnr_sample_rays and cnr_step_prologue, csrc/sample.hip's slice
tables) against tests/sampler_cpu.py -- the reference's sample_3d_points in float64 per element, the sort against torch.sort
exactly, the in-kernel Philox draws against the published generator under the counter layout include/cnr_hip.h states, and the
Box-Muller offsets to within what 64 steps of the generator's own 2^-24 grid move them.

Measured on an MI355X: see DESIGN.md, "The sampler's checks"."""
import numpy as np
import pytest
import torch

import modular_cases as M
import sampler_cpu as SC

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EPS, STOP_EPS = SC.EPS, SC.STOP_EPS
N_OBJ = 4


@pytest.fixture(scope="module")
def cnr(dev):
    import cnr_amd
    return cnr_amd


def cpu(out):
    return {k: v.detach().cpu() for k, v in out.items() if torch.is_tensor(v)}


def sample_recorded(cnr, dev, case, n1, n2, min_bound, world):
    return cpu(cnr.ops.sample_rays(case.rgbs.to(dev), case.depth.to(dev), case.dirs.to(dev), case.T.to(dev), n1, n2, EPS, STOP_EPS,
                                   min_bound=min_bound, world_frame=bool(world), u=case.u.to(dev), g=case.g.to(dev),
                                   want_rays=True, out={}))


def assert_all_written(out, keys=("z", "pts", "origins", "dirs_o", "gt_rgb", "gt_depth")):
    for k in keys:
        assert bool(torch.isfinite(out[k]).all()), k


# ---- (a) recorded draws against float64, per element -----------------------------------------------------------------------
@pytest.mark.parametrize("C,R,n1,n2,world,min_bound", SC.RECORDED_CASES)
def test_recorded_draws_against_fp64(cnr, dev, C, R, n1, n2, world, min_bound):
    seen = {}
    for rot in SC.recorded_rots(R):
        case = SC.build_case(C, R, n1, n2, min_bound, rot=rot)
        got = sample_recorded(cnr, dev, case, n1, n2, min_bound, world)
        want = SC.expected(case, n1, n2, EPS, STOP_EPS, min_bound, world, F64)
        ref = SC.expected(case, n1, n2, EPS, STOP_EPS, min_bound, world, F32)
        assert_all_written(got)
        rows = SC.check_groups(got, want, ref, case, n1, min_bound, f"recorded {C}x{R} ({n1},{n2}) world {world} min {min_bound}")
        for k, v in rows.items():
            seen[k] = seen.get(k, 0) + v
        assert torch.equal(got["labels"], want["labels"])
        assert torch.equal(got["depth_mask"], want["depth_mask"])
        assert torch.equal(got["gt_rgb"], ref["gt_rgb"]) and torch.equal(got["gt_depth"], case.depth)
    assert all(seen[k] > 0 for k in ("invalid", "free", "other", "this")), f"an empty branch: {seen}"


# ---- (b) the sort, exactly -----------------------------------------------------------------------------------------------
SORT_N2 = [1, 2, 33, 63, 64, 65, 96, 127, 128]


def sort_rows(n2, eps):
    """g (K, n2) float32, one row per kind of input the network can get wrong"""
    gen = M.gen(4000 + n2)
    sd = eps / 3.0
    rnd = lambda: M.randn(gen, n2) * sd
    denorm = torch.tensor(2.0 ** -149, dtype=F32)
    rows = {
        "random": rnd(),
        "ascending": rnd().sort().values,
        "descending": rnd().sort(descending=True).values,
        "all equal": torch.full((n2,), 0.0123, dtype=F32),
        # three values drawn at random: runs of about n2 / 3 equal elements, one of them across lanes 63 / 64 of the 128 network
        "ties": torch.tensor([-0.02, 0.004, 0.03], dtype=F32)[torch.randint(0, 3, (n2,), generator=gen)],
        "zeros": torch.tensor([0.0, -0.0, 1e-3, -1e-3], dtype=F32)[torch.randint(0, 4, (n2,), generator=gen)],
        "denormals": torch.where(M.rand(gen, n2) < 0.5, torch.randint(-1000, 1000, (n2,), generator=gen).to(F32) * denorm, rnd()),
        # beyond +-eps on both sides (the clip flattens both ends), the rest inside
        "far": torch.where(M.rand(gen, n2) < 0.6, M.randn(gen, n2) * 100 * eps, rnd()),
        "random 2": rnd(),
    }
    return list(rows), torch.stack(list(rows.values()))


@pytest.mark.parametrize("n2", SORT_N2)
def test_sort_exactly(cnr, dev, n2):
    n1 = 3
    names, g = sort_rows(n2, EPS)
    K = g.shape[0]
    assert K % 4 != 0 and K > 4                                           # more than one block, the last one ragged
    case = SC.build_case(1, K, n1, n2, 0.0, seed=1)
    rgbs, depth = case.rgbs.clone(), 0.5 + 3.0 * M.rand(M.gen(n2), 1, K)
    rgbs[..., 3] = 1                                                      # every row: this object, a valid depth
    case = case._replace(rgbs=rgbs, depth=depth, g=g[None].contiguous())
    if n2 >= 33:
        assert bool((g[names.index("far")] > EPS).any()) and bool((g[names.index("far")] < -EPS).any())
        d = g[names.index("denormals")]
        assert bool(((d != 0) & (d.abs() < 2.0 ** -126)).any())
    got = sample_recorded(cnr, dev, case, n1, n2, 0.0, 0)
    eps32 = SC.f32(EPS)
    want = depth[0][:, None] + torch.clip(g.sort(dim=-1).values, -eps32, eps32)        # float32: one addition per element
    assert want.dtype == F32
    for i, name in enumerate(names):
        bad = int((got["z"][0, i, n1:] != want[i]).sum())
        print(f"sort n2 = {n2}, {name}: {bad} of {n2} columns differ")
    assert torch.equal(got["z"][0, :, n1:], want)
    assert bool((got["depth_mask"] == 1).all()) and bool((got["labels"] == 1).all())


# ---- pools: a case as one slice of a device-resident pool -------------------------------------------------------------------
def make_pool(case, slices, at, with_perm, seed=0):
    """The case's rows as slice `at` of a (C, slices R + 3) pool whose other slices come from other cases (depths scaled, so
    that every slice has another maximum); with_perm: behind a random permutation.  -> dict of CPU tensors"""
    C, R = case.depth.shape
    S, n2 = case.u.shape[-1], case.g.shape[-1]
    P = slices * R + 3
    gen = M.gen(31 + seed + 7 * R + slices)
    parts = {k: [] for k in ("rgbs", "depth", "dirs", "T")}
    for k in range(slices):
        src = case if k == at else SC.build_case(C, R, S - n2, n2, seed=100 + k)
        f = 1.0 if k == at else (1.5 + 0.25 * k)
        for name in parts:
            parts[name].append(getattr(src, name) * f if name == "depth" else getattr(src, name))
    tail = SC.build_case(C, R, S - n2, n2, seed=99)
    rows = torch.arange(3) % R
    content = {name: torch.cat(parts[name] + [getattr(tail, name)[:, rows]], 1) for name in parts}
    content["depth"][:, slices * R:] *= 4.0                               # rows of no slice: the largest depths of the pool
    if with_perm:
        perm = torch.stack([torch.randperm(P, generator=gen) for _ in range(C)])
        pool = {}
        for name, t in content.items():
            pool[name] = torch.empty_like(t)
            for c in range(C):
                pool[name][c, perm[c]] = t[c]
        pool["perm"] = perm.to(torch.int32)
    else:
        pool = dict(content)
        pool["perm"] = None
    pool["indices"] = torch.randint(0, N_OBJ, (C, P), generator=gen)
    at_rows = (pool["perm"][:, at * R:(at + 1) * R].long() if with_perm else torch.arange(at * R, (at + 1) * R).repeat(C, 1))
    for name in parts:                                                    # the slice IS the case
        flat = pool[name].reshape(C, P, -1)
        assert torch.equal(torch.gather(flat, 1, at_rows[..., None].expand(-1, -1, flat.shape[-1])), getattr(case, name).reshape(C, R, -1))
    pool["slice_rows"], pool["P"], pool["slice_max"] = at_rows, P, content["depth"][:, :slices * R].view(C, slices, R).amax(-1)
    return pool


def on(dev, t):
    return None if t is None else t.to(dev).contiguous()


def raw_sample(cnr, dev, pool, R, n1, n2, state, max_bound, slices, seed=9, offset=0, min_bound=0.0, u=None, g=None):
    """cnr_sample_rays on a pool with max_bound exactly as given (None: every wave takes the slice maximum itself)"""
    C, S = pool["depth"].shape[0], n1 + n2
    o = dict(z=torch.full((C, R, S), float("nan"), device=dev), pts=torch.full((C, R, S, 3), float("nan"), device=dev),
             gt_rgb=torch.empty(C, R, 3, device=dev), gt_depth=torch.empty(C, R, device=dev),
             depth_mask=torch.empty(C, R, device=dev, dtype=torch.uint8), labels=torch.empty(C, R, device=dev, dtype=torch.uint8),
             ray_row=torch.empty(C, R, device=dev, dtype=torch.int32))
    cnr._C.call("cnr_sample_rays", on(dev, pool["rgbs"]), on(dev, pool["depth"]), on(dev, pool["dirs"]), on(dev, pool["T"]),
                on(dev, u), on(dev, g), int(seed), int(offset), state, pool["P"], max_bound, 0, C, R, n1, n2, float(EPS),
                float(STOP_EPS), float(min_bound), o["z"], o["pts"], None, None, o["gt_rgb"], o["gt_depth"], o["depth_mask"],
                o["labels"], on(dev, pool["indices"]), N_OBJ, o["ray_row"], on(dev, pool["perm"]), int(slices))
    return cpu(o)


# ---- (c) the slice maximum: by the wave, by cnr_sample_maxdepth, from a cnr_slice_maxdepth table ---------------------------------
@pytest.mark.parametrize("R", [1, 63, 65, 257])
@pytest.mark.parametrize("with_perm", [False, True])
def test_slice_maximum_three_ways(cnr, dev, R, with_perm):
    C, n1, n2, slices, at = 2, 1, 9, 3, 2
    case = SC.build_case(C, R, n1, n2, 0.0, rot=1)                        # (R = 1: the one row is an invalid one, whose z reads the maximum)
    assert bool(SC.branches(case, 0.0)["invalid"].any())
    pool = make_pool(case, slices, at, with_perm)
    smax = pool["slice_max"]
    assert len({float(v) for v in smax[0]}) == slices, "every slice has another maximum"
    state = torch.tensor([at * R, 5, 0], dtype=torch.int64, device=dev)
    depth, perm = on(dev, pool["depth"]), on(dev, pool["perm"])
    mb = torch.full((C,), float("nan"), device=dev)
    cnr._C.call("cnr_sample_maxdepth", depth, mb, state, pool["P"], perm, C, R)
    table = torch.full((C, slices), float("nan"), device=dev)
    cnr._C.call("cnr_slice_maxdepth", depth, perm, pool["P"], C, R, slices, table)
    assert torch.equal(mb.cpu(), smax[:, at]) and torch.equal(table.cpu(), smax)
    assert torch.equal(smax[:, at], case.depth.amax(-1))
    runs = [raw_sample(cnr, dev, pool, R, n1, n2, state, None, 0), raw_sample(cnr, dev, pool, R, n1, n2, state, mb, 0),
            raw_sample(cnr, dev, pool, R, n1, n2, state, table, slices)]
    assert bool(torch.isfinite(runs[0]["z"]).all()) and bool(torch.isfinite(runs[0]["pts"]).all())
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), k
    # ... and the value is in use: the last column of an invalid row lies in the last of S bins below the maximum
    inv = SC.branches(case, 0.0)["invalid"]
    top = smax[:, at][:, None].expand(C, R)[inv]
    zl = runs[0]["z"][..., -1][inv]
    S = n1 + n2
    nz = top > 0
    assert bool((zl[nz] < top[nz]).all()) and bool((zl[nz] >= top[nz] * ((S - 1) / S) * (1 - 1e-6)).all())
    assert torch.equal(runs[0]["gt_depth"], case.depth)


# ---- (d), (e) Philox mode ---------------------------------------------------------------------------------------------------
PHILOX_N = [(1, 9), (1, 64), (8, 65), (16, 112), (64, 128), (128, 128)]      # (8, 65), (16, 112): part of the second register live
PHILOX_KEYS = [(step, offset, seed) for step in (0, 7) for offset in (0, 2 ** 32 + 5) for seed in (9, 2 ** 40 + 3)]
PHILOX_CR = (2, 37)
_philox_runs = {}


def philox_restated(case, n1, n2, seed, offset, step, rays):
    """-> the case with the restated uniforms as u, the restated draws (float64, unsorted) and their bars, (C, R, n2) each"""
    C, R = case.depth.shape
    u = torch.from_numpy(SC.ray_uniforms(seed, offset, step, rays, n1 + n2)).view(C, R, n1 + n2)
    words = SC.ray_gauss_words(seed, offset, step, rays)
    g64 = torch.from_numpy(SC.per_ray(SC.gauss(words, EPS), n2)).view(C, R, n2)
    tol = torch.from_numpy(SC.per_ray(SC.gauss_tol(words, EPS), n2)).view(C, R, n2)
    return case._replace(u=u.contiguous(), g=g64.to(F32).contiguous()), g64, tol


def philox_run(cnr, dev, n1, n2, step, offset, seed):
    key = (n1, n2, step, offset, seed)
    if key not in _philox_runs:
        C, R = PHILOX_CR
        case = SC.build_case(C, R, n1, n2, 0.0, seed=2, tiny=True)
        pool = make_pool(case, 3, 1, with_perm=step == 7)
        state = torch.tensor([R, step, 0], dtype=torch.int64, device=dev)
        mb = on(dev, pool["slice_max"][:, 1].contiguous())
        drawn = raw_sample(cnr, dev, pool, R, n1, n2, state, mb, 0, seed=seed, offset=offset)
        case_u, g64, tol = philox_restated(case, n1, n2, seed, offset, step, SC.ray_indices(C, R))
        given = raw_sample(cnr, dev, pool, R, n1, n2, state, mb, 0, seed=seed, offset=offset, u=case_u.u, g=case_u.g)
        _philox_runs[key] = dict(case=case_u, pool=pool, drawn=drawn, given=given, g64=g64, tol=tol)
    return _philox_runs[key]


def assert_uniform_columns(run, n1, n2, what, min_bound=0.0):
    """the invalid, free-space and other-object columns: bit-equal between in-kernel draws and the restated u given, then held to
    the float64 oracle on that u"""
    case, drawn, given = run["case"], run["drawn"], run["given"]
    assert bool(torch.isfinite(drawn["z"]).all()) and bool(torch.isfinite(drawn["pts"]).all())
    counts = {}
    for name, (mask, cols) in SC.groups(case, n1, min_bound).items():
        counts[name] = int(mask.sum())
        assert counts[name] > 0, f"{what}: no {name} rows"
        if name == "this":
            continue
        for k in ("z", "pts"):
            a, b = drawn[k][mask][:, cols], given[k][mask][:, cols]
            assert torch.equal(a, b), f"{what}: {name} {k}: {int((a != b).sum())} of {a.numel()} elements are of another word"
    for k in ("gt_rgb", "gt_depth", "depth_mask", "labels", "ray_row"):
        assert torch.equal(drawn[k], given[k]), k
    want = SC.expected(case, n1, n2, EPS, STOP_EPS, min_bound, 0, F64)
    ref = SC.expected(case, n1, n2, EPS, STOP_EPS, min_bound, 0, F32)
    SC.check_groups(drawn, want, ref, case, n1, min_bound, what, only=("invalid", "free", "other"), rays=False)
    assert torch.equal(drawn["labels"], want["labels"]) and torch.equal(drawn["depth_mask"], want["depth_mask"])
    assert torch.equal(drawn["gt_depth"], case.depth)


def assert_gaussian_columns(run, n1, n2, what, min_bound=0.0):
    """this-object rows: z - d against clip(sort(restated draws)) position by position, to the ray's largest bar plus one ulp of z;
    non-decreasing and inside [d - eps, d + eps] exactly.  -> worst error in steps of the 2^-24 grid (rows of depth 2^-20, where z
    rounds the offset by far less than a step), and the same over all rows (z's own rounding included)"""
    case, drawn, g64, tol = run["case"], run["drawn"], run["g64"], run["tol"]
    this = SC.branches(case, min_bound)["this"]
    assert int(this.sum()) > 0, f"{what}: no this-object rows"
    d32 = case.depth[this]
    z = drawn["z"][this][:, n1:]
    eps32 = SC.f32(EPS)
    assert bool((z[:, 1:] >= z[:, :-1]).all()), f"{what}: offsets not sorted"
    assert bool((z >= (d32 - eps32)[:, None]).all()) and bool((z <= (d32 + eps32)[:, None]).all()), f"{what}: offsets not clipped"
    draws, bars = g64[this], tol[this]
    order = draws.argsort(dim=-1)
    want = torch.clip(torch.gather(draws, 1, order), -eps32, eps32)
    err = (z.double() - d32.double()[:, None] - want).abs()
    ulp = torch.from_numpy(np.spacing(z.abs().amax(-1).numpy())).double()
    bar = bars.amax(-1) + ulp
    worst = err.amax(-1)
    # in grid steps: each position against the bar of the draw that sorts there (64 steps by definition)
    steps = 64.0 * err / torch.gather(bars, 1, order)
    tiny = d32 == SC.TINY_DEPTH
    s_tiny = float(steps[tiny].max()) if bool(tiny.any()) else float("nan")
    print(f"{what}: {int(this.sum())} this-object rows ({int(tiny.sum())} of depth 2^-20): worst Gaussian error "
          f"{s_tiny:.2f} grid steps on the 2^-20 rows, {float(steps.max()):.2f} over all rows (z's rounding included); "
          f"max err / bar {float((worst / bar).max()):.3f}")
    assert bool((worst <= bar).all()), f"{what}: err / bar {float((worst / bar).max()):.3f}"
    return s_tiny, float(steps.max())


@pytest.mark.parametrize("step,offset,seed", PHILOX_KEYS)
@pytest.mark.parametrize("n1,n2", PHILOX_N)
def test_philox_uniforms_are_the_restated_words(cnr, dev, n1, n2, step, offset, seed):
    run = philox_run(cnr, dev, n1, n2, step, offset, seed)
    assert_uniform_columns(run, n1, n2, f"philox ({n1},{n2}) step {step} offset {offset} seed {seed}")
    pool = run["pool"]
    C = pool["depth"].shape[0]
    rr = torch.gather(pool["indices"], 1, pool["slice_rows"]) + torch.arange(C)[:, None] * N_OBJ
    assert torch.equal(run["drawn"]["ray_row"].long(), rr)


@pytest.mark.parametrize("step,offset,seed", PHILOX_KEYS)
@pytest.mark.parametrize("n1,n2", PHILOX_N)
def test_philox_gaussian_offsets(cnr, dev, n1, n2, step, offset, seed):
    run = philox_run(cnr, dev, n1, n2, step, offset, seed)
    assert_gaussian_columns(run, n1, n2, f"gauss ({n1},{n2}) step {step} offset {offset} seed {seed}")


@pytest.mark.parametrize("aligned", [True, False])
def test_philox_through_step_prologue_with_sharded_indices(cnr, dev, aligned):
    """cnr_step_prologue (aligned poses: sample_ray_pool, its first uniform block drawn ahead; else sample_ray) as rank 1 of 2 over the
    classes holding rays 32 .. 63 of 96: the draws are those of the rays' GLOBAL indices"""
    _C, ops = cnr._C, cnr.ops
    C, R, n1, n2, L = 2, 32, 16, 112, 32
    rng, seed, step = (1, 2, 96, 32), 2 ** 40 + 3, 7
    case = SC.build_case(C, R, n1, n2, 0.0, seed=3, tiny=True)
    pool = make_pool(case, 3, 1, with_perm=True)
    state = torch.tensor([R, step, 0], dtype=torch.int64, device=dev)
    table = on(dev, pool["slice_max"])
    T = on(dev, pool["T"])
    if not aligned:
        T = torch.empty(T.numel() + 1, device=dev)[1:].view_as(T).copy_(T)
        assert T.data_ptr() % 16 == 4
    theta, lay = cnr.fused.init_params(C, L, N_OBJ, M.gen(5), dev)
    out = ops.step_prologue(theta, lay, L, N_OBJ, torch.empty(C, _C.pack_bytes(), device=dev, dtype=torch.uint8),
                            torch.empty(C * N_OBJ, 4, 32, device=dev), torch.empty(C * N_OBJ, 4, 32, device=dev),
                            torch.zeros(1000, device=dev), on(dev, pool["rgbs"]), on(dev, pool["depth"]), on(dev, pool["dirs"]), T,
                            n1, n2, EPS, STOP_EPS, 0.0, seed, state, R, {}, table, on(dev, pool["indices"]), on(dev, pool["perm"]),
                            max_bound_slices=3, rng=rng)
    rays = SC.ray_indices(C, R, rng)
    assert rays.tolist() != SC.ray_indices(C, R).tolist()
    case_u, g64, tol = philox_restated(case, n1, n2, seed, 0, step, rays)
    given = raw_sample(cnr, dev, pool, R, n1, n2, state, table, 3, seed=seed, u=case_u.u, g=case_u.g)
    run = dict(case=case_u, pool=pool, drawn=cpu(out), given=given, g64=g64, tol=tol)
    what = f"prologue rng {rng} aligned {aligned}"
    assert_uniform_columns(run, n1, n2, what)
    assert_gaussian_columns(run, n1, n2, what)
    rr = torch.gather(pool["indices"], 1, pool["slice_rows"]) + torch.arange(C)[:, None] * N_OBJ
    assert torch.equal(run["drawn"]["ray_row"].long(), rr)


# ---- (f) the slice tables against torch, exactly -----------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 63, 257, 2049])
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("with_perm", [False, True])
def test_slice_tables(cnr, dev, R, slices, with_perm):
    _C = cnr._C
    C, min_bound = 3, 0.25
    P = slices * R + 3
    gen = M.gen(R + 10 * slices + with_perm)
    depth = M.rand(gen, C, P) * 4.0
    depth[M.rand(gen, C, P) < 0.2] = 0.25                                 # exactly the bound: not a valid depth
    labels = torch.randint(0, 3, (C, P), generator=gen).to(torch.uint8)
    perm = torch.stack([torch.randperm(P, generator=gen) for _ in range(C)]) if with_perm else torch.arange(P).repeat(C, 1)
    last = perm[:, (slices - 1) * R:slices * R]
    depth[1, last[1]] = 0.0                                               # class 1: its last slice has no valid depth
    labels[2, last[2]] = 2                                                # class 2: its last slice is all label 2
    for c in range(C):
        depth[c, perm[c, slices * R:]] += 8.0                             # (rows of no slice must not be read: larger than any)
    rgbs = torch.randint(0, 256, (C, P, 4), generator=gen).to(torch.uint8)
    rgbs[..., 3] = labels
    d_dev, r_dev = depth.to(dev), rgbs.to(dev)
    p_dev = perm.to(torch.int32).to(dev) if with_perm else None
    rows = perm[:, :slices * R].reshape(C, slices, R)
    d_s = torch.gather(depth, 1, rows.reshape(C, -1)).view(C, slices, R)
    l_s = torch.gather(labels, 1, rows.reshape(C, -1)).view(C, slices, R)
    table = torch.full((C, slices), float("nan"), device=dev)
    _C.call("cnr_slice_maxdepth", d_dev, p_dev, P, C, R, slices, table)
    assert torch.equal(table.cpu(), d_s.amax(-1))
    for s in range(slices):
        mb = torch.full((C,), float("nan"), device=dev)
        state = torch.tensor([s * R, 0, 0], dtype=torch.int64, device=dev)
        _C.call("cnr_sample_maxdepth", d_dev, mb, state, P, p_dev, C, R)
        assert torch.equal(mb.cpu(), d_s[:, s].amax(-1)), s
    counts = torch.full((slices, C + 1, 4), float("nan"), device=dev)
    _C.call("cnr_slice_maskcounts", r_dev, d_dev, p_dev, P, C, R, slices, float(min_bound), counts)
    mo, ms, md = l_s != 0, l_s != 2, d_s > min_bound
    per = torch.stack([(md & mo).sum(-1), mo.sum(-1), ms.sum(-1), torch.zeros(C, slices, dtype=torch.int64)], -1).permute(1, 0, 2).to(F32)
    empty = (per == 0).any(1).to(F32)
    empty[:, 3] = 0.0
    want = torch.cat([per, empty[:, None]], 1)
    assert torch.equal(counts.cpu(), want)
    if R > 1:
        assert want[slices - 1, C].tolist() == [1.0, 0.0, 1.0, 0.0]           # no valid depth in class 1, no label != 2 in class 2
        assert slices == 1 or want[0, C].tolist() == [0.0] * 4


# ---- (g) the bin edges are torch.linspace's, exactly ---------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(1, 9), (3, 33), (8, 56), (16, 112), (63, 65), (64, 128), (130, 126), (127, 127)])
def test_bin_edges_are_torch_linspace(cnr, dev, n1, n2):
    """u = 0 and ranges that are powers of two make every z a bin edge times a power of two, with nothing to round: row 0 (invalid,
    slice maximum 4) is 4 linspace(0, 1, S + 1), row 1 (depth 2.25, eps 0.25) 2 linspace(0, 1, n1 + 1) below n1, row 2 (depth = eps
    = 0.25, stop_eps 0.75, state 0) linspace(0, 1, n2 + 1) from n1 on."""
    S, eps, stop = n1 + n2, 0.25, 0.75
    case = SC.build_case(1, 4, n1, n2, 0.0)
    rgbs = case.rgbs.clone()
    rgbs[0, :, 3] = torch.tensor([0, 1, 0, 2], dtype=torch.uint8)
    depth = torch.tensor([[0.0, 2.25, 0.25, 4.0]])
    case = case._replace(rgbs=rgbs, depth=depth, u=torch.zeros(1, 4, S))
    got = cpu(cnr.ops.sample_rays(case.rgbs.to(dev), case.depth.to(dev), case.dirs.to(dev), case.T.to(dev), n1, n2, eps, stop,
                                  u=case.u.to(dev), g=case.g.to(dev), out={}))
    z = got["z"][0]
    assert torch.equal(z[0], 4.0 * torch.linspace(0, 1, S + 1, dtype=F32)[:-1])
    assert torch.equal(z[1, :n1], 2.0 * torch.linspace(0, 1, n1 + 1, dtype=F32)[:-1])
    assert torch.equal(z[2, n1:], torch.linspace(0, 1, n2 + 1, dtype=F32)[:-1])


# ---- the limit of in-kernel draws -----------------------------------------------------------------------------------------------
def test_in_kernel_draws_stop_at_256_columns(cnr, dev):
    """S = 258: accepted with recorded draws (test_recorded_draws_against_fp64 holds its values), refused with in-kernel draws --
    a fifth uniform column block would read the next step's first (tests/test_sampler_host.py) -- and nothing is launched"""
    C, R, n1, n2 = 1, 5, 130, 128
    case = SC.build_case(C, R, n1, n2)
    args = [t.to(dev) for t in (case.rgbs, case.depth, case.dirs, case.T)]
    out = {"z": torch.full((C, R, n1 + n2), -7.0, device=dev), "pts": torch.full((C, R, n1 + n2, 3), -7.0, device=dev)}
    with pytest.raises(cnr._C.CnrError, match="code -2"):               # CNR_E_SHAPE
        cnr.ops.sample_rays(*args, n1, n2, EPS, STOP_EPS, seed=9, out=out, max_bound=case.depth.amax(-1).to(dev))
    torch.cuda.synchronize()
    assert bool((out["z"] == -7.0).all()) and bool((out["pts"] == -7.0).all())
    # S = 256 is taken
    got = cnr.ops.sample_rays(*args, 128, 128, EPS, STOP_EPS, seed=9, out={})
    assert bool(torch.isfinite(got["z"]).all())
    # the step prologue has the same limit
    _C = cnr._C
    theta, lay = cnr.fused.init_params(C, 32, N_OBJ, M.gen(5), dev)
    state = torch.tensor([0, 0, 0], dtype=torch.int64, device=dev)
    pro = {"z": torch.full((C, R, n1 + n2), -7.0, device=dev)}
    with pytest.raises(_C.CnrError, match="code -2"):
        cnr.ops.step_prologue(theta, lay, 32, N_OBJ, torch.empty(C, _C.pack_bytes(), device=dev, dtype=torch.uint8),
                              torch.empty(C * N_OBJ, 4, 32, device=dev), torch.empty(C * N_OBJ, 4, 32, device=dev),
                              torch.zeros(1000, device=dev), *args, n1, n2, EPS, STOP_EPS, 0.0, 9, state, R, pro,
                              case.depth.amax(-1).to(dev), torch.zeros(C, R, dtype=torch.int64, device=dev), None)
    torch.cuda.synchronize()
    assert bool((pro["z"] == -7.0).all())
    # ... and the background step's tail sampler, which always draws in the kernel (refused ahead of everything the tail would read)
    z, pts = torch.full((1, R, n1 + n2), -7.0, device=dev), torch.full((1, R, n1 + n2, 3), -7.0, device=dev)
    with pytest.raises(_C.CnrError, match="code -2"):
        _C.call_struct("cnr_bg_tail_sample", theta=None, grad=None, exp_avg=None, exp_avg_sq=None, partials=None, chunks=0, records=None,
                       nrec=0, grad_scale=1.0, lr=0.0, beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0, packed=None,
                       rl_workspace=None, rl_R=0, losses=None, flags=None, rgbs=args[0], depth=args[1], dirs_c=args[2], T=args[3],
                       seed=9, offset=0, d_state=state, pool_rows=R, max_bound=case.depth.amax(-1).to(dev), max_bound_slices=0,
                       world_frame=1, R=R, n1=n1, n2=n2, eps=EPS, stop_eps=STOP_EPS, min_bound=0.0, perm=None, z=z, pts=pts, origins=None,
                       dirs_o=None, gt_rgb=torch.empty(1, R, 3, device=dev), gt_depth=None,
                       depth_mask=torch.empty(1, R, device=dev, dtype=torch.uint8), labels=torch.empty(1, R, device=dev, dtype=torch.uint8))
    torch.cuda.synchronize()
    assert bool((z == -7.0).all()) and bool((pts == -7.0).all())
