"""GPU: empty-space skipping of the scene view renderer.  The grid kernels (cnr_view_grid_cells, cnr_view_grid_dilate), the
active-sample pair (cnr_view_active_count / _emit) and cnr_view_scatter_active are compared exactly with tests/viewgrid_cpu.py;
a skipped render is compared bit for bit with its specification: the full render's samples, occupancy zero wherever the
restated lookup finds a clear cell, through cnr_view_composite.

The lookup is restated in float64 while the kernel works in float32, so a sample whose box coordinate lies within 1e-3 cell of
a cell face may fall either way: such samples are left out of the comparison of the active sets (for a uniform coordinate
about 6 * 1e-3 = 0.6 % of them; the share is printed and capped at 2 %), and the render's specification takes the kernel's
answer for them."""
import numpy as np
import pytest
import torch

import test_view_gpu as TV
import view_cpu as V
import view_scene as VS
import viewgrid_cpu as VG

pytestmark = pytest.mark.gpu
KMAX = V.KMAX


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


_t, _nan, _m7 = TV._t, TV._nan, TV._m7


# ---- grids ------------------------------------------------------------------------------------------------------------
def gpu_cells(cnr, dev, occ, G, sub, tau):
    words = _m7(dev, G ** 3 // 32 + 2)
    cnr._C.call("cnr_view_grid_cells", _t(occ, dev), G, sub, float(tau), words)
    torch.cuda.synchronize()
    assert (words[-2:] == -7).all()
    return words[:-2].cpu().numpy()


def gpu_dilate(cnr, dev, words, G, r):
    out = _m7(dev, G ** 3 // 32 + 2)
    cnr._C.call("cnr_view_grid_dilate", _t(words, dev), G, r, out)
    torch.cuda.synchronize()
    assert (out[-2:] == -7).all()
    return out[:-2].cpu().numpy()


@pytest.mark.parametrize("sub", [1, 2, 3])
@pytest.mark.parametrize("G", [4, 8, 12])
def test_cells(cnr, dev, G, sub):
    D, tau = G * sub + 1, np.float32(0.37)
    g = torch.Generator().manual_seed(100 * G + sub)
    lat = {}
    # a lattice point reaches tau with the probability that sets half of the cells: most set cells are set by a single
    # point, in their interior or on a face, an edge or a corner
    p = 1.0 - 0.5 ** (1.0 / (sub + 1) ** 3)
    rnd = (torch.rand(D, D, D, generator=g) * 0.3).numpy()
    rnd[torch.rand(D, D, D, generator=g).numpy() < p] = 0.5
    lat["random"] = rnd
    eq = (torch.rand(D, D, D, generator=g) * 0.3).numpy()
    eq[torch.rand(D, D, D, generator=g).numpy() < p] = tau                      # values exactly tau: they set the cell
    lat["equal"] = eq
    nan = np.zeros((D, D, D), np.float32)
    nan[D // 2, 1, D - 1] = np.nan                                              # a NaN sets the cells that own it
    lat["nan"] = nan
    lat["below"] = np.full((D, D, D), np.nextafter(tau, np.float32(0)), np.float32)
    lat["above"] = np.full((D, D, D), 0.9, np.float32)
    for name, occ in lat.items():
        occ = np.ascontiguousarray(occ, np.float32)
        want = VG.cells(occ, G, sub, tau)
        got = gpu_cells(cnr, dev, occ, G, sub, tau)
        assert np.array_equal(got, VG.pack(want)), (name, G, sub)
        share = want.mean()
        if name in ("random", "equal"):
            assert 0.2 < share < 0.8, (name, share)
        if name == "nan":
            assert 1 <= want.sum() <= 8
        if name in ("below", "above"):
            assert share == (name == "above")
    assert (eq == tau).any()


@pytest.mark.parametrize("r", [0, 1, 2])
def test_dilate(cnr, dev, r):
    G = 8
    singles = {"corner": (0, 0, 0), "far corner": (G - 1, G - 1, G - 1), "edge": (0, G - 1, 3), "centre": (4, 4, 4),
               "row end": (2, 5, G - 1),                # iz = G - 1: must not reach iz = 0 of the next row
               "linear 31": np.unravel_index(31, (G, G, G)), "linear 32": np.unravel_index(32, (G, G, G))}
    for name, c in singles.items():
        bits = np.zeros((G, G, G), bool)
        bits[tuple(c)] = True
        want = VG.dilate(bits, r)
        got = gpu_dilate(cnr, dev, VG.pack(bits), G, r)
        assert np.array_equal(got, VG.pack(want)), (name, r)
        if name == "centre":
            assert want.sum() == (2 * r + 1) ** 3
    G = 12
    bits = torch.rand(G, G, G, generator=torch.Generator().manual_seed(r)).numpy() < 0.005
    want = VG.dilate(bits, r)
    assert np.array_equal(gpu_dilate(cnr, dev, VG.pack(bits), G, r), VG.pack(want))
    assert 0 < want.mean() < 0.9


# ---- active samples ---------------------------------------------------------------------------------------------------
def _with_unmet_entity(to_box):
    """one more box, behind the camera of every scene here, in the middle of the entity list: no ray meets it"""
    far = V.box_affine((0.0, 0.0, -60.0), np.eye(3), (0.2, 0.2, 0.2))
    return np.concatenate([to_box[:2], far[None], to_box[2:]])


def _turned(to_box, seed=9):
    """The boxes the grids of the kernel tests live in: the scene's boxes turned by 0.2 rad, scaled by 0.9 .. 1.1 and shifted.
    Uniform samples between two opposite faces of the box they were cut against lie exactly on the faces of that box's cells
    whenever G (2 i + 1) / (2 S) is a whole number (S = 1 and S = 5 at G = 8), and so does every sample of an axis-parallel
    ray of scene B through a box centre; the float64 lookup says nothing about such a sample.  In the turned boxes the share
    of samples near a cell face is the 0.6 % of a uniform coordinate, and samples outside [-1,1]^3 show the clamp."""
    rng = np.random.default_rng(seed)
    out = []
    for A in to_box:
        M = rng.uniform(0.9, 1.1) * V.rot(rng.normal(size=3), 0.2)
        out.append(np.concatenate([M @ A[:, :3], (M @ A[:, 3] + rng.uniform(-0.05, 0.05, 3))[:, None]], 1))
    return np.stack(out)


def gpu_active(cnr, dev, seg, to_box, to_field, rows, S, words, ent_grid, G, slack=130):
    """count + emit into sentinel-filled buffers with `slack` entries of room behind the list -> dict"""
    _C, d, N = cnr._C, seg["dev"], seg["N"]
    E = to_box.shape[0]
    ws = torch.empty(max(int(_C.load().cnr_view_active_workspace_bytes(N, S, E)), 1), device=dev, dtype=torch.uint8)
    act_off, cnt = _m7(dev, E + 1, dtype=torch.int64), _m7(dev, 1, dtype=torch.int64)
    ent_off = _t(seg["entity_offset"], dev)
    _C.call("cnr_view_active_count", d["T"], d["dirs"], _t(to_box, dev, torch.float32), d["seg_pixel"], d["seg_entity"], d["seg_z"],
            ent_off, N, S, E, _t(words, dev), _t(ent_grid, dev, torch.int32), G, ws, act_off, cnt)
    off = act_off.tolist()
    M = off[E]
    assert M % 64 == 0 and 0 <= M <= N * S + 64 * E
    z = _nan(dev, N, S)
    idx, pts, brow = _m7(dev, M + slack, dtype=torch.int64), _nan(dev, M + slack, 3), _m7(dev, M // 64 + 2)
    _C.call("cnr_view_active_emit", d["T"], d["dirs"], _t(to_field, dev, torch.float32), d["seg_pixel"], d["seg_entity"], d["seg_z"],
            N, S, E, _t(rows, dev, torch.int32), ws, act_off, M, z, idx, pts, brow)
    torch.cuda.synchronize()
    assert (idx[M:] == -7).all() and torch.isnan(pts[M:]).all() and (brow[M // 64:] == -7).all()
    return dict(M=M, off=off, count=int(cnt.item()), z=z, idx=idx[:M].cpu().numpy(), pts=pts[:M], brow=brow[:M // 64].cpu().numpy())


def _check_list(a, active, seg, rows, S, pts_full):
    """the compact list `a` against the active set `active` (N,S) bool it claims to hold"""
    N, E = seg["N"], len(rows)
    ent = seg["seg_entity"][:N]
    per_entity = np.array([int(active[ent == e].sum()) for e in range(E)])
    padded = (per_entity + 63) // 64 * 64
    assert a["off"] == [0] + np.cumsum(padded).tolist()
    assert a["count"] == int(active.sum())
    flat = np.nonzero(active.reshape(-1))[0]
    want_idx = np.full(a["M"], -1, np.int64)
    want_row = np.zeros(a["M"] // 64, np.int64)
    k = 0
    for e in range(E):
        o = a["off"][e]
        want_idx[o:o + per_entity[e]] = flat[k:k + per_entity[e]]
        want_row[o // 64:a["off"][e + 1] // 64] = rows[e]
        k += per_entity[e]
    assert np.array_equal(a["idx"], want_idx)
    assert np.array_equal(a["brow"], want_row)
    live = torch.from_numpy(want_idx >= 0).to(pts_full.device)
    gathered = pts_full.reshape(-1, 3)[torch.from_numpy(np.maximum(want_idx, 0)).to(pts_full.device)]
    assert torch.equal(a["pts"][live], gathered[live])                          # bit for bit what cnr_view_points writes
    assert not a["pts"][~live].any()                                            # padding at the origin


@pytest.mark.parametrize("name", ["A", "B_axis_parallel"])
def test_active_samples(cnr, dev, name):
    T, dirs, to_box = TV.SCENES[name]()
    to_box = _with_unmet_entity(to_box)
    E, G = to_box.shape[0], 8
    n_alloc = int(V.segments(T.astype(np.float32), dirs, to_box.astype(np.float32), VS.ZMIN, VS.ZMAX, np.float64)["N"]) + 5
    seg = TV.gpu_segments(cnr, dev, T, dirs, to_box, n_alloc)
    N, d = seg["N"], seg["dev"]
    to_box = _turned(to_box)                    # from here on: the boxes of the grids
    off = seg["entity_offset"]
    assert off[2] == off[3] and off[3] < off[4], "entity 2 must have no segment"
    rng = np.random.default_rng(5)
    to_field = np.stack([V.box_affine(rng.normal(size=3), V.rot(rng.normal(size=3), rng.uniform(0, 3)), rng.uniform(0.5, 2.0) * np.ones(3))
                         for _ in range(E)]).astype(np.float32)
    rows = np.array([3, 0, 7, 1, 5, 2][:E])
    random_bits = torch.rand(E, G, G, G, generator=torch.Generator().manual_seed(11)).numpy() < 0.5
    odd = []
    for S in (1, 5, 64, 128):
        odd.append((N * S) % 64 != 0)
        z, pts = _nan(dev, N, S), _nan(dev, N, S, 3)
        cnr._C.call("cnr_view_points", d["T"], d["dirs"], _t(to_field, dev), d["seg_pixel"], d["seg_entity"], d["seg_z"], N, S, z, pts)
        every = np.ones((N, S), bool)
        # all set: grids full of ones, and the last entity without a grid at all
        ent_grid = np.arange(E)
        ent_grid[-1] = -1
        a = gpu_active(cnr, dev, seg, to_box, to_field, rows, S, VG.pack(np.ones((E, G, G, G), bool)), ent_grid, G)
        assert torch.equal(a["z"], z)
        assert np.array_equal(a["idx"][a["idx"] >= 0], np.arange(N * S))
        assert all((a["off"][e + 1] - a["off"][e]) % 64 == 0 for e in range(E)) and a["off"][2] == a["off"][3]
        _check_list(a, every, seg, rows, S, pts)
        # all clear
        a = gpu_active(cnr, dev, seg, to_box, to_field, rows, S, VG.pack(np.zeros((E, G, G, G), bool)), np.arange(E), G)
        assert a["M"] == 0 and a["count"] == 0 and a["off"] == [0] * (E + 1) and torch.equal(a["z"], z)
        # random: the grids of the entities permuted, to show that entity_grid is followed
        ent_grid = np.roll(np.arange(E), 1)
        a = gpu_active(cnr, dev, seg, to_box, to_field, rows, S, VG.pack(random_bits), ent_grid, G)
        want, near = VG.lookup(T, dirs, to_box, seg["seg_pixel"][:N], seg["seg_entity"][:N], seg["seg_z"][:N], S, random_bits, ent_grid)
        got = np.zeros(N * S, bool)
        got[a["idx"][a["idx"] >= 0]] = True
        got = got.reshape(N, S)
        print(f"{name} S={S}: {N * S} samples, {int(got.sum())} active, {near.mean():.3%} near a cell face left out")
        assert near.mean() <= 0.02
        assert np.array_equal(got[~near], want[~near])
        assert 0.1 < got.mean() < 0.9 and torch.equal(a["z"], z)
        _check_list(a, got, seg, rows, S, pts)
    assert any(odd), "one N * S must not be a multiple of 64"


def test_scatter(cnr, dev):
    NS, M = 300, 192
    g = torch.Generator().manual_seed(3)
    idx = torch.full((M,), -1, dtype=torch.int64)
    perm = torch.randperm(NS, generator=g)
    idx[:50], idx[64:64 + 64], idx[128:128 + 7] = perm[:50], perm[50:114], perm[114:121]      # three runs, two of them padded
    sig_c, col_c = torch.randn(M, generator=g), torch.rand(M, 3, generator=g)
    sigma, color = _nan(dev, NS + 3), _nan(dev, NS + 3, 3)
    cnr._C.call("cnr_view_scatter_active", sig_c.to(dev), col_c.to(dev), idx.to(dev), M, NS, sigma, color)
    torch.cuda.synchronize()
    assert torch.isnan(sigma[NS:]).all() and torch.isnan(color[NS:]).all()
    want_s, want_c = torch.full((NS,), float("-inf")), torch.zeros(NS, 3)
    live = idx >= 0
    want_s[idx[live]], want_c[idx[live]] = sig_c[live], col_c[live]
    assert torch.equal(sigma[:NS].cpu(), want_s) and torch.equal(color[:NS].cpu(), want_c)
    assert int(torch.isinf(sigma[:NS]).sum()) == NS - 121
    # an empty list: the fill alone
    sigma, color = _nan(dev, NS), _nan(dev, NS, 3)
    cnr._C.call("cnr_view_scatter_active", None, None, None, 0, NS, sigma, color)
    assert bool(torch.isinf(sigma).all()) and not color.any()


# ---- the skipped render -----------------------------------------------------------------------------------------------
SEED, S_E2E, G_E2E = 2, 16, 8
KEYS = ("rgb", "depth", "opacity", "var", "instance")
PATHS = {"fp32": ("fp32", 32), "fused": ("fused", 128)}


@pytest.fixture(scope="module", params=list(PATHS))
def e2e(cnr, dev, request):
    """the e2e scene of tests/test_view_gpu.py, with seeded random grids (about half of the cells set)"""
    precision, bg_hidden = PATHS[request.param]
    cfg = VS.small_camera(cnr.cfg.synthetic_config(device=str(dev), latent_dim=32))
    cls_dict, scene_bg = VS.make_scene(cnr, cfg, seed=SEED, bg_hidden=bg_hidden)
    scene_bg.trainer.eval_precision = precision
    r = cnr.view.SceneRenderer(cls_dict, scene_bg, cfg)
    bits = torch.rand(len(r.entities), G_E2E, G_E2E, G_E2E, generator=torch.Generator().manual_seed(7)) < 0.5
    r.set_grids(bits)
    return cfg, cls_dict, scene_bg, r, VS.camera_pose(), bits.numpy()


def _specified(cnr, dev, r, T, bits, ent_grid, skipped, what, **edit):
    """The specification of `skipped` = render(T, skip_empty=True, return_samples=True, **edit): the samples of the unskipped
    render, occupancy zero where the restated lookup says inactive, through cnr_view_composite."""
    with torch.no_grad():
        full = r.render(T, n_samples=S_E2E, return_samples=True, **edit)
    s = full["samples"]
    N, P = s["z"].shape[0], r.W * r.H
    want, near = VG.lookup(np.asarray(T, np.float64), r.dirs().cpu().numpy(), s["to_box"].cpu().numpy(), s["seg_pixel"].cpu().numpy(),
                           s["seg_entity"].cpu().numpy(), s["seg_z"].cpu().numpy(), S_E2E, bits, ent_grid)
    got = np.zeros(N * S_E2E, bool)
    got[skipped["samples"]["active_idx"].cpu().numpy()[skipped["samples"]["active_idx"].cpu().numpy() >= 0]] = True
    got = got.reshape(N, S_E2E)
    print(f"{what}: {N * S_E2E} samples, {int(got.sum())} active, {near.mean():.3%} near a cell face")
    assert near.mean() <= 0.02 and np.array_equal(got[~near], want[~near])
    assert 0.2 < want.mean() < 0.8
    active = np.where(near, got, want)
    sigma, color = VG.masked_composite_inputs(s["sigma"], s["color"], active)
    out = dict(rgb=_nan(dev, P, 3), depth=_nan(dev, P), opacity=_nan(dev, P), var=_nan(dev, P), mass=_nan(dev, P, KMAX), instance=_m7(dev, P))
    cnr._C.call("cnr_view_composite", sigma, color, s["z"], s["pix_segs"], s["seg_entity"], s["inst_ids"], P, S_E2E, 0.5,
                out["rgb"], out["depth"], out["opacity"], out["var"], out["mass"], out["instance"])
    # the fields at the active samples do not depend on how the samples are batched
    a = torch.from_numpy(active).to(dev)
    ds = (skipped["samples"]["sigma"][a] - s["sigma"][a]).abs().max().item()
    dc = (skipped["samples"]["color"][a] - s["color"][a]).abs().max().item()
    print(f"{what}: largest difference at active samples, skipped against unskipped evaluation: sigma {ds:.3e}, colour {dc:.3e}")
    assert torch.equal(skipped["samples"]["z"], s["z"])
    assert torch.equal(skipped["samples"]["sigma"], sigma) and torch.equal(skipped["samples"]["color"], color)
    return {k: v.reshape(r.W, r.H, *v.shape[1:]) for k, v in out.items()}, full


def test_skipped_render_is_the_masked_composite(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, bits = e2e
    with torch.no_grad():
        skipped = r.render(T, n_samples=S_E2E, skip_empty=True, return_samples=True)
    evaluated, all_samples = r.active_samples
    want, full = _specified(cnr, dev, r, T, bits, np.arange(len(r.entities)), skipped, "random grids")
    for k in KEYS:
        assert torch.equal(skipped[k], want[k]), k
    assert not torch.equal(skipped["rgb"], full["rgb"]), "the grids must skip something that shows"
    assert all_samples == full["samples"]["z"].numel() and 0.2 < evaluated / all_samples < 0.8


def test_all_set_and_all_clear_grids(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, bits = e2e
    with torch.no_grad():
        plain = r.render(T, n_samples=S_E2E)
        try:
            r.set_grids(torch.ones_like(torch.from_numpy(bits)))
            ones = r.render(T, n_samples=S_E2E, skip_empty=True)
            r.set_grids([None] * len(r.entities[:-1]) + [torch.ones(4, 4, 4, dtype=torch.bool)])      # entities without a grid
            none = r.render(T, n_samples=S_E2E, skip_empty=True)
            r.set_grids(torch.zeros_like(torch.from_numpy(bits)))
            zeros = r.render(T, n_samples=S_E2E, skip_empty=True)
            assert r.active_samples[0] == 0 and r.active_samples[1] > 0
        finally:
            r.set_grids(torch.from_numpy(bits))
    for k in KEYS:
        assert torch.equal(ones[k], plain[k]) and torch.equal(none[k], plain[k]), k
    for k in ("rgb", "depth", "opacity", "var"):
        assert not zeros[k].any(), k
    assert bool((zeros["instance"] == -1).all()) and bool((plain["instance"] >= 0).any())


def test_chunks_do_not_change_a_skipped_bit(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, bits = e2e
    with torch.no_grad():
        one = r.render(T, n_samples=S_E2E, skip_empty=True)
        small = r.render(T, n_samples=S_E2E, skip_empty=True, chunk=64)
    for k in KEYS:
        assert torch.equal(small[k], one[k]), k


def test_hidden_keeps_the_other_grids(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, bits = e2e
    assert [e.inst_id for e in r.entities] == [0, 1, 2, 3]
    without = cnr.view.SceneRenderer({10: cls_dict[10]}, scene_bg, cfg)
    without.set_grids(torch.from_numpy(bits[:3]))
    with torch.no_grad():
        hid = r.render(T, n_samples=S_E2E, hidden={3}, skip_empty=True)
        ref = without.render(T, n_samples=S_E2E, skip_empty=True)
        hid1 = r.render(T, n_samples=S_E2E, hidden={1}, skip_empty=True)      # the entities behind it keep THEIR grids
    for k in KEYS:
        assert torch.equal(hid[k], ref[k]), k
    with torch.no_grad():
        skipped = r.render(T, n_samples=S_E2E, hidden={1}, skip_empty=True, return_samples=True)
    want, _ = _specified(cnr, dev, r, T, bits, np.array([0, 2, 3]), skipped, "hidden 1", hidden={1})
    for k in KEYS:
        assert torch.equal(hid1[k], want[k]), k


def test_a_moved_entity_takes_its_grid_along(cnr, dev, e2e):
    cfg, cls_dict, scene_bg, r, T, bits = e2e
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = 1.2 * V.rot((0, 1, 0.3), 0.5), (0.3, 0.1, -0.2)
    with torch.no_grad():
        still = r.render(T, n_samples=S_E2E, skip_empty=True)
        moved = r.render(T, n_samples=S_E2E, transforms={2: E}, skip_empty=True, return_samples=True)
    want, _ = _specified(cnr, dev, r, T, bits, np.arange(len(r.entities)), moved, "moved", transforms={2: E})
    for k in KEYS:
        assert torch.equal(moved[k], want[k]), k
    assert not torch.equal(moved["rgb"], still["rgb"])


@pytest.mark.parametrize("d", [0, 1])
def test_build_grids(cnr, dev, e2e, d):
    """build_grids(resolution=8, sub=1) entity by entity: the threshold is the median of the entity's own cell maxima (random
    initial weights put every occupancy near 0.5), so about half of its cells are set before the dilation."""
    cfg, cls_dict, scene_bg, r, T, bits = e2e
    G, sub = 8, 1
    cats = [e.cat for e in r.entities]
    assert cats == [-1, 0, 0, 1], "the background, a two-object category and a world-frame category"
    try:
        for i in range(len(r.entities)):
            occ = r.lattice_occupancy(i, G * sub + 1).cpu().numpy()
            assert occ.shape == (9, 9, 9) and occ.dtype == np.float32
            top = torch.nn.functional.max_pool3d(torch.from_numpy(occ)[None, None], sub + 1, sub).reshape(-1)
            tau = float(top.median())
            want = VG.cells(occ, G, sub, tau)
            assert 0.2 <= want.mean() <= 0.8, (i, want.mean())
            r.build_grids(resolution=G, sub=sub, threshold=tau, dilate=d)
            got = r.grids()
            assert got.shape == (len(r.entities), G, G, G)
            assert np.array_equal(got[i].cpu().numpy(), VG.dilate(want, d)), (i, d)
            assert torch.equal(r._grids[1][i].cpu(), torch.from_numpy(VG.pack(VG.dilate(want, d))))
    finally:
        r.set_grids(torch.from_numpy(bits))
