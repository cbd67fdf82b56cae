"""The numpy restatement of the TSDF mesh contract (tests/tsdfmesh_cpu.py) judged on its own, and
utils.tsdf_unit_neighbourhood on CPU tensors against a dictionary."""
import numpy as np
import pytest
import torch

import mc_cpu as MC
import tsdf_cpu as TC
import tsdfmesh_cpu as TM

VOXEL = 0.01


def _table(keys):
    import cnr_amd
    return cnr_amd.utils.tsdf_unit_neighbourhood(torch.from_numpy(np.asarray(keys, np.int64))).numpy()


UNIT_SETS = {"no_plus_x": [(0, 0, 0), (0, 1, 0), (1, 1, 0)],
             "cube": [(x, y, z) for x in (3, 4) for y in (-2, -1) for z in (-1, 0)],
             "range_ends": [(-2 ** 20, -2 ** 20, 5), (2 ** 20 - 1, 0, 2 ** 20 - 1), (2 ** 20 - 1, 1, 2 ** 20 - 1)]}


@pytest.mark.parametrize("name", sorted(UNIT_SETS))
def test_neighbourhood_table_equals_the_dictionary(name):
    import cnr_amd
    keys, ijk = TM.block_set(UNIT_SETS[name])
    got, want = _table(keys), TM.neighbourhood_brute(keys)
    assert got.dtype == np.int32 and got.shape == (len(keys), 27) and np.array_equal(got, want)
    assert np.array_equal(got[:, 13], np.arange(len(keys)))
    t = torch.from_numpy(keys)
    nb = cnr_amd.utils.tsdf_unit_tables(t, torch.zeros(len(t), dtype=torch.int64))[3].numpy()
    assert np.array_equal(got[:, [22, 16, 14]], nb)
    if name == "no_plus_x":
        u0, uy, uxy = (int(np.flatnonzero((ijk == np.array(v)).all(1))[0]) for v in UNIT_SETS[name])
        assert got[u0, 22] == -1 and got[u0, 16] == uy and got[u0, 25] == uxy and got[uy, 22] == uxy and got[uxy, 1] == u0
    if name == "cube":
        assert (got >= 0).sum() == 8 * 8                      # every unit sees all eight
    if name == "range_ends":
        lo = int(np.flatnonzero(ijk[:, 0] == -2 ** 20)[0])
        assert (got[lo, :9] == -1).all() and (got[lo].reshape(3, 3, 3)[:, 0] == -1).all()       # x - 1 and y - 1 leave the range
        hi = np.flatnonzero(ijk[:, 0] == 2 ** 20 - 1)
        assert (got[hi, 18:] == -1).all() and (got[hi].reshape(2, 3, 3, 3)[..., 2] == -1).all()
        assert got[hi[0], 16] == hi[1] and got[hi[1], 10] == hi[0]                               # ... the y neighbours stay
    assert np.array_equal(_table(np.zeros(0, np.int64)), np.zeros((0, 27), np.int32))


# ---- the sphere -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    units, tsdf, weight, color = TM.sphere_blocks(VOXEL)
    out, parts = TM.mesh(units, tsdf, weight, color, VOXEL, parts=True)
    return (units, tsdf, weight, color), out, parts


def test_sphere_is_closed_outward_and_on_the_sphere(sphere):
    _, (v, c, n, f), parts = sphere
    assert len(v) > 1000 and len(f) > 2000
    uk, cnt, nv, dup = MC.edge_stats(f)
    assert (cnt == 2).all() and not dup                       # every edge in two faces, in opposite directions
    assert MC.euler(v, f) == 2 and len(np.unique(f)) == len(v) == nv
    assert MC.signed_volume(v, f) > 0
    assert abs(MC.signed_volume(v, f) / (4 / 3 * np.pi * 0.1 ** 3) - 1) < 0.02
    r = np.linalg.norm(v, axis=1)
    print("sphere: worst |r - R| / voxel", np.abs(r - 10 * VOXEL).max() / VOXEL, "worst cosine", (n * v / r[:, None]).sum(1).min())
    assert np.abs(r - 10 * VOXEL).max() < 0.05 * VOXEL
    assert ((n * v / r[:, None]).sum(1) >= 0.999).all()
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12
    assert c.min() >= 0 and c.max() <= 1 and c.std() > 0.05
    assert set(TM.cell_unit_counts(parts).tolist()) == {1, 2, 4}         # (the sphere does not pass through the origin's corner)


def test_sphere_equals_dense_marching_cubes(sphere):
    """the same blocks as one 32^3 volume: mc_cpu on -tsdf, level 0, descent"""
    (units, tsdf, weight, color), (v, c, n, f), parts = sphere
    ijk = TC.unpack(units).reshape(-1, 3)
    D = 32
    dense = np.zeros((D, D, D), np.float32)
    for u, (x, y, z) in enumerate(ijk + 1):
        dense[16 * x:16 * x + 16, 16 * y:16 * y + 16, 16 * z:16 * z + 16] = tsdf[u].reshape(16, 16, 16)
    dv, dn, df = MC.marching_cubes(-dense, level=0, ascent=False)
    assert len(dv) == len(v) and len(df) == len(f)
    # the dense side's vertex keys, in its order (point, axis), from its own inside test
    ins = (-dense) > 0
    keys = []
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, D - 1), slice(1, D)
        p = np.stack(np.nonzero(ins[tuple(lo)] != ins[tuple(hi)]), 1)
        keys.append(((p[:, 0] * D + p[:, 1]) * D + p[:, 2]) * 3 + a)
    dkey = np.sort(np.concatenate(keys))
    assert len(dkey) == len(dv)
    o = parts["owner"]
    g = (ijk[o[:, 0]] + 1) * 16 + o[:, 1:4]
    mkey = ((g[:, 0] * D + g[:, 1]) * D + g[:, 2]) * 3 + o[:, 4]
    assert np.array_equal(np.sort(mkey), dkey)
    rows = lambda k: k[np.lexsort(k.T[::-1])]
    assert np.array_equal(rows(mkey[f]), rows(dkey[df]))
    dense_pos = dv.astype(np.float64) * (D - 1) - 15.5        # voxel units about the origin
    order = np.argsort(mkey)
    assert np.abs(v[order] / VOXEL - dense_pos).max() < 1e-5
    assert ((n[order] * dn).sum(1) > 0.9999).all()            # both point to increasing tsdf


def _extract_keys(hood, tsdf, weight):
    """(unit, i, j, k, axis) of the points tsdf_cpu.extract emits, in its order"""
    f, obs = TM.tiles(hood, tsdf, weight)
    band = obs & (f < np.float32(0.98)) & (f >= np.float32(-0.98))
    cross = np.zeros((len(hood), 16, 16, 16, 3), bool)
    for a in range(3):
        e = [0, 0, 0]
        e[a] = 1
        cross[..., a] = TM._shift(band, (0, 0, 0)) & TM._shift(band, e) & (TM._shift(f, (0, 0, 0)) * TM._shift(f, e) < 0)
    return np.stack(np.nonzero(cross), 1)


@pytest.mark.parametrize("case", ["sphere", "random"])
def test_vertices_in_the_band_are_the_extracted_points(case):
    units, tsdf, weight, color = TM.sphere_blocks(VOXEL) if case == "sphere" else TM.random_blocks(UNIT_SETS["cube"], 5)
    hood = TM.neighbourhood_brute(units)
    (v, c, n, f), parts = TM.mesh(units, tsdf, weight, color, VOXEL, parts=True)
    pts, cols = TC.extract(units, hood[:, [22, 16, 14]], tsdf, weight, color, VOXEL)
    keys = _extract_keys(hood, tsdf, weight)
    assert len(keys) == len(pts) > 500
    at = {tuple(k): i for i, k in enumerate(keys.tolist())}
    pick = np.array([at.get(tuple(o), -1) for o in parts["owner"].tolist()])
    shared = pick >= 0
    assert shared.sum() > 500
    assert np.array_equal(v[shared], pts[pick[shared]]) and np.array_equal(c[shared], cols[pick[shared]])
    # the others have an end outside the band (the sphere: none), or their cells were all invalid
    tiles_f, _ = TM.tiles(hood, tsdf, weight)
    o = parts["owner"][~shared]
    far = o[:, 1:4].copy()
    far[np.arange(len(o)), o[:, 4]] += 1
    f0, f1 = tiles_f[o[:, 0], o[:, 1] + 1, o[:, 2] + 1, o[:, 3] + 1], tiles_f[o[:, 0], far[:, 0] + 1, far[:, 1] + 1, far[:, 2] + 1]
    lim = np.float32(0.98)
    assert ((f0 >= lim) | (f0 < -lim) | (f1 >= lim) | (f1 < -lim)).all()
    assert (len(o) == 0) == (case == "sphere")


# ---- holes ------------------------------------------------------------------------------------------------------------------
def _one_block(seed=3):
    units, tsdf, weight, color = TM.random_blocks([(2, -1, 0)], seed, unobserved=0.0)
    assert (weight != 0).all()
    return units, tsdf, weight, color


def test_an_unobserved_voxel_removes_exactly_its_eight_cells():
    units, tsdf, weight, color = _one_block()
    _, full = TM.mesh(units, tsdf, weight, color, VOXEL, parts=True)
    w = weight.copy().reshape(1, 16, 16, 16)
    w[0, 5, 9, 3] = 0
    out, holed = TM.mesh(units, tsdf, w.reshape(1, -1), color, VOXEL, parts=True)
    gone = full["valid"] & ~holed["valid"]
    assert not (holed["valid"] & ~full["valid"]).any()
    want = np.zeros_like(gone)
    want[0, 5:7, 9:11, 3:5] = True                            # cells (4..5, 8..9, 2..3): valid's index = cell + 1
    assert np.array_equal(gone, want)
    v, c, n, f = out
    assert len(np.unique(f)) == len(v)                        # no vertex unreferenced
    assert (holed["used"] <= full["used"]).all()


def test_a_crossed_edge_without_a_valid_cell_has_no_vertex():
    units, tsdf, weight, color = _one_block()
    t, w = tsdf.copy().reshape(16, 16, 16), weight.copy().reshape(16, 16, 16)
    t[6, 7, 8], t[7, 7, 8] = 0.5, -0.5                        # the x edge of voxel (6, 7, 8), crossed
    for dj in (-1, 1):                                        # a 2 x 2 column of voxel pairs around the edge: the pair diagonally
        for dk in (-1, 1):                                    # across from it in each of its four cells is unobserved, the edge's
            w[6:8, 7 + dj, 8 + dk] = 0                        # own two ends stay observed
    out, parts = TM.mesh(units, t.reshape(1, -1), w.reshape(1, -1), color, VOXEL, parts=True)
    assert w[6, 7, 8] != 0 and w[7, 7, 8] != 0
    assert not parts["valid"][0, 7, 7:9, 8:10].any()          # the four cells around the edge
    assert not parts["used"][0, 6, 7, 8, 0] and parts["vid"][0, 6, 7, 8, 0] == -1
    v, c, n, f = out
    assert len(np.unique(f)) == len(v)
    # with the column observed again the edge has its vertex
    _, again = TM.mesh(units, t.reshape(1, -1), weight, color, VOXEL, parts=True)
    assert again["used"][0, 6, 7, 8, 0]


# ---- missing units ------------------------------------------------------------------------------------------------------------
def test_cells_cross_only_into_units_that_exist():
    units, tsdf, weight, color = TM.random_blocks(UNIT_SETS["no_plus_x"], 11, unobserved=0.0)
    ijk = TC.unpack(units).reshape(-1, 3)
    u0, uy, uxy = (int(np.flatnonzero((ijk == np.array(v)).all(1))[0]) for v in UNIT_SETS["no_plus_x"])
    out, parts = TM.mesh(units, tsdf, weight, color, VOXEL, parts=True)
    own = parts["valid"][:, 1:, 1:, 1:]                       # the cells named by the units' own voxels
    assert not own[u0, 15].any()                              # across unit 0's +x face: nothing there
    assert own[u0, :15, 15, :15].all()                        # across its +y face: unit +y
    assert own[uy, 15, :15, :15].all()                        # from +y across its +x face: unit +x+y
    assert not own[u0, 15, 15].any() and not own[:, :, :, 15].any()       # the x-y edge needs +x too; no unit at +z
    assert not own[uxy, 15].any() and not own[uxy, :, 15].any() and not own[uy, :, 15].any()
    v, c, n, f = out
    assert len(np.unique(f)) == len(v)
    assert set(TM.cell_unit_counts(parts).tolist()) == {1, 2}
    # only the diagonal pair: no cell crosses any face
    sub = [u0, uxy]
    out2, parts2 = TM.mesh(units[sub], tsdf[sub], weight[sub], color[sub], VOXEL, parts=True)
    own2 = parts2["valid"][:, 1:, 1:, 1:]
    assert not own2[:, 15].any() and not own2[:, :, 15].any() and not own2[:, :, :, 15].any() and own2[:, :15, :15, :15].all()
    assert set(TM.cell_unit_counts(parts2).tolist()) == {1}
    # ... and each unit's part is the mesh of that unit alone
    alone = [TM.mesh(units[[u]], tsdf[[u]], weight[[u]], color[[u]], VOXEL) for u in sub]
    assert np.array_equal(out2[0], np.concatenate([a[0] for a in alone]))
    assert np.array_equal(out2[3], np.concatenate([alone[0][3], alone[1][3] + len(alone[0][0])]))
