"""TEST INFRASTRUCTURE: numpy restatement of the TSDF mesh contract of DESIGN.md §3.10 (csrc/tsdf_mesh.hip,
utils.TSDFVolume.extract_triangle_mesh_raw), written from the contract: every fp64 product and sum is one numpy operation, so the
kernels must reproduce every bit.  Per unit a 19^3 tile of the voxels -1 .. 17 per axis, gathered through the 27-table."""
import numpy as np

import mc_cpu as MC
import tsdf_cpu as TC

UNIT = TC.UNIT
TILE = UNIT + 3
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]          # column (dx+1) 9 + (dy+1) 3 + dz+1


def neighbourhood_brute(units):
    """(U,) keys -> (U,27) int32 by a dictionary: the unit at each offset, -1 where there is none or its index leaves
    [-2^20, 2^20)"""
    at = {int(k): i for i, k in enumerate(units)}
    hood = np.full((len(units), 27), -1, np.int32)
    for i, ijk in enumerate(TC.unpack(np.asarray(units, np.int64)).reshape(-1, 3)):
        for col, d in enumerate(OFFSETS):
            n = ijk + np.array(d)
            if (n >= -TC.BIAS).all() and (n < TC.BIAS).all():
                hood[i, col] = at.get(int(TC.pack(*n)), -1)
    return hood


def tiles(hood, tsdf, weight):
    """-> (f (U,19,19,19) f32, observed (U,19,19,19) bool): tile index t = voxel t - 1 of the unit's frame"""
    U = len(hood)
    f0, w0 = tsdf.reshape(U, UNIT, UNIT, UNIT), weight.reshape(U, UNIT, UNIT, UNIT)
    f, obs = np.zeros((U, TILE, TILE, TILE), np.float32), np.zeros((U, TILE, TILE, TILE), bool)
    dst = {-1: slice(0, 1), 0: slice(1, UNIT + 1), 1: slice(UNIT + 1, UNIT + 3)}
    src = {-1: slice(UNIT - 1, UNIT), 0: slice(0, UNIT), 1: slice(0, 2)}
    for col, (dx, dy, dz) in enumerate(OFFSETS):
        has = hood[:, col] >= 0
        n = hood[has, col]
        f[has, dst[dx], dst[dy], dst[dz]] = f0[n][:, src[dx], src[dy], src[dz]]
        obs[has, dst[dx], dst[dy], dst[dz]] = w0[n][:, src[dx], src[dy], src[dz]] != 0
    return f, obs


def _shift(a, d):
    """a[:, i + d0, j + d1, k + d2] for the 16^3 own voxels (tile index 1 .. 16)"""
    return a[:, 1 + d[0]:1 + d[0] + UNIT, 1 + d[1]:1 + d[1] + UNIT, 1 + d[2]:1 + d[2] + UNIT]


def classify(hood, tsdf, weight):
    """-> dict: f, obs (tiles), valid (U,17,17,17) of the cells with min corner -1 .. 15, case (U,16,16,16) of the own cells (0
    where invalid), used (U,16,16,16,3) owned edges that a valid cell uses"""
    f, obs = tiles(hood, tsdf, weight)
    U = len(hood)
    valid = np.ones((U, UNIT + 1, UNIT + 1, UNIT + 1), bool)
    for c in range(8):
        a, b, d = (c >> 2) & 1, (c >> 1) & 1, c & 1
        valid &= obs[:, a:a + UNIT + 1, b:b + UNIT + 1, d:d + UNIT + 1]
    with np.errstate(invalid="ignore"):
        neg = (f < 0) & obs
    case = np.zeros((U, UNIT, UNIT, UNIT), np.int64)
    for c in range(8):
        case |= _shift(neg, ((c >> 2) & 1, (c >> 1) & 1, c & 1)).astype(np.int64) << c
    case[~valid[:, 1:, 1:, 1:]] = 0
    used = np.zeros((U, UNIT, UNIT, UNIT, 3), bool)
    for a in range(3):
        e = [0, 0, 0]
        e[a] = 1
        crossed = _shift(obs, (0, 0, 0)) & _shift(obs, e) & (_shift(neg, (0, 0, 0)) != _shift(neg, e))
        # the four cells around the edge: min corners back by 0 or 1 along the two other axes (valid's index = voxel + 1)
        b, c = [x for x in range(3) if x != a]
        around = np.zeros((U, UNIT, UNIT, UNIT), bool)
        for db in (0, 1):
            for dc in (0, 1):
                lo = [1, 1, 1]
                lo[b] -= db
                lo[c] -= dc
                around |= valid[:, lo[0]:lo[0] + UNIT, lo[1]:lo[1] + UNIT, lo[2]:lo[2] + UNIT]
        used[..., a] = crossed & around
    return dict(f=f, obs=obs, valid=valid, case=case, used=used)


def _gradient(f, obs, ui, t, axis):
    """the tsdf gradient's component along `axis` at the tile voxels t (n,3) of the units ui, fp64"""
    lo, hi = t.copy(), t.copy()
    lo[:, axis] -= 1
    hi[:, axis] += 1
    fm, fp, f0 = (f[ui, x[:, 0], x[:, 1], x[:, 2]].astype(np.float64) for x in (lo, hi, t))
    om, op = obs[ui, lo[:, 0], lo[:, 1], lo[:, 2]], obs[ui, hi[:, 0], hi[:, 1], hi[:, 2]]
    return np.where(om & op, (fp - fm) * 0.5, np.where(op, fp - f0, np.where(om, f0 - fm, 0.0)))


def mesh(units, tsdf, weight, color, voxel, hood=None, parts=False):
    """-> (verts (V,3) f64, colors (V,3) f64, normals (V,3) f64, faces (F,3) i32), or None when V or F is 0.
    parts=True: -> (that or None, dict of the classification with `vid` (U,16,16,16,3) vertex ids, -1 where none, and `owner`
    (V,5): unit, i, j, k, axis of every vertex)"""
    units = np.asarray(units, np.int64)
    U = len(units)
    hood = neighbourhood_brute(units) if hood is None else hood
    c = classify(hood, tsdf, weight)
    f, obs, used, case = c["f"], c["obs"], c["used"], c["case"]
    ui, i, j, k, a = np.nonzero(used)                         # C order: unit, voxel, axis
    V = len(ui)
    vid = np.full(used.shape, -1, np.int64)
    vid[ui, i, j, k, a] = np.arange(V)
    c.update(vid=vid, owner=np.stack([ui, i, j, k, a], 1))
    # faces: unit, cell, table order
    cu, ci, cj, ck = np.nonzero(MC.NTRI[case])
    cs = case[cu, ci, cj, ck]
    nt = MC.NTRI[cs]
    rep = np.repeat(np.arange(len(cu)), nt)
    tri = np.arange(len(rep)) - np.repeat(np.cumsum(nt) - nt, nt)
    faces = np.empty((len(rep), 3), np.int64)
    for col in range(3):
        lo = MC.EDGE_LO[MC.TRI[cs[rep], 3 * tri + col]]
        corner, axis = lo >> 2, lo & 3
        o = np.stack([ci[rep] + ((corner >> 2) & 1), cj[rep] + ((corner >> 1) & 1), ck[rep] + (corner & 1)], 1)
        over = o >> 4                                        # 1 where the owner is voxel 0 of the next unit
        nu = hood[cu[rep], 13 + 9 * over[:, 0] + 3 * over[:, 1] + over[:, 2]]
        assert (nu >= 0).all()
        faces[:, col] = vid[nu, o[:, 0] & 15, o[:, 1] & 15, o[:, 2] & 15, axis]
    assert (faces >= 0).all()
    faces = faces[:, [0, 2, 1]]                               # the table's normal points to the negative corners
    c["cells"] = np.stack([cu, ci, cj, ck], 1)
    if V == 0 or len(faces) == 0:
        return (None, c) if parts else None
    # vertices
    rows = np.arange(V)
    ijk = np.stack([i, j, k], 1)
    t0 = ijk + 1
    t1 = t0.copy()
    t1[rows, a] += 1
    r0 = np.abs(f[ui, t0[:, 0], t0[:, 1], t0[:, 2]].astype(np.float64))
    r1 = np.abs(f[ui, t1[:, 0], t1[:, 1], t1[:, 2]].astype(np.float64))
    p = TC.unpack(units[ui]).astype(np.float64) * (16.0 * voxel) + (ijk + 0.5) * voxel
    p0 = p[rows, a]
    p1 = p0 + voxel
    p[rows, a] = (p0 * r1 + p1 * r0) / (r0 + r1)
    far = ijk.copy()
    far[rows, a] += 1
    over = far >> 4
    nu = hood[ui, 13 + 9 * over[:, 0] + 3 * over[:, 1] + over[:, 2]]
    col4 = np.asarray(color).reshape(U, UNIT, UNIT, UNIT, 3)
    c0 = col4[ui, i, j, k].astype(np.float64)
    c1 = col4[nu, far[:, 0] & 15, far[:, 1] & 15, far[:, 2] & 15].astype(np.float64)
    cols = (c0 * r1[:, None] + c1 * r0[:, None]) / (r0 + r1)[:, None] / 255.0
    n = np.stack([(_gradient(f, obs, ui, t0, b) * r1 + _gradient(f, obs, ui, t1, b) * r0) / (r0 + r1) for b in range(3)], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        has = ln > 0
        n = np.where(has[:, None], n / np.where(has, ln, 1.0)[:, None], 0.0)
    out = (p, cols, n, faces.astype(np.int32))
    return (out, c) if parts else out


def cell_unit_counts(c):
    """number of distinct units among the 8 corners of every cell of c['cells'] (1, 2, 4 or 8)"""
    cells = c["cells"]
    over = (cells[:, 1:] == UNIT - 1).sum(1)
    return 1 << over


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def block_set(ijk_list):
    """unit indices -> ascending keys (U,) and their (U,3) indices"""
    keys = np.sort(TC.pack(*np.asarray(ijk_list, np.int64).T))
    return keys, TC.unpack(keys).reshape(-1, 3)


def sphere_blocks(voxel=0.01, radius=10.0, band=4.0):
    """2 x 2 x 2 units around the origin, every weight 1, tsdf = clip((|p| - radius voxel) / (band voxel), -1, 1); colours from
    the position"""
    units, ijk = block_set([(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)])
    centres = np.stack([TC.voxel_centres(u, voxel) for u in ijk])                      # (8,4096,3)
    tsdf = np.clip((np.linalg.norm(centres, axis=-1) - radius * voxel) / (band * voxel), -1, 1).astype(np.float32)
    weight = np.ones_like(tsdf)
    color = np.clip(128 + centres / voxel * 7, 0, 255).astype(np.float32)
    return units, tsdf, weight, color


def random_blocks(ijk_list, seed, unobserved=0.1):
    """tsdf uniform in (-1, 1), `unobserved` of the weights zero, random colours"""
    units, _ = block_set(ijk_list)
    rng = np.random.default_rng(seed)
    U = len(units)
    tsdf = rng.uniform(-1, 1, (U, UNIT ** 3)).astype(np.float32)
    weight = (rng.uniform(0, 1, (U, UNIT ** 3)) >= unobserved).astype(np.float32) * rng.integers(1, 4, (U, UNIT ** 3)).astype(np.float32)
    color = rng.integers(0, 256, (U, UNIT ** 3, 3)).astype(np.float32)
    return units, tsdf, weight, color
