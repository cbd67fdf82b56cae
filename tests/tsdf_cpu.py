"""TEST INFRASTRUCTURE: numpy restatement of the TSDF contract of DESIGN.md §3.10 (csrc/tsdf.hip, utils.TSDFVolume): the depth
image, the touch list and its tables, the integration, the extraction and the radius count.  Written from the contract: every
fp64 product and sum is one numpy operation, the running means are float32 arrays, so the kernels must reproduce every bit.
Frames are in the loaders' (W,H) layout."""
import numpy as np

UNIT = 16
STRIDE = 4
AXIS_BITS = 21
BIAS = 1 << (AXIS_BITS - 1)
MASK = (1 << AXIS_BITS) - 1


def depth_image(depth, obj_mask, inst_id, depth_scale=0.001, max_depth=6.0):
    """metric (W,H) depth -> what the volume sees: masked, uint16(trunc(depth / depth_scale)), / 1000 in fp32, 0 beyond max_depth"""
    d = np.where(np.asarray(obj_mask) == inst_id, np.asarray(depth, np.float32), np.float32(0))
    with np.errstate(all="ignore"):
        t = np.trunc(d.astype(np.float64) / depth_scale)
    u16 = np.where((t >= 0) & (t < 9.2e18), t, 0).astype(np.uint64) & np.uint64(0xFFFF)      # astype(uint16) wraps; NaN -> 0
    out = u16.astype(np.float32) / np.float32(1000.0)
    out[out.astype(np.float64) > max_depth] = 0
    return out


def pack(ix, iy, iz):
    return ((np.asarray(ix, np.int64) + BIAS) << (2 * AXIS_BITS)) | ((np.asarray(iy, np.int64) + BIAS) << AXIS_BITS) | \
           (np.asarray(iz, np.int64) + BIAS)


def unpack(key):
    key = np.asarray(key, np.int64)
    return np.stack([((key >> (2 * AXIS_BITS)) & MASK) - BIAS, ((key >> AXIS_BITS) & MASK) - BIAS, (key & MASK) - BIAS], -1)


def touch(depth, K, T_WC, voxel, trunc):
    """one frame -> keys (samples, 8) int64, samples x major, -1 in unused slots"""
    fx, fy, cx, cy = K
    W, H = depth.shape
    UL = 16.0 * voxel
    if not 0 < 2.0 * trunc <= UL:
        raise ValueError("trunc <= 8 voxel: [p - trunc, p + trunc] may span two units per axis, not three")
    xs, ys = np.meshgrid(np.arange(0, W, STRIDE), np.arange(0, H, STRIDE), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    d = depth[xs, ys].astype(np.float64)
    px, py = (xs - cx) * d / fx, (ys - cy) * d / fy
    T = np.asarray(T_WC, np.float64)
    keys = np.full((len(xs), 8), -1, np.int64)
    with np.errstate(all="ignore"):
        p = [((T[a, 0] * px + T[a, 1] * py) + T[a, 2] * d) + T[a, 3] for a in range(3)]
        lo = [np.floor((p[a] - trunc) / UL) for a in range(3)]
        hi = [np.floor((p[a] + trunc) / UL) for a in range(3)]
    seen = d > 0
    ok = np.ones(len(xs), bool)
    for a in range(3):
        ok &= (lo[a] >= -BIAS) & (hi[a] < BIAS)
        ok &= hi[a] - lo[a] <= 1
    if (seen & ~ok).any():
        raise OverflowError("a unit index outside [-2^20, 2^20), or three units on an axis")
    for k in range(8):
        u = [lo[0] + ((k >> 2) & 1), lo[1] + ((k >> 1) & 1), lo[2] + (k & 1)]
        use = seen & (u[0] <= hi[0]) & (u[1] <= hi[1]) & (u[2] <= hi[2])
        keys[use, k] = pack(u[0][use].astype(np.int64), u[1][use].astype(np.int64), u[2][use].astype(np.int64))
    return keys


def unit_tables(keys_per_frame):
    """[keys of frame 0, of frame 1, ...] -> (units (U,) ascending, frame_ofs (U+1,), frame_idx (M,) int32, neighbours (U,3) int32)"""
    frames_of = {}
    for f, keys in enumerate(keys_per_frame):
        for key in np.unique(keys[keys >= 0]):
            frames_of.setdefault(int(key), []).append(f)
    units = np.array(sorted(frames_of), np.int64)
    at = {int(k): i for i, k in enumerate(units)}
    frame_ofs = np.zeros(len(units) + 1, np.int64)
    frame_idx = []
    for i, k in enumerate(units):
        frame_idx += sorted(frames_of[int(k)])
        frame_ofs[i + 1] = len(frame_idx)
    nb = np.full((len(units), 3), -1, np.int32)
    for i, ijk in enumerate(unpack(units).reshape(-1, 3)):
        for a in range(3):
            n = ijk.copy()
            n[a] += 1
            if n[a] < BIAS:
                nb[i, a] = at.get(int(pack(*n)), -1)
    return units, frame_ofs, np.array(frame_idx, np.int32), nb


def voxel_centres(unit_ijk, voxel):
    """(4096, 3) fp64 centres of a unit's voxels, voxel (i, j, k) at (i 16 + j) 16 + k"""
    idx = np.indices((UNIT, UNIT, UNIT)).reshape(3, -1).T
    return np.asarray(unit_ijk, np.float64) * (16.0 * voxel) + (idx + 0.5) * voxel


def integrate(units, frame_ofs, frame_idx, depths, colors, T_CW, K, voxel, trunc):
    """-> tsdf (U,4096) f32, weight (U,4096) f32, color (U,4096,3) f32"""
    fx, fy, cx, cy = K
    F, W, H = depths.shape
    U = len(units)
    tsdf, weight, color = np.zeros((U, UNIT ** 3), np.float32), np.zeros((U, UNIT ** 3), np.float32), np.zeros((U, UNIT ** 3, 3), np.float32)
    one = np.float32(1)
    for ui, ijk in enumerate(unpack(units).reshape(-1, 3)):
        c = voxel_centres(ijk, voxel)
        f, w, col = tsdf[ui], weight[ui], color[ui]
        for fr in frame_idx[frame_ofs[ui]:frame_ofs[ui + 1]]:
            T = np.asarray(T_CW[fr], np.float64)
            with np.errstate(all="ignore"):
                x, y, z = [((T[a, 0] * c[:, 0] + T[a, 1] * c[:, 1]) + T[a, 2] * c[:, 2]) + T[a, 3] for a in range(3)]
                m = ~(z <= 0)
                uf, vf = (x * fx / z + cx) + 0.5, (y * fy / z + cy) + 0.5
                m &= (uf >= 0.0001) & (uf < W - 0.0001) & (vf >= 0.0001) & (vf < H - 0.0001)
                pu, pv = np.where(m, uf, 0).astype(np.int64), np.where(m, vf, 0).astype(np.int64)
                d = depths[fr][pu, pv]
                m &= d > 0
                a, b = (pu - cx) / fx, (pv - cy) / fy
                sdf = (d.astype(np.float64) - z) * np.sqrt((a * a + b * b) + 1.0)
                m &= sdf > -trunc
                t = np.minimum(1.0, sdf / trunc).astype(np.float32)
                wn = w + one
                f[m] = ((f * w + t) / wn)[m]
                col[m] = ((col * w[:, None] + colors[fr][pu, pv].astype(np.float32)) / wn[:, None])[m]
                w[m] = wn[m]
    return tsdf, weight, color


def extract(units, neighbours, tsdf, weight, color, voxel):
    """-> (points (n,3) f64, colors (n,3) f64) in the order unit, voxel, axis"""
    U = len(units)
    valid = (weight != 0) & (tsdf < np.float32(0.98)) & (tsdf >= np.float32(-0.98))
    shape = (U, UNIT, UNIT, UNIT)
    f0, v0, c0 = tsdf.reshape(shape), valid.reshape(shape), color.reshape(shape + (3,))
    cross = np.zeros(shape + (3,), bool)
    f1s, c1s = [], []
    for a in range(3):
        f1, v1, c1 = np.zeros_like(f0), np.zeros_like(v0), np.zeros_like(c0)
        inner, first, last = [slice(None)] * 4, [slice(None)] * 4, [slice(None)] * 4
        inner[a + 1], first[a + 1], last[a + 1] = slice(1, None), 0, UNIT - 1
        head = [slice(None)] * 4
        head[a + 1] = slice(0, UNIT - 1)
        f1[tuple(head)], v1[tuple(head)], c1[tuple(head)] = f0[tuple(inner)], v0[tuple(inner)], c0[tuple(inner)]
        has = neighbours[:, a] >= 0
        n = neighbours[has, a]
        lastu, firstn = [has] + last[1:], [n] + first[1:]
        f1[tuple(lastu)], v1[tuple(lastu)], c1[tuple(lastu)] = f0[tuple(firstn)], v0[tuple(firstn)], c0[tuple(firstn)]
        cross[..., a] = v0 & v1 & (f0 * f1 < 0)
        f1s.append(f1)
        c1s.append(c1)
    ui, i, j, k, a = np.nonzero(cross)                      # C order: unit, voxel, axis
    ijk = np.stack([i, j, k], 1)
    p = unpack(units[ui]).astype(np.float64) * (16.0 * voxel) + (ijk + 0.5) * voxel
    F1, C1 = np.stack(f1s, -1), np.stack(c1s, -2)           # (U,16,16,16,3), (U,16,16,16,3 axes,3 channels)
    r0, r1 = np.abs(f0[ui, i, j, k].astype(np.float64)), np.abs(F1[ui, i, j, k, a].astype(np.float64))
    rows = np.arange(len(ui))
    p0 = p[rows, a]
    p1 = p0 + voxel
    p[rows, a] = (p0 * r1 + p1 * r0) / (r0 + r1)
    cc0, cc1 = c0[ui, i, j, k].astype(np.float64), C1[ui, i, j, k, a].astype(np.float64)
    cols = (cc0 * r1[:, None] + cc1 * r0[:, None]) / (r0 + r1)[:, None] / 255.0
    return p, cols


def fuse(depths, colors, T_WC, K, voxel, trunc):
    """the whole volume of F frames -> dict of every stage (T_CW = np.linalg.inv(T_WC), as the product takes it)"""
    depths, T_WC = np.asarray(depths, np.float32), np.asarray(T_WC, np.float64)
    keys = [touch(depths[f], K, T_WC[f], voxel, trunc) for f in range(len(depths))]
    units, frame_ofs, frame_idx, nb = unit_tables(keys)
    tsdf, weight, color = integrate(units, frame_ofs, frame_idx, depths, np.asarray(colors), np.linalg.inv(T_WC), K, voxel, trunc)
    points, cols = extract(units, nb, tsdf, weight, color, voxel)
    return dict(keys=np.stack(keys), units=units, frame_ofs=frame_ofs, frame_idx=frame_idx, neighbours=nb, tsdf=tsdf, weight=weight,
                color=color, points=points, colors=cols)


def radius_counts(points, r):
    """(n,3) fp32 values -> (n,) counts of the points with (dx dx + dy dy) + dz dz < r r in fp64, the point itself included.
    Candidates come from a cKDTree with a radius a little larger; the decision is the contract's arithmetic."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, np.float32).astype(np.float64)
    counts = np.ones(len(p), np.int64)
    pairs = cKDTree(p).query_pairs(r * (1 + 1e-6), output_type="ndarray")
    if len(pairs):
        d = p[pairs[:, 0]] - p[pairs[:, 1]]
        near = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r * r
        counts += np.bincount(pairs[near].reshape(-1), minlength=len(p))
    return counts


def radius_counts_brute(points, r):
    p = np.asarray(points, np.float32).astype(np.float64)
    d = p[:, None, :] - p[None, :, :]
    return (((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < r * r).sum(1)


# ---- scenes ------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera -> world pose (4,4): the camera at `eye`, its z axis towards `target`"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def render_plane(normal, offset, K, T_WC, W, H, rng=None, quantum=0.001):
    """metric (W,H) f32 depth of the plane normal . p = offset seen from T_WC (0 where the ray misses it), rounded to `quantum`,
    and a (W,H,3) u8 image"""
    fx, fy, cx, cy = K
    x, y = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    rays = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x, dtype=np.float64)], -1) @ T_WC[:3, :3].T
    n = np.asarray(normal, np.float64)
    denom = rays @ n
    with np.errstate(all="ignore"):
        d = (offset - T_WC[:3, 3] @ n) / denom
    d = np.where(np.isfinite(d) & (d > 0), d, 0.0)
    d = (np.round(d / quantum) * quantum).astype(np.float32)
    img = np.stack([(x * 7 + y * 3) % 256, (x * 5 + 11) % 256, (y * 13 + 1) % 256], -1).astype(np.uint8)
    return d, img
