"""numpy restatement of ScanNet mask refinement (cnr_amd.utils.geometry_segmentation / refine_inst_data, csrc/geoseg.hip;
DESIGN.md section 3.12), stage by stage in the kernels' own arithmetic: fp32 images, every product, sum, quotient and square
root rounded on its own.  The normals come from tests/fpfh_cpu.py.  tests/test_geoseg_host.py checks the restated labelling,
hole filling and morphology against scipy.ndimage and the vote against what the reference's refine_inst_data recorded
(tests/golden/geoseg/refine_cases.npz); tests/test_geoseg_gpu.py compares the kernels with this file, array_equal."""
import functools

import numpy as np

import fpfh_cpu as FC

F32 = np.float32
NORMAL_RADIUS, NORMAL_MAX_NN = 0.1, 100


# ---- 2.1 point map and normals -------------------------------------------------------------------------------------------
def point_map(depth, fx, fy, cx, cy):
    """(H,W) f32 depth -> P (H,W,3) f32: x = (u - cx) z / fx, y = (v - cy) z / fy in fp64 from the f32 depth, zero where invalid"""
    d = np.asarray(depth, F32)
    H, W = d.shape
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = d.astype(np.float64)
    P = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], -1).astype(F32)
    P[~(d > 0)] = 0
    return P


def normal_image(P, depth, parts=False):
    """normals of the valid pixels in raster order (hybrid search 0.1 / 100 on the f32 points), negated where n_z > 0 -> (H,W,3) f32
    [, the fp64 normals (n,3), the neighbour counts (n,), the eigenvalues ascending (n,3)]"""
    valid = np.asarray(depth) > 0
    pts = P[valid]
    idx, _, count = FC.hybrid_search(pts, NORMAL_RADIUS, NORMAL_MAX_NN)
    n, lam = FC.estimate_normals(pts, idx, count, return_eigen=True)
    n = np.where(n[:, 2:] > 0, -n, n)
    N = np.zeros(P.shape, F32)
    N[valid] = n.astype(F32)
    return (N, n, count, lam) if parts else N


# ---- morphology ------------------------------------------------------------------------------------------------------------
def _window(a, fill, reduce):
    """3x3 reduction, pixels outside the image ignored (they hold `fill`, the reduction's neutral element)"""
    H, W = a.shape
    p = np.full((H + 2, W + 2), fill, a.dtype)
    p[1:-1, 1:-1] = a
    out = a.copy()
    for dy in range(3):
        for dx in range(3):
            out = reduce(out, p[dy:dy + H, dx:dx + W])
    return out


def erode3(a):
    a = np.asarray(a)
    return _window(a, np.inf if a.dtype.kind == "f" else np.iinfo(a.dtype).max, np.minimum)


def dilate3(a):
    a = np.asarray(a)
    return _window(a, -np.inf if a.dtype.kind == "f" else np.iinfo(a.dtype).min, np.maximum)


def reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


# ---- 2.2 / 2.3 -------------------------------------------------------------------------------------------------------------
def maps(P, N, depth):
    """-> (disc, conv) uint8"""
    d = np.asarray(depth, F32)
    P, N = np.asarray(P, F32), np.asarray(N, F32)
    H, W = d.shape
    ero, dil = erode3(d), dilate3(d)
    valid = d > 0
    ratio = np.where(valid, np.maximum(d - ero, dil - d) / np.where(valid, d, F32(1)), F32(0)).astype(F32)
    disc = ratio > F32(0.01)
    m = np.full((H, W), 10, F32)
    ys, xs = np.mgrid[0:H, 0:W]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy == 0 and dx == 0:
                continue
            ny, nx = reflect101(ys + dy, H), reflect101(xs + dx, W)
            e = P[ny, nx] - P
            dot = (e[..., 0] * (-N[..., 0]) + e[..., 1] * (-N[..., 1])) + e[..., 2] * (-N[..., 2])
            Nn = N[ny, nx]
            proj = (N[..., 0] * Nn[..., 0] + N[..., 1] * Nn[..., 1]) + N[..., 2] * Nn[..., 2]
            m = np.minimum(m, np.where(dot > F32(-0.0005), F32(1), proj))
    assert m.dtype == F32 and ratio.dtype == F32
    return disc.astype(np.uint8), (m > F32(0.9)).astype(np.uint8)


def edge_map(disc, conv, depth):
    """1 = region pixel: open3(conv) & ~close3(disc) & (depth > 0)"""
    opened = dilate3(erode3(np.asarray(conv, np.uint8)))
    closed = erode3(dilate3(np.asarray(disc, np.uint8)))
    return ((opened != 0) & (closed == 0) & (np.asarray(depth) > 0)).astype(np.uint8)


# ---- 2.4 connected components ----------------------------------------------------------------------------------------------
def ccl(mask, connectivity=8):
    """(H,W) or (F,H,W) mask -> int32 labels: the smallest raster index of the pixel's component within its frame, -1 outside
    the mask.  A sequential union/find (the smaller root wins), nothing of the kernel's tiling."""
    mask = np.asarray(mask)
    if mask.ndim == 3:
        return np.stack([ccl(m, connectivity) for m in mask]) if len(mask) else np.zeros(mask.shape, np.int32)
    if connectivity not in (4, 8):
        raise ValueError("connectivity 4 or 8")
    H, W = mask.shape
    m = (mask != 0).ravel().tolist()
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for p in range(H * W):
        if not m[p]:
            continue
        y, x = divmod(p, W)
        for dy, dx in back:
            yy, xx = y + dy, x + dx
            if yy < 0 or xx < 0 or xx >= W or not m[yy * W + xx]:
                continue
            a, b = find(p), find(yy * W + xx)
            if a != b:
                parent[max(a, b)] = min(a, b)
    out = np.full(H * W, -1, np.int32)
    for p in range(H * W):
        if m[p]:
            out[p] = find(p)
    return out.reshape(H, W)


def label_counts(labels):
    """(H,W) labels -> (H,W) int32: counts.ravel()[l] = pixels with label l"""
    labels = np.asarray(labels)
    return np.bincount(labels[labels >= 0].ravel(), minlength=labels.size).astype(np.int32).reshape(labels.shape)


# ---- 2.5 growth and segments -----------------------------------------------------------------------------------------------
def drop_small(labels, min_count):
    c = label_counts(labels).ravel()
    return np.where((labels >= 0) & (c[np.maximum(labels, 0)] >= min_count), labels, -1).astype(np.int32)


def grow(P, depth, edge, labels):
    """labels: int32 with -1 where edge == 0 (small components already dropped) -> the second label image"""
    P, d, edge = np.asarray(P, F32), np.asarray(depth, F32), np.asarray(edge)
    H, W = d.shape
    out = np.where(edge != 0, labels, -1).astype(np.int32)
    src = out.copy()
    is_edge = (edge == 0) & (d > 0)
    best = np.full((H, W), 0.05, F32)
    ys, xs = np.mgrid[0:H, 0:W]
    for i in range(-4, 5):
        for j in range(-4, 5):
            if i == 0 and j == 0:
                continue
            xo, yo = xs + i, ys + j
            cand = is_edge & (xo >= 0) & (xo < W) & (yo >= 0) & (yo < H)
            y, x, qy, qx = ys[cand], xs[cand], yo[cand], xo[cand]
            e = P[y, x] - P[qy, qx]
            dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
            assert dist.dtype == F32
            ql = src[qy, qx]
            ok = (edge[qy, qx] != 0) & (ql >= 0) & (dist < best[y, x])
            out[y[ok], x[ok]] = ql[ok]
            best[y[ok], x[ok]] = dist[ok]
    return out


def segment_ids(grown, min_pixels):
    c = label_counts(grown).ravel()
    return np.flatnonzero(c >= min_pixels).astype(np.int32)


# ---- 2.6 / 2.7 -------------------------------------------------------------------------------------------------------------
def fill_holes(mask, ccl_fn=None):
    """binary_fill_holes with its default structure: the mask plus the 4-connected components of its complement that do not
    touch the image border"""
    mask = np.asarray(mask) != 0
    lab = (ccl_fn or ccl)(~mask, 4)
    border = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
    open_roots = np.unique(border[border >= 0])
    return mask | ((lab >= 0) & ~np.isin(lab, open_roots))


def object_ids(inst):
    ids = np.unique(np.asarray(inst))
    return ids[(ids != 0) & (ids != -1)]


def vote(inst, filled_masks, threshold=0.7):
    """-> (refined of inst's dtype, chosen: per segment the index into object_ids or -1)"""
    inst = np.asarray(inst)
    ids = object_ids(inst)
    refined = np.zeros_like(inst)
    chosen = np.full(len(filled_masks), -1, np.int64)
    if len(ids) == 0:
        return refined, chosen
    for k, f in enumerate(filled_masks):
        total = int(f.sum())
        if total == 0:
            continue
        rates = np.array([float(int((f & (inst == o)).sum())) / float(total) for o in ids])
        if rates.max() > threshold:
            chosen[k] = int(np.argmax(rates))
            refined[f] = ids[chosen[k]]
    return refined, chosen


def refine_inst_data(inst, segment_masks, threshold=0.7, ccl_fn=None):
    return vote(inst, [fill_holes(m, ccl_fn) for m in segment_masks], threshold)[0]


# ---- the colouring ---------------------------------------------------------------------------------------------------------
def label_colormap(n=256):
    """the PASCAL-VOC colormap: bit b of id >> 3j goes to bit 7 - j of the channel b"""
    cmap = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap[i] = (r, g, b)
    return cmap


# ---- the whole of 2.2 - 2.5 ------------------------------------------------------------------------------------------------
def segmentation(P, N, depth, min_area=500, min_pixels=500, ccl_fn=None):
    """-> dict(disc, conv, edge, labels, kept, grown, seg_ids, masks, output)"""
    disc, conv = maps(P, N, depth)
    edge = edge_map(disc, conv, depth)
    labels = (ccl_fn or ccl)(edge, 8)
    kept = drop_small(labels, min_area)
    grown = grow(P, depth, edge, kept)
    ids = segment_ids(grown, min_pixels)
    masks = [grown == i for i in ids]
    output = np.zeros(grown.shape + (3,), np.uint8)
    cmap = label_colormap()
    for k, m in enumerate(masks):
        output[m] = cmap[k % 256]
    return dict(disc=disc, conv=conv, edge=edge, labels=labels, kept=kept, grown=grown, seg_ids=ids, masks=masks, output=output)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
W_PX, H_PX = 96, 80
INTRINSICS = dict(fx=100.0, fy=100.0, cx=47.5, cy=39.5)
ID_A, ID_B, ID_POSTER = 3, 5, 9
RECT_A = (10, 39, 15, 59)            # u0, u1, v0, v1, inclusive
RECT_B = (55, 87, 20, 64)
BOXES_MIN = 200                      # min_area = min_pixels of scene "boxes"


def _rect_mask(r, grow_by=0):
    m = np.zeros((H_PX, W_PX), bool)
    u0, u1, v0, v1 = r
    m[max(v0 - grow_by, 0):v1 + 1 + grow_by, max(u0 - grow_by, 0):u1 + 1 + grow_by] = True
    return m


@functools.lru_cache(maxsize=None)
def scene_boxes():
    """a wall at 2.0 m, rectangle A at 1.2 m and B at 1.5 m in front of it, a 6x6 patch without depth in the wall; the raw
    instance map holds A's mask dilated by 3 px, B's shifted by 3 px and a 20x20 poster on the bare wall
    -> dict(depth, rgb, inst, P, N, A, B)"""
    depth = np.full((H_PX, W_PX), 2.0, F32)
    A, B = _rect_mask(RECT_A), _rect_mask(RECT_B)
    depth[A], depth[B] = 1.2, 1.5
    depth[68:74, 44:50] = 0.0
    inst = np.zeros((H_PX, W_PX), np.int32)
    inst[_rect_mask(RECT_A, 3)] = ID_A
    inst[np.roll(B, 3, axis=1)] = ID_B
    inst[1:21, 41:54] = ID_POSTER                     # the bare wall between the rectangles is 15 px wide: 20 x 13
    inst[60:80, 12:32] = ID_POSTER                    # and 20 x 20 below A, over the rows A's dilation reaches
    return _finish(depth, inst, dict(A=A, B=B), seed=1)


def room_depth(H, W, fx, fy, cx, cy, n_holes, seed):
    """a slanted floor meeting a slightly turned wall (a concave junction) and a sphere that grows out of the wall, seen by any
    camera; n_holes pixels without depth -> (depth (H,W) f32, the sphere's pixels)"""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b = (u - cx) / fx, (v - cy) / fy
    wall = 2.5 / (1.0 - 0.1 * a)                                      # z - 0.1 x = 2.5
    floor = np.where(b + 0.2 > 0, 1.0 / np.maximum(b + 0.2, 1e-9), np.inf)         # y + 0.2 z = 1
    c, r = np.array([-0.25, -0.15, 2.65]), 0.5                       # the sphere: |z d - c| = r along d = (a, b, 1)
    dd, dc = a * a + b * b + 1.0, a * c[0] + b * c[1] + c[2]
    disc = dc * dc - dd * (c @ c - r * r)
    sphere = np.where(disc > 0, (dc - np.sqrt(np.maximum(disc, 0))) / dd, np.inf)
    depth = np.minimum(np.minimum(wall, floor), sphere).astype(F32)
    holes = np.random.default_rng(seed).choice(H * W, n_holes, replace=False)
    depth.ravel()[holes] = 0.0
    return depth, (sphere < wall) & (sphere < floor)


@functools.lru_cache(maxsize=None)
def scene_room():
    """room_depth at the scenes' camera: wall and floor run off the image on all four sides; 24 pixels without depth"""
    depth, on_sphere = room_depth(H_PX, W_PX, n_holes=24, seed=5, **INTRINSICS)
    inst = np.zeros((H_PX, W_PX), np.int32)
    inst[on_sphere] = ID_A
    inst[50:, :40] = ID_B
    return _finish(depth, inst, {}, seed=2)


def _finish(depth, inst, extra, seed):
    P = point_map(depth, **INTRINSICS)
    rgb = np.random.default_rng(seed).integers(0, 256, depth.shape + (3,), dtype=np.uint8)
    N, n64, count, lam = normal_image(P, depth, parts=True)
    return dict(depth=depth, rgb=rgb, inst=inst, P=P, N=N, normals64=n64, count=count, eigenvalues=lam, **extra)


SCENES = {"boxes": (scene_boxes, BOXES_MIN), "room": (scene_room, BOXES_MIN)}


# ---- adversarial masks -----------------------------------------------------------------------------------------------------
def spiral(H, W):
    """a one-pixel-wide rectangular spiral, one component, crossing every 16-pixel tile border many times"""
    m = np.zeros((H, W), np.uint8)
    y0, x0, y1, x1 = 0, 0, H - 1, W - 1
    first = True
    while y0 <= y1 and x0 <= x1:
        m[y0, (x0 if first else max(x0 - 2, 0)):x1 + 1] = 1
        m[y0:y1 + 1, x1] = 1
        if y1 - y0 >= 2:
            m[y1, x0:x1 + 1] = 1
        if x1 - x0 >= 2 and y1 - y0 >= 2:
            m[y0 + 2:y1 + 1, x0] = 1
        y0, x0, y1, x1, first = y0 + 2, x0 + 2, y1 - 2, x1 - 2, False
    return m


def serpentine(H, W):
    """full rows two apart, joined alternately at the right and the left end"""
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def u_shapes(H, W):
    """columns two apart joined only by the bottom row: the roots of all columns meet last"""
    m = np.zeros((H, W), np.uint8)
    m[:, ::2] = 1
    m[H - 1] = 1
    return m


def frame_ring(H, W):
    m = np.zeros((H, W), np.uint8)
    m[0], m[-1], m[:, 0], m[:, -1] = 1, 1, 1, 1
    m[H // 2, W // 2] = 1
    return m


def checkerboard(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys + xs) % 2 == 0).astype(np.uint8)


def ccl_masks(H=70, W=45):
    rng = np.random.default_rng(11)
    return {"zeros": np.zeros((H, W), np.uint8), "ones": np.ones((H, W), np.uint8), "checkerboard": checkerboard(H, W),
            "spiral": spiral(H, W), "serpentine": serpentine(H, W), "u_shapes": u_shapes(H, W), "frame_ring": frame_ring(H, W),
            "random_half": (rng.random((H, W)) < 0.5).astype(np.uint8), "random_dense": (rng.random((H, W)) < 0.62).astype(np.uint8),
            "row": (rng.random((1, 131)) < 0.7).astype(np.uint8), "column": (rng.random((77, 1)) < 0.7).astype(np.uint8)}


def fill_masks():
    """name -> mask for the hole filling: nested rings, a hole that meets the border only diagonally (4-connectivity does not
    leak: filled), a hole open to the border"""
    H, W = 40, 52
    nested = np.zeros((H, W), np.uint8)
    for k in (2, 6, 10, 14):
        nested[k:H - k, k:W - k] = 1
        nested[k + 1:H - k - 1, k + 1:W - k - 1] = 0
    nested[19:21, 24:28] = 1
    diagonal = np.zeros((H, W), np.uint8)
    diagonal[0, 1:6], diagonal[1:6, 0], diagonal[5, 1:6], diagonal[1:6, 5] = 1, 1, 1, 1     # hole 1..4 x 1..4 next to corner (0,0)
    diagonal[20:30, 20:30], diagonal[23:27, 23:27] = 1, 0
    opened = np.zeros((H, W), np.uint8)
    opened[5:30, 5:30], opened[8:27, 8:27] = 1, 0
    opened[15, 0:9] = 0
    opened[5:30, 5] = 1
    opened[15, 5] = 0                                   # a gap in the ring: the hole is open to the outside
    return {"nested": nested, "diagonal": diagonal, "open": opened}


def tie_plane(H=24, W=33, col=16):
    """a fronto-parallel plane at 1 m cut by a one-pixel vertical line of edge pixels between two labels: for the pixels of the
    line the left and the right neighbour are equally far, and the left one comes first in the loop order"""
    depth = np.ones((H, W), F32)
    P = point_map(depth, fx=64.0, fy=64.0, cx=float(col), cy=12.0)      # u - cx = -1 and +1: the same |x| to the last bit
    edge = np.ones((H, W), np.uint8)
    edge[:, col] = 0
    labels = np.where(np.arange(W)[None] < col, 0, col + 1).astype(np.int32) * np.ones((H, 1), np.int32)
    labels[:, col] = -1
    return P, depth, edge, labels


def refine_cases():
    """name -> (inst (H,W) int32, masks (K,H,W) bool): the inputs whose refine_inst_data outputs the reference recorded
    (tests/golden/gen_geoseg_golden.py -> tests/golden/geoseg/refine_cases.npz)"""
    H, W = 24, 30
    out = {}

    def blank():
        return np.zeros((H, W), np.int32)

    def box(v0, v1, u0, u1):
        m = np.zeros((H, W), bool)
        m[v0:v1, u0:u1] = True
        return m

    inst = blank()
    inst[3, 4:9], inst[4, 4:6] = 4, 4                     # 7 of the segment's 10 pixels: a rate of exactly 7/10 does not assign
    out["rate_equal"] = (inst, np.stack([box(3, 5, 4, 9)]))
    inst = blank()
    inst[2:9, 3:13], inst[9, 3:4] = 4, 4                  # 71 of 100
    inst[15:20, 3:13] = 8
    out["rate_above"] = (inst, np.stack([box(2, 12, 3, 13)]))
    inst = blank()
    inst[2:14, 2:16], inst[6:20, 10:28] = 4, 6
    out["overlap_later_wins"] = (inst, np.stack([box(2, 14, 2, 16), box(6, 20, 10, 28)]))
    ring = box(3, 21, 4, 26) & ~box(5, 19, 6, 24)
    island = box(9, 14, 11, 18)
    inst = blank()
    inst[2:22, 3:27], inst[9:14, 11:18] = 6, 4
    out["ring_swallows_island"] = (inst, np.stack([island, ring]))
    out["island_after_ring"] = (inst, np.stack([ring, island]))
    inst = blank()
    inst[:, :10] = -1
    out["no_objects"] = (inst, np.stack([box(2, 12, 3, 13)]))
    d = fill_masks()["diagonal"] != 0
    inst = np.zeros(d.shape, np.int32)
    inst[0:6, 0:6], inst[20:30, 20:30] = 5, 7
    inst[0, 0] = 0
    out["diagonal_hole"] = (inst, np.stack([d]))
    out["int64_ids"] = (out["overlap_later_wins"][0].astype(np.int64) * 1000, out["overlap_later_wins"][1])
    return out
