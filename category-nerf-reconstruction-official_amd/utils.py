"""Ensemble glue with the reference's signature (src/utils.py:24-28).

``update_vmap(models, optimiser)`` stacks the per-class modules' parameters into ``(C, ...)`` leaves,
registers them as a new param group, and returns ``(fmodel, params, buffers)`` such that
``functorch.vmap(fmodel)(params, buffers, *stacked_inputs)`` -- the exact call at train.py:154-155 --
lands in the class-batched HIP kernels through the Functions' ``vmap`` rules (ops.py).
"""
import numpy as np
import torch
from torch.func import functional_call, stack_module_state


def combine_state_for_ensemble(models):
    """(fmodel, params, buffers) like functorch's helper: params/buffers are tuples of stacked
    tensors in ``named_parameters()`` / ``named_buffers()`` order."""
    params, buffers = stack_module_state(models)
    pnames, bnames = list(params.keys()), list(buffers.keys())
    base = models[0]

    def fmodel(p, b, *args, **kwargs):
        state = {n: t for n, t in zip(pnames, p)}
        state.update({n: t for n, t in zip(bnames, b)})
        return functional_call(base, state, args, kwargs)

    return fmodel, tuple(params[n] for n in pnames), tuple(buffers[n] for n in bnames)


def update_vmap(models, optimiser):
    fmodel, params, buffers = combine_state_for_ensemble(models)
    [p.requires_grad_() for p in params]
    optimiser.add_param_group({"params": params})
    return (fmodel, params, buffers)


# ---- sim3 <-> 8-vector [scale, qw, qx, qy, qz, tx, ty, tz] ------------------------------------------------------------
# The form the reference keeps per object in ``sceneCategory.object_tensor_dict`` and writes into checkpoints
# (src/utils.py:367-447 get_tensor_from_transform_sim3 / get_transform_from_tensor_sim3; consumers read element 0 as the
# scale and elements 1: as quaternion + translation, train.py:231-234, src/scene_cateogries.py:378-379).
def get_tensor_from_transform_sim3(RT):
    """(4,4) sim3 (numpy or tensor) -> float32 tensor (8,).  scale = det(R s)^(1/3); the quaternion comes from scipy's
    Rotation (w first), the same third-party routine the reference calls, so the numbers are identical."""
    import numpy as np
    from scipy.spatial.transform import Rotation
    M = np.array(RT.detach().cpu().numpy() if torch.is_tensor(RT) else RT, dtype=np.float64)
    scale = np.linalg.det(M[:3, :3]) ** (1.0 / 3.0)
    scale32 = torch.tensor([scale], dtype=torch.float32)
    Rm = M[:3, :3] / scale32.numpy()                      # the reference divides by the float32 scale tensor
    x, y, z, w = Rotation.from_matrix(Rm).as_quat()
    vec = np.concatenate([[w, x, y, z], M[:3, 3]])
    return torch.cat([scale32, torch.from_numpy(vec).float()], 0)


def get_transform_from_tensor_sim3(vec):
    """(8,) or (n,8) [scale, qw, qx, qy, qz, t] -> (4,4) / (n,4,4) sim3 matrices (differentiable torch ops)."""
    single = vec.dim() == 1
    v = vec[None] if single else vec
    s, q, t = v[:, 0], v[:, 1:5], v[:, 5:8]
    qr, qi, qj, qk = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    R = torch.stack([1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                     two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                     two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)],
                    -1).view(-1, 3, 3)
    T = torch.eye(4, device=v.device, dtype=v.dtype).repeat(v.shape[0], 1, 1)
    T[:, :3, :3] = R * s[:, None, None]
    T[:, :3, 3] = t
    return T[0] if single else T


def quad2rotation(quad):
    """(n,4) quaternions [r, i, j, k] (need not be unit) -> (n,3,3) rotations (src/utils.py:468-491)"""
    qr, qi, qj, qk = quad.unbind(-1)
    two_s = 2.0 / (quad * quad).sum(-1)
    return torch.stack([1 - two_s * (qj ** 2 + qk ** 2), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                        two_s * (qi * qj + qk * qr), 1 - two_s * (qi ** 2 + qk ** 2), two_s * (qj * qk - qi * qr),
                        two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi ** 2 + qj ** 2)],
                       -1).view(-1, 3, 3)


def get_transform_from_tensor(inputs):
    """(7,) or (n,7) [qr, qi, qj, qk, tx, ty, tz] -> (4,4) / (n,4,4) rigid transforms (src/utils.py:411-430; train.py:232 calls
    it on object_tensor_dict[obj][1:])."""
    single = inputs.dim() == 1
    v = inputs[None] if single else inputs
    RT = torch.eye(4, device=v.device, dtype=v.dtype).repeat(v.shape[0], 1, 1)
    RT[:, :3, :3] = quad2rotation(v[:, :4])
    RT[:, :3, 3] = v[:, 4:7]
    return RT[0] if single else RT


# ---- dataset helpers (src/utils.py:16-22, :30-51, :69-78, :322-327) ---------------------------------------------------
class BoundingBox():
    """An oriented 3-D box as the registration result stores it (bbox3D of inst_dict.pkl): extent, R, center, points3d (8,3)."""

    def __init__(self):
        super(BoundingBox, self).__init__()
        self.extent = None
        self.R = None
        self.center = None
        self.points3d = None


def enlarge_bbox(bbox, scale, w, h):
    """[min_x, min_y, max_x, max_y] grown by int(0.5 * scale * size) per side, clipped to [0, w-1] x [0, h-1]; None when either
    margin is 0.  Arithmetic is whatever the inputs carry: torch tensors (Replica) give float32 margins, ints give double."""
    assert scale >= 0
    import numpy as np
    min_x, min_y, max_x, max_y = bbox
    margin_x = int(0.5 * scale * (max_x - min_x))
    margin_y = int(0.5 * scale * (max_y - min_y))
    if margin_x == 0 or margin_y == 0:
        return None
    min_x, max_x = np.clip(min_x - margin_x, 0, w - 1), np.clip(max_x + margin_x, 0, w - 1)
    min_y, max_y = np.clip(min_y - margin_y, 0, h - 1), np.clip(max_y + margin_y, 0, h - 1)
    return [int(min_x), int(min_y), int(max_x), int(max_y)]


def get_bbox2d_batch(img):
    """(b, h, w) masks -> (rmins, rmaxs, cmins, cmaxs) int64: first row with a set pixel, one past the last, the same for
    columns (0 and h / w for an empty mask, as torch.argmax gives)."""
    b, h, w = img.shape[:3]
    rows, cols = torch.any(img, axis=2).float(), torch.any(img, axis=1).float()
    rmins = torch.argmax(rows, dim=1)
    rmaxs = h - torch.argmax(rows.flip(dims=[1]), dim=1)
    cmins = torch.argmax(cols, dim=1)
    cmaxs = w - torch.argmax(cols.flip(dims=[1]), dim=1)
    return rmins, rmaxs, cmins, cmaxs


def load_matrix_from_txt(path, shape=(4, 4)):
    """whitespace-separated floats of a text file -> float64 array of `shape`"""
    import numpy as np
    with open(path) as f:
        values = [float(v) for v in f.read().split()]
    return np.array(values).reshape(shape)


# ---- point clouds for category registration (src/utils.py:189-366) -----------------------------------------------------
# DESIGN.md §3.9.  The reference builds these on open3d / trimesh; here the clouds live on the device and the unprojection,
# voxel down-sample and nearest-neighbour work are kernels of csrc/pointcloud.hip.
def _cuda_device(device=None):
    if device is not None and torch.device(device).type == "cuda":
        return torch.device(device)
    return torch.device("cuda", torch.cuda.current_device())


def voxel_down_sample_device(points, colors, voxel_size):
    """open3d's voxel_down_sample on (n,3) f32 device points (colors (n,3) f32 or None): voxel index floor((p - (min - v / 2)) / v)
    per axis in fp64, the mean of each voxel's points and colours in fp64, summed in input order.
    -> (points (m,3) f64, colors (m,3) f64 or None, keys (m,) i64, counts (m,) i64), voxels in ascending (ix, iy, iz)."""
    from . import _C
    lib = _C.load()
    points = points.contiguous()
    n, dev = len(points), points.device
    if n == 0:
        raise ValueError("voxel_down_sample of an empty point cloud")
    if not voxel_size > 0:
        raise ValueError("voxel_size must be positive")
    mn = torch.empty(3, device=dev, dtype=torch.float32)
    _C.call("cnr_points_min", points, n, _C.workspace(lib.cnr_points_min_workspace_bytes(n), dev, "cnr_points_min"), mn)
    keys = torch.empty(n, device=dev, dtype=torch.int64)
    _C.call("cnr_voxel_keys", points, n, mn, float(voxel_size), keys)
    skeys, perm = torch.sort(keys, stable=True)
    ws = _C.workspace(lib.cnr_voxel_segments_workspace_bytes(n), dev, "cnr_voxel_segments")
    cnt = torch.empty(2, device=dev, dtype=torch.int64)
    _C.call("cnr_voxel_segments_count", skeys, n, ws, cnt[:1])
    cnt[1] = skeys[0]
    m, first = (int(v) for v in cnt.cpu())
    if first < 0:
        raise ValueError("voxel_down_sample: non-finite points, or more than 2^21 voxels along an axis")
    out_p = torch.empty(m, 3, device=dev, dtype=torch.float64)
    out_c = torch.empty(m, 3, device=dev, dtype=torch.float64) if colors is not None else None
    out_k = torch.empty(m, device=dev, dtype=torch.int64)
    out_n = torch.empty(m, device=dev, dtype=torch.int64)
    _C.call("cnr_voxel_segments_emit", skeys, perm, points, colors.contiguous() if colors is not None else None, n, ws,
            out_p, out_c, out_k, out_n)
    return out_p, out_c, out_k, out_n


class PointCloud:
    """The part of open3d.geometry.PointCloud that registration uses, on the device: ``points`` / ``colors`` (numpy float64
    views of the fp32 device arrays, as np.asarray(pcd.points) gives), ``+=``, ``voxel_down_sample``,
    ``compute_point_cloud_distance`` and ``estimate_normals`` / ``normals`` (float64, device-backed; ``voxel_down_sample`` and
    ``+=`` drop them).  ``remove_radius_outlier`` keeps the kept points' normals."""

    def __init__(self, points=None, colors=None, device=None):
        dev = points.device if torch.is_tensor(points) and points.is_cuda else _cuda_device(device)
        as_dev = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(
            device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        self.points_device = as_dev(points) if points is not None else torch.zeros(0, 3, device=dev)
        self.colors_device = as_dev(colors) if colors is not None else None
        self.normals_device = None
        if self.colors_device is not None and len(self.colors_device) != len(self.points_device):
            raise ValueError("a colour per point")

    def __len__(self):
        return len(self.points_device)

    @property
    def points(self):
        return self.points_device.double().cpu().numpy()

    @property
    def colors(self):
        return self.colors_device.double().cpu().numpy() if self.colors_device is not None else np.zeros((0, 3))

    @property
    def normals(self):
        return self.normals_device.cpu().numpy() if self.normals_device is not None else np.zeros((0, 3))

    def has_normals(self):
        return self.normals_device is not None

    def estimate_normals(self, radius, max_nn):
        """open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) with this package's orientation (every normal
        points away from the cloud's centroid): fills `normals` (float64, held on the device)"""
        self.normals_device = estimate_normals_device(self.points_device, radius, max_nn)
        return self

    def __iadd__(self, other):
        self.normals_device = None
        both = self.colors_device is not None and other.colors_device is not None and len(self) and len(other)
        if len(self) == 0:
            self.points_device, self.colors_device = other.points_device, other.colors_device
            return self
        if len(other) == 0:
            return self
        self.colors_device = torch.cat([self.colors_device, other.colors_device.to(self.points_device.device)]) if both else None
        self.points_device = torch.cat([self.points_device, other.points_device.to(self.points_device.device)])
        return self

    def voxel_down_sample(self, voxel_size):
        p, c, _, _ = voxel_down_sample_device(self.points_device, self.colors_device, voxel_size)
        return PointCloud(p.float(), c.float() if c is not None else None)

    def remove_radius_outlier(self, nb_points, radius):
        """open3d's remove_radius_outlier: the points with more than nb_points points of this cloud, themselves included, closer
        than radius (radius_neighbour_counts) -> (the cloud of the kept points in their order, kept_index (m,) int64 device)"""
        if len(self) == 0:
            return PointCloud(self.points_device, self.colors_device), torch.zeros(0, dtype=torch.int64, device=self.points_device.device)
        kept = torch.nonzero(radius_neighbour_counts(self.points_device, radius) > int(nb_points)).reshape(-1)
        out = PointCloud(self.points_device[kept], self.colors_device[kept] if self.colors_device is not None else None)
        out.normals_device = self.normals_device[kept] if self.normals_device is not None else None
        return out, kept

    def compute_point_cloud_distance(self, other):
        """per point of this cloud the distance to the nearest point of `other` -> (n,) f32 device tensor"""
        from . import metrics
        return metrics.nn_dist(self.points_device, other.points_device)


def _intrinsics(intrinsic):
    if hasattr(intrinsic, "fx"):
        return float(intrinsic.fx), float(intrinsic.fy), float(intrinsic.cx), float(intrinsic.cy)
    K = np.asarray(intrinsic.intrinsic_matrix if hasattr(intrinsic, "intrinsic_matrix") else intrinsic, np.float64)
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _unproject_frames(frames, inst_ids, intrinsic, dev, return_counts=False):
    """frames: [(image (W,H,3) u8, depth (W,H) f32, obj_mask (W,H) i32, T_WC (4,4))], one instance id each -> PointCloud of all
    frames' kept pixels in frame order.  One read-back (the counts) for all frames; return_counts: -> (cloud, points per entry)."""
    from . import _C
    lib = _C.load()
    fx, fy, cx, cy = _intrinsics(intrinsic)
    up = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt).contiguous()
    staged, counts = [], torch.zeros(max(len(frames), 1), device=dev, dtype=torch.int64)
    for k, ((image, depth, mask, T_WC), inst_id) in enumerate(zip(frames, inst_ids)):
        d, m, im = up(depth, torch.float32), up(mask, torch.int32), up(image, torch.uint8)
        W, H = d.shape
        if m.shape != (W, H) or im.shape != (W, H, 3):
            raise ValueError("depth (W,H), obj_mask (W,H) and image (W,H,3) of one frame")
        ws = _C.workspace(lib.cnr_unproject_workspace_bytes(W, H), dev, "cnr_unproject")
        _C.call("cnr_unproject_count", d, m, W, H, int(inst_id), ws, counts[k:k + 1])
        T = torch.from_numpy(np.ascontiguousarray(np.asarray(T_WC, np.float64).reshape(4, 4))).to(dev)
        staged.append((d, m, im, W, H, int(inst_id), T, ws))
    counts = counts.cpu().numpy()[:len(frames)]
    total = int(counts.sum())
    points = torch.empty(total, 3, device=dev, dtype=torch.float32)
    colors = torch.empty(total, 3, device=dev, dtype=torch.float32)
    o = 0
    for (d, m, im, W, H, inst_id, T, ws), c in zip(staged, counts):
        if c:
            _C.call("cnr_unproject_emit", d, m, im, W, H, inst_id, fx, fy, cx, cy, T, ws, points[o:o + c], colors[o:o + c])
        o += int(c)
    return (PointCloud(points, colors), counts) if return_counts else PointCloud(points, colors)


def unproject_colored_pointcloud(rgb, depth, intrinsic_open3d, T_CW, device=None):
    """src/utils.py:341-351: the pixels with 0 < depth <= 8.0 (depth_trunc) of one (W,H) frame as a coloured cloud in the world
    frame, inv(T_CW) . ((u - cx) z / fx, (v - cy) z / fy, z, 1).  Points come in the memory order of the (W,H) arrays (u major);
    open3d walks its transposed image v major."""
    depth = depth if torch.is_tensor(depth) else np.asarray(depth)
    mask = torch.ones(tuple(depth.shape), dtype=torch.int32)
    return _unproject_frames([(rgb, depth, mask, np.linalg.inv(np.asarray(T_CW, np.float64)))], [1], intrinsic_open3d,
                             _cuda_device(device))


def accumulate_pointcloud(inst_id, inst_info_list, frame_samples, intrinsic_open3d, voxel_size=0.01, device=None):
    """src/utils.py:189-210: the instance's pixels of every frame of inst_info_list, unprojected into one cloud (frame order,
    then pixel order), then voxel_down_sample(voxel_size).  sample['T'] is the camera-to-world pose the kernel wants."""
    frames = []
    for entry in inst_info_list:
        s = frame_samples[entry["frame"]]
        if s["frame_id"] != entry["frame"]:
            raise ValueError(f"frame {entry['frame']}: sample_dict holds frame {s['frame_id']} under that key")
        frames.append((s["image"], s["depth"], s["obj_mask"], s["T"]))
    cloud = _unproject_frames(frames, [inst_id] * len(frames), intrinsic_open3d, _cuda_device(device))
    if len(cloud) == 0:
        raise ValueError(f"instance {inst_id}: no pixel with a valid depth in its {len(frames)} frames")
    return cloud.voxel_down_sample(voxel_size)


def unproject_pointcloud(depth, intrinsic_open3d, T_CW, device=None):
    """src/utils.py:329-339: the pixels with a positive depth of one frame as a cloud without colours in the world frame.  depth
    is the (H,W) image the reference hands to open3d; points come column by column (the kernel's order), not row by row, and a
    depth beyond 8 m -- which the loaders have already zeroed -- is dropped."""
    depth = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
    d = np.ascontiguousarray(depth.T, dtype=np.float32)
    cloud = _unproject_frames([(np.zeros(d.shape + (3,), np.uint8), d, np.ones(d.shape, np.int32),
                                np.linalg.inv(np.asarray(T_CW, np.float64)))], [1], intrinsic_open3d, _cuda_device(device))
    return PointCloud(cloud.points_device)


# ---- TSDF fusion (src/utils.py:212-247) --------------------------------------------------------------------------------
# open3d's ScalableTSDFVolume restated (equality with open3d is unverified), on the kernels of csrc/tsdf.hip.
TSDF_UNIT = 16                       # voxels per unit edge (volume_unit_resolution)
TSDF_AXIS_BITS = 21
TSDF_BLOCK_BYTES = 20 * TSDF_UNIT ** 3          # tsdf, weight and three colours, f32, per unit
DEFAULT_TSDF_BLOCK_BYTES = 32 << 30  # what a volume's blocks may take unless told otherwise (a room at 1 cm: about 1.6 GB)


def tsdf_depth_image(depth, obj_mask, inst_id, depth_scale=0.001, max_depth=6.0):
    """The depth image the volume sees, from a sample's metric (W,H) depth (device tensors): masked to obj_mask == inst_id,
    uint16(trunc(depth / depth_scale)) in fp64 (wrapping like numpy's astype), u16 / 1000 in fp32 (open3d's own default scale,
    whatever depth_scale is: the reference's quirk), 0 beyond max_depth -> (W,H) f32.  cnr_tsdf_depth_image: torch divides by a
    scalar as a product with its reciprocal on the device, which is not this contract."""
    from . import _C
    depth, obj_mask = depth.to(torch.float32).contiguous(), obj_mask.to(device=depth.device, dtype=torch.int32).contiguous()
    if depth.shape != obj_mask.shape or depth.numel() == 0:
        raise ValueError("depth and obj_mask of one frame")
    out = torch.empty_like(depth)
    _C.call("cnr_tsdf_depth_image", depth, obj_mask, depth.numel(), int(inst_id), float(depth_scale), float(max_depth), out)
    return out


def tsdf_unit_tables(keys, frames):
    """The torch side of cnr_tsdf_touch: keys (n,) int64 (negative = unused slot) with their frame numbers (n,), frames ascending
    -> (units (U,) ascending int64, frame_ofs (U+1,) int64, frame_idx (M,) int32: per unit its frames ascending, neighbours
    (U,3) int32: the +x, +y, +z unit or -1)"""
    used = keys >= 0
    keys, frames = keys[used], frames[used].to(torch.int64)
    order = torch.sort(keys, stable=True)[1]               # stable: the frames, ascending on entry, stay so inside a unit
    keys, frames = keys[order], frames[order]
    head = torch.ones(len(keys), dtype=torch.bool, device=keys.device)
    head[1:] = (keys[1:] != keys[:-1]) | (frames[1:] != frames[:-1])
    keys, frames = keys[head], frames[head]
    units, per_unit = torch.unique_consecutive(keys, return_counts=True)
    frame_ofs = torch.zeros(len(units) + 1, dtype=torch.int64, device=keys.device)
    frame_ofs[1:] = torch.cumsum(per_unit, 0)
    nb = torch.full((len(units), 3), -1, dtype=torch.int32, device=keys.device)
    if len(units):
        for a in range(3):
            shift = (2 - a) * TSDF_AXIS_BITS
            inside = ((units >> shift) & ((1 << TSDF_AXIS_BITS) - 1)) < (1 << TSDF_AXIS_BITS) - 1
            want = units + (1 << shift)
            at = torch.searchsorted(units, want).clamp_(max=len(units) - 1)
            nb[:, a] = torch.where(inside & (units[at] == want), at, torch.full_like(at, -1)).to(torch.int32)
    return units.contiguous(), frame_ofs, frames.to(torch.int32).contiguous(), nb.contiguous()


def _unit_neighbours(units):
    """tsdf_unit_tables' neighbours alone, for ascending unit keys"""
    return tsdf_unit_tables(units, torch.zeros(len(units), dtype=torch.int64, device=units.device))[3]


def tsdf_unit_neighbourhood(units):
    """units (U,) ascending int64 keys (device or CPU) -> hood (U,27) int32: for the offset (dx, dy, dz) in {-1,0,1}^3 at column
    (dx + 1) 9 + (dy + 1) 3 + (dz + 1) the index of that unit, or -1 where there is none or its index leaves the 21-bit range.
    Column 13 is the unit itself; columns 22, 16 and 14 are tsdf_unit_tables' +x, +y, +z neighbours.  What cnr_tsdf_mesh_count
    and _emit take: the three +1 columns do not chain to a diagonal (unit +x+y can exist while +x does not)."""
    units = units.to(torch.int64)
    U, mask = len(units), (1 << TSDF_AXIS_BITS) - 1
    if U == 0:
        return torch.full((0, 27), -1, dtype=torch.int32, device=units.device)
    # all 27 columns at once: (U,27,3) biased indices of the wanted units, one searchsorted
    shifts = torch.tensor([2 * TSDF_AXIS_BITS, TSDF_AXIS_BITS, 0], dtype=torch.int64, device=units.device)
    col = torch.arange(27, dtype=torch.int64, device=units.device)
    offsets = torch.stack([col // 9 - 1, col // 3 % 3 - 1, col % 3 - 1], 1)
    n = ((units[:, None] >> shifts) & mask)[:, None, :] + offsets[None]
    inside = ((n >= 0) & (n <= mask)).all(-1)
    want = torch.where(inside, (n << shifts).sum(-1), torch.full_like(inside, -1, dtype=torch.int64))
    at = torch.searchsorted(units, want.reshape(-1)).clamp_(max=U - 1).reshape(U, 27)
    return torch.where(units[at] == want, at, torch.full_like(at, -1)).to(torch.int32).contiguous()


class TSDFVolume:
    """ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8) for one batch of frames: integrate_frames once, then
    extract_point_cloud.  After integrate_frames: units, frame_ofs, frame_idx (and, on request, the kernel's slots),
    neighbours, tsdf (U,4096), weight (U,4096), color (U,4096,3).  max_block_bytes bounds what the blocks (20 KB per unit) may
    take; a larger volume raises CnrError before they are allocated."""

    def __init__(self, voxel_length=0.01, sdf_trunc=0.04, device=None, max_block_bytes=DEFAULT_TSDF_BLOCK_BYTES):
        if not (voxel_length > 0 and 0 < 2.0 * sdf_trunc <= TSDF_UNIT * voxel_length):
            raise ValueError("TSDFVolume: voxel_length > 0 and 0 < sdf_trunc <= 8 voxel_length (a depth sample's [p - trunc, p + trunc] "
                             "may span two units per axis, not three)")
        self.voxel_length, self.sdf_trunc, self.max_block_bytes = float(voxel_length), float(sdf_trunc), int(max_block_bytes)
        self.device = _cuda_device(device)
        self.units = None

    def integrate_frames(self, depths, colors, intrinsic, T_WC, keep_touch=False):
        """depths (F,W,H) f32 as tsdf_depth_image gives them, colors (F,W,H,3) u8, T_WC (F,4,4) camera -> world.  Each frame's
        touch slots are reduced to its distinct units at once, so the list that is sorted holds one entry per unit and frame;
        keep_touch=True keeps the raw slots as touch_keys / touch_frames (F, slots) for inspection."""
        from . import _C
        lib, dev = _C.load(), self.device
        if self.units is not None:
            raise ValueError("TSDFVolume: integrate_frames runs once per volume")
        fx, fy, cx, cy = _intrinsics(intrinsic)
        depths = torch.as_tensor(depths).to(device=dev, dtype=torch.float32).contiguous()
        colors = torch.as_tensor(colors).to(device=dev, dtype=torch.uint8).contiguous()
        F, W, H = depths.shape
        T_WC = np.ascontiguousarray(np.asarray(T_WC, np.float64).reshape(F, 4, 4))
        if colors.shape != (F, W, H, 3) or F < 1:
            raise ValueError("depths (F,W,H) and colors (F,W,H,3) of the same frames")
        slots = int(lib.cnr_tsdf_touch_slots(W, H))
        if slots < 0:
            raise _C.CnrError(f"cnr_tsdf_touch: a {W} x {H} frame is refused ({slots})")
        keys = torch.empty(F if keep_touch else 1, slots, device=dev, dtype=torch.int64)
        tags = torch.empty(F if keep_touch else 1, slots, device=dev, dtype=torch.int32)
        err = torch.zeros(1, device=dev, dtype=torch.int32)
        T_dev = torch.from_numpy(T_WC).to(dev)
        per_frame = []
        for f in range(F):
            k, t = (keys[f], tags[f]) if keep_touch else (keys[0], tags[0])
            _C.call("cnr_tsdf_touch", depths[f], W, H, fx, fy, cx, cy, T_dev[f], self.voxel_length, self.sdf_trunc, f, k, t, err)
            per_frame.append(torch.unique(k[k >= 0]))
        if keep_touch:
            self.touch_keys, self.touch_frames = keys, tags
        frame_of = torch.repeat_interleave(torch.arange(F, device=dev), torch.tensor([len(k) for k in per_frame], device=dev))
        self.units, self.frame_ofs, self.frame_idx, self.neighbours = tsdf_unit_tables(torch.cat(per_frame), frame_of)
        U = len(self.units)
        if int(err.item()):
            raise _C.CnrError("cnr_tsdf_touch: a depth sample lies more than 2^20 units from the origin, is not a number, or touches "
                              "three units on an axis")
        if U * TSDF_BLOCK_BYTES > self.max_block_bytes:
            raise _C.CnrError(f"TSDFVolume: the blocks of {U} units take {U * TSDF_BLOCK_BYTES} bytes, more than max_block_bytes = "
                              f"{self.max_block_bytes}")
        self.tsdf = torch.empty(U, TSDF_UNIT ** 3, device=dev, dtype=torch.float32)
        self.weight = torch.empty(U, TSDF_UNIT ** 3, device=dev, dtype=torch.float32)
        self.color = torch.empty(U, TSDF_UNIT ** 3, 3, device=dev, dtype=torch.float32)
        if U:
            T_CW = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(T_WC))).to(dev)
            _C.call("cnr_tsdf_integrate", self.units, U, self.frame_ofs, self.frame_idx, depths, colors, T_CW, F, W, H, fx, fy, cx, cy,
                    self.voxel_length, self.sdf_trunc, self.tsdf, self.weight, self.color)
        return self

    def extract_points(self):
        """-> (points (n,3), colors (n,3)) f64 device tensors in the order unit, voxel, axis"""
        from . import _C
        if self.units is None:
            raise ValueError("TSDFVolume: extract before integrate_frames")
        U, dev = len(self.units), self.device
        if U == 0:
            return torch.zeros(0, 3, device=dev, dtype=torch.float64), torch.zeros(0, 3, device=dev, dtype=torch.float64)
        ws = _C.workspace(_C.load().cnr_tsdf_extract_workspace_bytes(U), dev, "cnr_tsdf_extract")
        cnt = torch.zeros(1, device=dev, dtype=torch.int64)
        _C.call("cnr_tsdf_extract_count", self.tsdf, self.weight, self.neighbours, U, ws, cnt)
        n = int(cnt.item())
        points = torch.empty(n, 3, device=dev, dtype=torch.float64)
        colors = torch.empty(n, 3, device=dev, dtype=torch.float64)
        if n:
            _C.call("cnr_tsdf_extract_emit", self.units, self.tsdf, self.weight, self.color, self.neighbours, U, self.voxel_length,
                    ws, points, colors)
        return points, colors

    def extract_point_cloud(self):
        points, colors = self.extract_points()
        return PointCloud(points.float(), colors.float())

    @classmethod
    def from_blocks(cls, units, tsdf, weight, color, voxel_length, sdf_trunc, device=None, max_block_bytes=DEFAULT_TSDF_BLOCK_BYTES):
        """A volume of given blocks (a saved volume, or a synthetic one): units (U,) ascending distinct keys, tsdf (U,4096),
        weight (U,4096), color (U,4096,3); `neighbours` as tsdf_unit_tables fills it."""
        vol = cls(voxel_length, sdf_trunc, device=device, max_block_bytes=max_block_bytes)
        dev = vol.device
        units = torch.as_tensor(units).to(device=dev, dtype=torch.int64).contiguous()
        U = len(units)
        if units.dim() != 1 or (U and int(units.min()) < 0) or (U > 1 and not bool((units[1:] > units[:-1]).all())):
            raise ValueError("TSDFVolume.from_blocks: units (U,) are distinct keys of three biased 21-bit indices, ascending")
        if U * TSDF_BLOCK_BYTES > vol.max_block_bytes:
            from . import _C
            raise _C.CnrError(f"TSDFVolume: the blocks of {U} units take {U * TSDF_BLOCK_BYTES} bytes, more than max_block_bytes = "
                              f"{vol.max_block_bytes}")
        blocks = [torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous() for a in (tsdf, weight, color)]
        want = [(U, TSDF_UNIT ** 3), (U, TSDF_UNIT ** 3), (U, TSDF_UNIT ** 3, 3)]
        if [tuple(b.shape) for b in blocks] != want:
            raise ValueError(f"TSDFVolume.from_blocks: tsdf, weight, color of {U} units have the shapes {want}")
        vol.units, vol.neighbours = units, _unit_neighbours(units)
        vol.tsdf, vol.weight, vol.color = blocks
        return vol

    def extract_triangle_mesh_raw(self):
        """Marching cubes over the observed voxels (weight != 0), across units (csrc/tsdf_mesh.hip) ->
        (verts (V,3) f64, colors (V,3) f64 in [0, 1], normals (V,3) f64, faces (F,3) i32) device tensors, vertices in the order
        unit, voxel, axis and faces in the order unit, voxel, table; None when there is no vertex or no face.  Normals and
        right-hand face normals point to increasing tsdf (free space)."""
        from . import _C
        if self.units is None:
            raise ValueError("TSDFVolume: extract before integrate_frames")
        U, dev = len(self.units), self.device
        if U == 0:
            return None
        hood = tsdf_unit_neighbourhood(self.units)
        ws = _C.workspace(_C.load().cnr_tsdf_mesh_workspace_bytes(U), dev, "cnr_tsdf_mesh")
        cnt = torch.zeros(2, device=dev, dtype=torch.int64)
        _C.call("cnr_tsdf_mesh_count", self.tsdf, self.weight, hood, U, ws, cnt)
        V, F = (int(v) for v in cnt.tolist())
        if V == 0 or F == 0:
            return None
        if V >= 1 << 31:
            raise _C.CnrError(f"cnr_tsdf_mesh: {V} vertices, more than int32 faces can name")
        verts, colors, normals = (torch.empty(V, 3, device=dev, dtype=torch.float64) for _ in range(3))
        faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
        _C.call("cnr_tsdf_mesh_emit", self.units, self.tsdf, self.weight, self.color, hood, U, self.voxel_length, ws, verts, colors,
                normals, faces)
        return verts, colors, normals, faces

    def extract_triangle_mesh(self):
        """-> vis.Mesh (f64 vertices and normals, vertex colours clip(rint(255 c), 0, 255)), or None when the volume has no face"""
        from . import vis
        raw = self.extract_triangle_mesh_raw()
        if raw is None:
            return None
        verts, colors, normals, faces = (a.cpu().numpy() for a in raw)
        mesh = vis.Mesh(verts, faces, normals)
        mesh.visual.vertex_colors = np.clip(np.rint(255.0 * colors), 0, 255)
        return mesh


def _radius_cell_tables(points, radius):
    """The cell tables cnr_radius_count and cnr_hybrid_search take, for (n,3) f32 device points (n >= 1) and cells of edge
    radius: cnr_radius_cell_keys, a stable sort, the distinct cells and their starts -> (perm, sorted keys, cells, starts)"""
    from . import _C
    n, dev = len(points), points.device
    keys = torch.empty(n, device=dev, dtype=torch.int64)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    _C.call("cnr_radius_cell_keys", points, n, float(radius), keys, err)
    skeys, perm = torch.sort(keys, stable=True)
    cells, per_cell = torch.unique_consecutive(skeys, return_counts=True)
    if int(err.item()):
        raise _C.CnrError("cnr_radius_cell_keys: a point lies more than 2^20 cells from the origin, or is not a number")
    starts = torch.zeros(len(cells) + 1, dtype=torch.int64, device=dev)
    starts[1:] = torch.cumsum(per_cell, 0)
    return perm.contiguous(), skeys.contiguous(), cells.contiguous(), starts


def radius_neighbour_counts(points, radius):
    """(n,3) f32 device points -> (n,) int32: per point the points with squared distance < radius^2, itself included
    (cnr_radius_cell_keys, a sort, cnr_radius_count)"""
    from . import _C
    points = points.to(torch.float32).contiguous()
    n, dev = len(points), points.device
    if not radius > 0:
        raise ValueError("radius must be positive")
    if n == 0:
        return torch.zeros(0, device=dev, dtype=torch.int32)
    perm, skeys, cells, starts = _radius_cell_tables(points, radius)
    counts = torch.zeros(n, device=dev, dtype=torch.int32)
    _C.call("cnr_radius_count", points, n, perm, skeys, cells, starts, len(cells), float(radius), counts)
    return counts


HYBRID_MAX_NN = 128


def hybrid_search(points, radius, max_nn):
    """open3d's KDTreeSearchParamHybrid(radius, max_nn) for every point of (n,3) f32 device points against the cloud itself
    (cnr_hybrid_search): the points with fp64 squared distance < radius^2, the point itself included, by (distance, index)
    ascending, the first max_nn -> (idx (n,max_nn) int32 padded with -1, d2 (n,max_nn) f64 padded with 0, count (n,) int32)"""
    from . import _C
    points = points.to(torch.float32).contiguous()
    n, dev, max_nn = len(points), points.device, int(max_nn)
    if not radius > 0:
        raise ValueError("radius must be positive")
    if not 1 <= max_nn <= HYBRID_MAX_NN:
        raise ValueError(f"max_nn must lie in [1, {HYBRID_MAX_NN}]")
    idx = torch.empty(n, max_nn, device=dev, dtype=torch.int32)
    d2 = torch.empty(n, max_nn, device=dev, dtype=torch.float64)
    count = torch.empty(n, device=dev, dtype=torch.int32)
    if n:
        perm, skeys, cells, starts = _radius_cell_tables(points, radius)
        _C.call("cnr_hybrid_search", points, n, perm, skeys, cells, starts, len(cells), float(radius), max_nn, idx, d2, count)
    return idx, d2, count


def sequential_centroid(points):
    """the fp64 mean of (n,3) f32 device points, summed one after the other on the host (the reference point of the normals'
    orientation: one read-back of the cloud per estimate_normals) -> (3,) float64 numpy"""
    p = points.double().cpu().numpy()
    return np.cumsum(p, axis=0)[-1] / float(len(p))


def estimate_normals_device(points, radius, max_nn, centroid=None):
    """(n,3) f32 device points -> normals (n,3) f64 device tensor: hybrid_search(radius, max_nn), cnr_estimate_normals with the
    cloud's sequential_centroid (or `centroid`)"""
    from . import _C
    points = points.to(torch.float32).contiguous()
    n = len(points)
    normals = torch.empty(n, 3, device=points.device, dtype=torch.float64)
    if n:
        idx, _, count = hybrid_search(points, radius, max_nn)
        c = sequential_centroid(points) if centroid is None else np.asarray(centroid, np.float64).reshape(3)
        _C.call("cnr_estimate_normals", points, n, idx, count, int(max_nn), float(c[0]), float(c[1]), float(c[2]), normals)
    return normals


MIN_POINTS_AFTER_OUTLIER_REMOVAL = 100


def _fuse_instance_volume(inst_id, inst_info_list, frame_samples, intrinsic_open3d, voxel_size, depth_scale, max_depth, device,
                          max_block_bytes):
    """the instance's masked depth of every frame of inst_info_list integrated into one TSDFVolume(voxel_size, 4 voxel_size)
    -> (volume, number of frames)"""
    dev = _cuda_device(device)
    depths, images, poses = [], [], []
    for entry in inst_info_list:
        s = frame_samples[entry["frame"]]
        if s["frame_id"] != entry["frame"]:
            raise ValueError(f"frame {entry['frame']}: sample_dict holds frame {s['frame_id']} under that key")
        up = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=dev, dtype=dt)
        depths.append(tsdf_depth_image(up(s["depth"], torch.float32), up(s["obj_mask"], torch.int32), inst_id, depth_scale, max_depth))
        images.append(up(s["image"], torch.uint8))
        poses.append(np.asarray(s["T"], np.float64))
    if not depths:
        raise ValueError(f"instance {inst_id}: no frames")
    volume = TSDFVolume(voxel_size, 4 * voxel_size, device=dev, max_block_bytes=max_block_bytes)
    volume.integrate_frames(torch.stack(depths), torch.stack(images), intrinsic_open3d, np.stack(poses))
    return volume, len(depths)


def accumulate_pointcloud_tsdf(inst_id, inst_info_list, frame_samples, intrinsic_open3d, voxel_size=0.01, depth_scale=0.001,
                               max_depth=6.0, device=None, max_block_bytes=DEFAULT_TSDF_BLOCK_BYTES):
    """src/utils.py:212-247: the instance's depth of every frame of inst_info_list fused into a TSDF volume (voxel_size,
    sdf_trunc = 4 voxel_size, RGB8), its surface points, voxel_down_sample(voxel_size), remove_radius_outlier(100, 0.05) -- and
    the unfiltered cloud where fewer than 100 points survive that."""
    volume, n_frames = _fuse_instance_volume(inst_id, inst_info_list, frame_samples, intrinsic_open3d, voxel_size, depth_scale,
                                             max_depth, device, max_block_bytes)
    cloud = volume.extract_point_cloud()
    if len(cloud) == 0:
        raise ValueError(f"instance {inst_id}: the TSDF volume of its {n_frames} frames has no surface point")
    cloud = cloud.voxel_down_sample(voxel_size)
    kept, _ = cloud.remove_radius_outlier(nb_points=100, radius=0.05)
    if len(kept) < MIN_POINTS_AFTER_OUTLIER_REMOVAL:
        print("too few points left after outlier rejection")
        return cloud
    return kept


def accumulate_mesh_tsdf(inst_id, inst_info_list, frame_samples, intrinsic_open3d, voxel_size=0.01, depth_scale=0.001,
                         max_depth=6.0, device=None, max_block_bytes=DEFAULT_TSDF_BLOCK_BYTES):
    """The classical baseline: the volume of accumulate_pointcloud_tsdf (the same frames, the same fusion), and its triangle
    mesh (TSDFVolume.extract_triangle_mesh) -> vis.Mesh in world coordinates, coloured.  mesh.units = the volume's unit count."""
    volume, n_frames = _fuse_instance_volume(inst_id, inst_info_list, frame_samples, intrinsic_open3d, voxel_size, depth_scale,
                                             max_depth, device, max_block_bytes)
    mesh = volume.extract_triangle_mesh()
    if mesh is None:
        raise ValueError(f"instance {inst_id}: the TSDF volume of its {n_frames} frames has no surface triangle")
    mesh.units = len(volume.units)
    return mesh


def transform_pointcloud(cloud, T_rel):
    """(n,3) points -> R p + t for the (4,4) transform T_rel, (n,3) (src/utils.py:361-366)"""
    T = np.asarray(T_rel)
    return np.asarray(cloud) @ T[:3, :3].T + T[:3, 3]


MIN_BOX_EXTENT = 0.10       # a box is at least 10 cm along every edge (what the renderer samples)


def _host_points(cloud):
    return np.array(cloud.points if hasattr(cloud, "points") else cloud, dtype=np.float64).reshape(-1, 3)


def get_bound(inst_pcs):
    """src/utils.py:249-268: the oriented box of a cloud as a BoundingBox (R and center place the box in the world, extent >=
    10 cm), from metrics.oriented_bounds where the reference calls trimesh's.  None, after a message, when the cloud spans no
    volume (fewer than 4 points, or flat to rounding: where qhull refuses a 3-D hull)."""
    from . import metrics
    pts = _host_points(inst_pcs)
    spread = np.linalg.svd(pts - pts.mean(0), compute_uv=False) if len(pts) >= 4 else np.zeros(3)
    if not spread[2] > 1e-12 * max(spread[0], 1e-300):
        print("fail to get initial pose from instance point cloud")
        return None
    to_box, extents = metrics.oriented_bounds(pts)
    from_box = np.linalg.inv(to_box)
    box = BoundingBox()
    box.R, box.center = from_box[:3, :3], from_box[:3, 3]
    box.extent = np.maximum(np.asarray(extents, np.float64), MIN_BOX_EXTENT)
    return box


def get_obb(inst_info):
    """src/utils.py:270-284: inst_info['bbox3D'] = the box of inst_info['pcs'] in the frame of inst_info['T_obj'] with its
    scale taken out: centred on that frame's origin, so each extent is twice the larger of the two reaches along its axis, at
    least 10 cm.  T_obj's 3 x 3 part becomes that rotation times half the largest extent."""
    pose = inst_info["T_obj"]
    frame = np.array(pose, dtype=np.float64)
    frame[:3, :3] /= np.cbrt(np.linalg.det(frame[:3, :3]))
    local = transform_pointcloud(_host_points(inst_info["pcs"]), np.linalg.inv(frame))
    reach = np.maximum(local.max(axis=0), -local.min(axis=0))
    box = BoundingBox()
    box.R, box.center = frame[:3, :3], frame[:3, 3]
    box.extent = np.maximum(2.0 * reach, MIN_BOX_EXTENT)
    pose[:3, :3] = frame[:3, :3] * (box.extent.max() / 2.0)
    inst_info["bbox3D"] = box


def get_pose_from_pointcloud(inst_pcs, inst_id=None):
    """src/utils.py:286-296: (T_obj, bbox3D) of a cloud: its oriented box, and the similarity [R * max(extent) / 2 | center].
    A cloud without a 3-D hull raises a ValueError naming the instance (the reference fails on None.extent)."""
    box = get_bound(inst_pcs)
    if box is None:
        raise ValueError(f"instance {inst_id}: its point cloud has no 3-D convex hull, so no pose can be taken from it")
    T_obj = np.eye(4)
    T_obj[:3, :3] = box.R * (box.extent.max() / 2.0)
    T_obj[:3, 3] = box.center
    return T_obj, box


def get_possible_transform_from_bbox():
    """src/utils.py:298-320: the 24 proper rotations that map a box onto itself, as (4,4) transforms: for every ordered pair of
    axes (x, y), the four sign choices (+,+), (-,+), (+,-), (-,-), z = x cross y."""
    from itertools import permutations
    transform_list = []
    for ax, ay in permutations([0, 1, 2], 2):
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            x_axis, y_axis = sx * np.eye(3)[ax], sy * np.eye(3)[ay]
            transform = np.eye(4)
            transform[:3, :3] = np.vstack([x_axis, y_axis, np.cross(x_axis, y_axis)]).T
            transform_list.append(transform)
    return transform_list


# ---- ScanNet mask refinement (src/utils.py:561-727) ----------------------------------------------------------------------
# geometry_segmentation and refine_inst_data on the kernels of csrc/geoseg.hip; the point map and the normals
# on those of csrc/pointcloud.hip and csrc/fpfh.hip.  The reference's cv2 contour stage is restated on connected components
# (equality with cv2 and open3d is unverified).
GEOSEG_NORMAL_RADIUS, GEOSEG_NORMAL_MAX_NN = 0.1, 100
FILL_CHUNK_BYTES = 256 << 20          # what one cnr_fill_holes call's stack (masks, labels, flags) may take


class Segment():
    def __init__(self):
        self.points = None
        self.normals = None
        self.rgbs = None


def label_colormap(n_label=256):
    """imgviz.label_colormap(): the PASCAL-VOC colormap, (n_label, 3) uint8 -- bit b of (id >> 3 j) becomes bit 7 - j of
    channel b, for j = 0..7"""
    ids = np.arange(n_label, dtype=np.int64)
    cmap = np.zeros((n_label, 3), np.uint8)
    for j in range(8):
        for ch in range(3):
            cmap[:, ch] |= ((((ids >> (3 * j)) >> ch) & 1) << (7 - j)).astype(np.uint8)
    return cmap


def _device_mask(mask):
    if not torch.is_tensor(mask) or not mask.is_cuda:
        from . import _C
        raise _C.CnrError("a device tensor is expected; there is no CPU path")
    return (mask != 0).to(torch.uint8).contiguous()


def _raise_if_set(err, what):
    if int(err.item()):
        from . import _C
        raise _C.CnrError(f"{what}: a union/find loop ran out of its bound (the label array is corrupt)")


def connected_components(mask, connectivity=8, check=True):
    """(H,W) or (F,H,W) device mask (non-zero = set) -> int32 labels of the same shape (cnr_ccl): the smallest raster index
    v W + u, within its frame, of the pixel's 4- or 8-connected component, -1 outside the mask"""
    from . import _C
    m = _device_mask(mask)
    if m.dim() not in (2, 3):
        raise ValueError("mask (H,W) or (F,H,W)")
    F = 1 if m.dim() == 2 else m.shape[0]
    H, W = m.shape[-2:]
    labels = torch.empty(m.shape, device=m.device, dtype=torch.int32)
    if F == 0:
        return labels
    err = torch.zeros(1, device=m.device, dtype=torch.int32)
    _C.call("cnr_ccl", m, F, H, W, int(connectivity), labels, err)
    if check:
        _raise_if_set(err, "cnr_ccl")
    return labels


def label_counts(labels):
    """(H,W) or (F,H,W) int32 device labels -> int32 counts of the same shape: counts[f].ravel()[l] = pixels of frame f labelled l"""
    from . import _C
    labels = labels.contiguous()
    F = 1 if labels.dim() == 2 else labels.shape[0]
    counts = torch.empty(labels.shape, device=labels.device, dtype=torch.int32)
    if F:
        _C.call("cnr_label_counts", labels, F, labels.shape[-2], labels.shape[-1], counts)
    return counts


def _fill_holes_stack(labels, seg_ids, masks, K, H, W, dev):
    """cnr_fill_holes in chunks over K -> (K,H,W) uint8"""
    from . import _C
    lib = _C.load()
    filled = torch.empty(K, H, W, device=dev, dtype=torch.uint8)
    err = torch.zeros(1, device=dev, dtype=torch.int32)
    chunk = max(1, min(K, 65535, FILL_CHUNK_BYTES // (6 * H * W)))
    for k0 in range(0, K, chunk):
        k = min(chunk, K - k0)
        ws = _C.workspace(lib.cnr_fill_holes_workspace_bytes(k, H, W), dev, "cnr_fill_holes")
        _C.call("cnr_fill_holes", labels, seg_ids[k0:k0 + k] if seg_ids is not None else None,
                masks[k0:k0 + k] if masks is not None else None, k, H, W, ws, filled[k0:k0 + k], err)
    return filled, err


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes (default structure) of an (H,W) or (K,H,W) device mask -> bool tensor (cnr_fill_holes)"""
    m = _device_mask(mask)
    if m.dim() not in (2, 3):
        raise ValueError("mask (H,W) or (K,H,W)")
    stack = m.reshape((-1,) + tuple(m.shape[-2:]))
    filled, err = _fill_holes_stack(None, None, stack, stack.shape[0], m.shape[-2], m.shape[-1], m.device)
    _raise_if_set(err, "cnr_fill_holes")
    return filled.reshape(m.shape).bool()


def _geoseg_point_map(depth, intrinsic):
    """depth (H,W) f32 device -> (P (H,W,3) f32: the camera-frame point of every valid pixel, zero elsewhere; valid (H,W) bool)"""
    H, W = depth.shape
    dev = depth.device
    d_t = depth.t().contiguous()                               # the unprojection kernel walks (W,H) frames, u major
    cloud, counts = _unproject_frames([(torch.zeros(W, H, 3, dtype=torch.uint8, device=dev), d_t,
                                        torch.ones(W, H, dtype=torch.int32, device=dev), np.eye(4))], [1], intrinsic, dev,
                                      return_counts=True)
    valid = depth > 0
    if int(counts[0]) != int(valid.sum()):
        raise ValueError("geometry_segmentation: depth values beyond 8 m (or not finite); the loaders zero them")
    P_t = torch.zeros(W, H, 3, device=dev, dtype=torch.float32)
    P_t[valid.t()] = cloud.points_device
    return P_t.permute(1, 0, 2).contiguous(), valid


def _geoseg_points_normals(depth, intrinsic):
    """-> (P, N (H,W,3) f32: the normals of the valid pixels, estimated on them in raster order and negated where n_z > 0)"""
    P, valid = _geoseg_point_map(depth, intrinsic)
    N = torch.zeros(P.shape, device=P.device, dtype=torch.float32)
    if bool(valid.any()):
        n = estimate_normals_device(P[valid], GEOSEG_NORMAL_RADIUS, GEOSEG_NORMAL_MAX_NN)
        n = torch.where(n[:, 2:] > 0, -n, n)                   # src/utils.py:571
        N[valid] = n.to(torch.float32)
    return P, N


def geoseg_maps(P, N, depth):
    """cnr_geoseg_maps on device tensors -> (disc, conv) (H,W) uint8"""
    from . import _C
    H, W = depth.shape
    disc = torch.empty(H, W, device=depth.device, dtype=torch.uint8)
    conv = torch.empty(H, W, device=depth.device, dtype=torch.uint8)
    _C.call("cnr_geoseg_maps", P.contiguous(), N.contiguous(), depth.contiguous(), H, W, disc, conv)
    return disc, conv


def geoseg_edge_map(disc, conv, depth):
    """cnr_geoseg_edge_map -> (H,W) uint8, 1 = region pixel"""
    from . import _C
    H, W = depth.shape
    edge = torch.empty(H, W, device=depth.device, dtype=torch.uint8)
    _C.call("cnr_geoseg_edge_map", disc.contiguous(), conv.contiguous(), depth.contiguous(), H, W, edge)
    return edge


def geoseg_grow(P, depth, edge, labels, counts=None, min_area=0):
    """cnr_geoseg_grow -> the second label image (H,W) int32"""
    from . import _C
    H, W = depth.shape
    out = torch.empty(H, W, device=depth.device, dtype=torch.int32)
    _C.call("cnr_geoseg_grow", P.contiguous(), depth.contiguous(), edge.contiguous(), labels.contiguous(),
            counts.contiguous() if counts is not None else None, int(min_area), H, W, out)
    return out


def _segment_frame(depth, intrinsic, min_area, min_pixels, points_normals=None):
    """2.1 - 2.5 on one (H,W) f32 device depth frame -> dict(P, N, disc, conv, edge, labels, grown, seg_ids (K,) int32 device)"""
    P, N = points_normals if points_normals is not None else _geoseg_points_normals(depth, intrinsic)
    disc, conv = geoseg_maps(P, N, depth)
    edge = geoseg_edge_map(disc, conv, depth)
    err = torch.zeros(1, device=depth.device, dtype=torch.int32)
    from . import _C
    H, W = depth.shape
    labels = torch.empty(H, W, device=depth.device, dtype=torch.int32)
    _C.call("cnr_ccl", edge, 1, H, W, 8, labels, err)
    grown = geoseg_grow(P, depth, edge, labels, label_counts(labels), min_area)
    seg_ids = torch.nonzero(label_counts(grown).reshape(-1) >= int(min_pixels)).reshape(-1).to(torch.int32)
    _raise_if_set(err, "cnr_ccl")
    return dict(P=P, N=N, disc=disc, conv=conv, edge=edge, labels=labels, grown=grown, seg_ids=seg_ids)


def _as_device_depth(depth, device):
    dev = depth.device if torch.is_tensor(depth) and depth.is_cuda else _cuda_device(device)
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32))
    d = d.to(device=dev, dtype=torch.float32).contiguous()
    if d.dim() != 2 or d.shape[0] < 3 or d.shape[1] < 3:
        raise ValueError("depth (H,W) with H, W >= 3")
    return d


def geometry_segmentation(rgb, depth, intrinsic_open3d, min_area=500, min_pixels=500, device=None, normal_image=None):
    """src/utils.py:561-694 on the device: rgb (H,W,3) uint8, depth (H,W) f32 in metres with 0 = invalid ->
    (normal_image (H,W,3) f32, output (H,W,3) uint8 label colouring, segment_masks [(H,W) bool], segments [Segment]).
    Regions are the 8-connected components of the edge map with at least min_area pixels, grown onto the edge pixels; those with
    at least min_pixels pixels are the segments, in ascending label (= first pixel in raster order).  `normal_image`: normals to
    use in place of the estimated ones (the tests' hook)."""
    d = _as_device_depth(depth, device)
    dev = d.device
    H, W = d.shape
    rgb = np.asarray(rgb.cpu() if torch.is_tensor(rgb) else rgb)
    if rgb.shape != (H, W, 3):
        raise ValueError("rgb (H,W,3) of the depth's size")
    pn = None
    if normal_image is not None:
        pn = (_geoseg_point_map(d, intrinsic_open3d)[0],
              torch.from_numpy(np.ascontiguousarray(normal_image, dtype=np.float32)).to(dev))
    s = _segment_frame(d, intrinsic_open3d, min_area, min_pixels, pn)
    grown, seg_ids = s["grown"], s["seg_ids"]
    K = len(seg_ids)
    rank = torch.full((H * W + 1,), -1, device=dev, dtype=torch.int64)
    rank[seg_ids.long()] = torch.arange(K, device=dev)
    rank_img = rank[grown.long().clamp(min=-1)]                # -1 indexes the spare last entry, which stays -1
    cmap = torch.from_numpy(label_colormap()).to(dev)
    output = torch.where((rank_img >= 0)[..., None], cmap[rank_img.clamp(min=0) % 256], torch.zeros(3, dtype=torch.uint8, device=dev))
    rank_np, P_np, N_np = rank_img.cpu().numpy(), s["P"].cpu().numpy(), s["N"].cpu().numpy()
    segment_masks, segments = [], []
    for k in range(K):
        m = rank_np == k
        seg = Segment()
        seg.points, seg.normals, seg.rgbs = P_np[m], N_np[m], rgb[m]
        segment_masks.append(m)
        segments.append(seg)
    return N_np, output.cpu().numpy(), segment_masks, segments


def _vote(inst, filled, threshold):
    """inst (H,W) int32 device, filled (K,H,W) uint8 device -> refined (H,W) int32 device (cnr_refine_vote, cnr_refine_apply)"""
    from . import _C
    H, W = inst.shape
    dev, K = inst.device, filled.shape[0]
    ids = torch.unique(inst)
    ids = ids[(ids != 0) & (ids != -1)].to(torch.int32).contiguous()
    O = len(ids)
    refined = torch.zeros(H, W, device=dev, dtype=torch.int32)
    if O == 0 or K == 0:
        return refined                                         # "this frame has no foreground objects"
    counts = torch.empty(K, O + 1, device=dev, dtype=torch.int32)
    chosen = torch.empty(K, device=dev, dtype=torch.int32)
    _C.call("cnr_refine_vote", filled, inst, ids, K, O, H, W, counts)
    _C.call("cnr_refine_apply", filled, counts, ids, K, O, H, W, float(threshold), chosen, refined)
    return refined


def _inst_to_device(inst_data, dev):
    inst = inst_data if torch.is_tensor(inst_data) else torch.from_numpy(np.ascontiguousarray(inst_data))
    if inst.dim() != 2 or inst.dtype.is_floating_point:
        raise ValueError("inst_data: an (H,W) integer array")
    wide = inst.to(torch.int64)
    if inst.numel() and (int(wide.min()) < -(1 << 31) or int(wide.max()) >= (1 << 31)):
        raise ValueError("inst_data: ids outside int32")
    return wide.to(device=dev, dtype=torch.int32).contiguous()


def refine_inst_data(inst_data, segment_masks, threshold=0.7, device=None):
    """src/utils.py:696-721 on the device: every segment mask with its holes filled votes for the object id (the distinct values
    of inst_data without 0 and -1) that covers the largest share of it; a share > threshold assigns the id to the filled mask,
    later segments over earlier ones -> (H,W) array of inst_data's dtype"""
    dev = inst_data.device if torch.is_tensor(inst_data) and inst_data.is_cuda else _cuda_device(device)
    inst = _inst_to_device(inst_data, dev)
    H, W = inst.shape
    out_dtype = inst_data.dtype
    K = len(segment_masks)
    if K:
        masks = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(m) != 0 for m in segment_masks]), dtype=np.uint8)).to(dev)
        if masks.shape[1:] != (H, W):
            raise ValueError("segment masks of inst_data's size")
        filled, err = _fill_holes_stack(None, None, masks, K, H, W, dev)
        refined = _vote(inst, filled, threshold)
        _raise_if_set(err, "cnr_fill_holes")
    else:
        refined = torch.zeros(H, W, device=dev, dtype=torch.int32)
    if torch.is_tensor(inst_data):
        return refined.to(out_dtype)
    return refined.cpu().numpy().astype(out_dtype)


def refine_frame(depth, inst, intrinsic, min_area=500, min_pixels=500, threshold=0.7):
    """geometry_segmentation and refine_inst_data of one frame without leaving the device (the loaders' path): depth (H,W) f32,
    inst (H,W) int32 device tensors -> refined (H,W) int32 device tensor"""
    s = _segment_frame(depth, intrinsic, min_area, min_pixels)
    K = len(s["seg_ids"])
    H, W = depth.shape
    if K == 0:
        return torch.zeros(H, W, device=depth.device, dtype=torch.int32)
    filled, err = _fill_holes_stack(s["grown"], s["seg_ids"].contiguous(), None, K, H, W, depth.device)
    refined = _vote(inst.contiguous(), filled, threshold)
    _raise_if_set(err, "cnr_fill_holes")
    return refined
