"""The reference's dataset loaders (src/dataset.py): ``get_dataset(cfg)`` -> ``Replica`` or ``ScanNet`` with the same attributes,
``inst_dict`` and ``sample_dict`` -- without cv2, open3d, torchvision or TEASER++.

Images are decoded with PIL in a thread pool, uploaded in pinned batches and parsed on the device (csrc/frames.hip): one
instance table per label frame (ids in np.unique order, pixel count, bounds, class range), then one pass that writes the frame
arrays in the reference's (W, H) layout.  The per-instance decisions are host logic on the small table, in the reference's
order and dtypes, quirks included.  The loaders read the cached registration result
``<dataset_dir>/inst_dict.pkl`` (``registration.load_registration_result``) with a restricted unpickler; without one,
``get_dataset(cfg, register=True)`` runs category registration for Replica (category_registration.py), and
``get_dataset(cfg, register=True, tsdf=True)`` for ScanNet sequences.  A ScanNet frame without a refined
mask is refined on request, ``get_dataset(cfg, refine=True)``: geometry segmentation and the overlap vote on the device
(utils.refine_frame, csrc/geoseg.hip), written to ``instance-refined/`` and ``inst_to_cls/`` as the reference does."""
import glob
import io
import os
import pickle
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _C
from .utils import BoundingBox

ID_BOUND = 65537            # ids 0 .. 65536: ScanNet's raw uint16 ids shifted by +1
NSTAT = 7                   # include/cnr_hip.h CNR_FRAME_NSTAT: count, row min/max, column min/max, class min/max
BATCH = 16                  # frames per upload
DECODE_WORKERS = 16


def get_dataset(cfg, register=False, tsdf=False, refine=False, pretrain=None, rays_per_step=None):
    """register=True: a Replica dataset without a usable cache runs category registration (category_registration.
    register_dataset) and writes <dataset_dir>/inst_dict.pkl; the default raises NotImplementedError there, as before.
    A ScanNet dataset does so only with tsdf=True as well (its background cloud is a TSDF fusion).
    refine=True: a ScanNet frame that wants a refined mask (use_refined_mask) and has none on disk gets one computed and written
    (src/dataset.py:358-366); the default raises NotImplementedError there, as before.
    pretrain=ITERS: with registration.load_pretrained false, registration trains the per-object fields it probes for ITERS steps
    of rays_per_step rays (default cfg.n_per_optim) instead of raising (object_fields.ObjectFieldTrainer)."""
    if cfg.dataset_format == "Replica":
        return Replica(cfg, register=register, pretrain=pretrain, rays_per_step=rays_per_step)
    if cfg.dataset_format == "ScanNet":
        return ScanNet(cfg, register=register, tsdf=tsdf, refine=refine, pretrain=pretrain, rays_per_step=rays_per_step)
    raise ValueError("Dataset format {} not found".format(cfg.dataset_format))


class PinholeIntrinsics:
    """What the reference keeps as open3d.camera.PinholeCameraIntrinsic (width, height, fx, fy, cx, cy)."""

    def __init__(self, width, height, fx, fy, cx, cy):
        self.width, self.height, self.fx, self.fy, self.cx, self.cy = width, height, fx, fy, cx, cy

    @property
    def intrinsic_matrix(self):
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])


# ---- registration cache ------------------------------------------------------------------------------------------------
def _tensor_from_bytes(b):
    return torch.load(io.BytesIO(b), weights_only=True)


def _allowed_globals():
    import collections
    import torch._utils
    try:
        from numpy._core import multiarray
    except ImportError:                                  # numpy < 2
        from numpy.core import multiarray
    allowed = {("utils", "BoundingBox"): BoundingBox,
               ("torch.storage", "_load_from_bytes"): _tensor_from_bytes,
               ("torch._utils", "_rebuild_tensor_v2"): torch._utils._rebuild_tensor_v2,
               ("collections", "OrderedDict"): collections.OrderedDict,
               ("numpy", "ndarray"): np.ndarray, ("numpy", "dtype"): np.dtype}
    for mod in ("numpy.core.multiarray", "numpy._core.multiarray"):
        allowed[(mod, "_reconstruct")] = multiarray._reconstruct
        allowed[(mod, "scalar")] = multiarray.scalar
    return allowed


class RegistrationUnpickler(pickle.Unpickler):
    """Loads the reference's inst_dict.pkl: dicts, lists, numpy arrays and scalars, torch tensors (rebuilt through
    torch.load(weights_only=True)) and utils.BoundingBox (this package's).  Any other global is refused."""

    _allowed = None

    def find_class(self, module, name):
        if RegistrationUnpickler._allowed is None:
            RegistrationUnpickler._allowed = _allowed_globals()
        try:
            return RegistrationUnpickler._allowed[(module, name)]
        except KeyError:
            raise pickle.UnpicklingError(f"inst_dict.pkl: global {module}.{name} is not allowed") from None


def load_registration_result(path):
    with open(path, "rb") as f:
        return RegistrationUnpickler(f).load()


def _has_cache(root_dir, cfg):
    return bool(getattr(cfg, "load_registration_result", False)) and os.path.exists(os.path.join(root_dir, "inst_dict.pkl"))


def _load_inst_dict(dataset, cfg):
    register = getattr(dataset, "register", False)
    pre = {}                   # (only when asked for: a registration without pretrain is called exactly as before)
    if getattr(dataset, "pretrain", None) is not None:
        pre = dict(pretrain=dataset.pretrain, rays_per_step=getattr(dataset, "rays_per_step", None))
    result_file = os.path.join(dataset.root_dir, "inst_dict.pkl")
    if _has_cache(dataset.root_dir, cfg):
        dataset.inst_dict = load_registration_result(result_file)
        return
    if register and dataset.name == "replica":
        from . import category_registration
        category_registration.register_dataset(dataset, cfg, **pre)
        return
    if register and getattr(dataset, "tsdf", False):
        from . import category_registration
        category_registration.register_dataset(dataset, cfg, tsdf=True, **pre)
        return
    if dataset.name == "replica":
        raise NotImplementedError(
            f"{result_file}: no cached registration result (registration.load_registration_result = "
            f"{getattr(cfg, 'load_registration_result', None)}).  Category-level registration (get_all_poses, "
            "get_uncertainty_fields, align_poses) runs only on request: get_dataset(cfg, register=True)")
    raise NotImplementedError(
        f"{result_file}: no cached registration result (registration.load_registration_result = "
        f"{getattr(cfg, 'load_registration_result', None)}).  Category-level registration of ScanNet sequences (open3d's TSDF "
        "integration and geometry_segmentation, align_poses with TEASER++) runs only on request and only from refined masks "
        "on disk: get_dataset(cfg, register=True, tsdf=True)")


# ---- decoding ----------------------------------------------------------------------------------------------------------
def _read_png16(path):
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype != np.uint16:
        if a.min() < 0 or a.max() > 65535:
            raise ValueError(f"{path}: values outside uint16")
        a = a.astype(np.uint16)
    return a


def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def _pool():
    return ThreadPoolExecutor(max_workers=min(DECODE_WORKERS, os.cpu_count() or 1))


def _pinned(arrays):
    t = torch.from_numpy(np.stack(arrays))
    return t.pin_memory()


# ---- device kernels ----------------------------------------------------------------------------------------------------
class FrameTable:
    """The instance table of F label frames (cnr_frame_instances_count / _emit): offsets (F+1,), ids (N,), stats (N, 7)
    on the host, and what cnr_frame_finish needs on the device."""

    def __init__(self, inst, cls=None, edge=0, id_shift=0):
        F, Hs, Ws = inst.shape
        self.inst, self.label_i32, self.edge, self.id_shift = inst, int(inst.dtype == torch.int32), edge, id_shift
        if inst.dtype not in (torch.int32, torch.uint16) or (cls is not None and cls.dtype != inst.dtype):
            raise TypeError("label frames are uint16 or int32, instance and class maps alike")
        self.F, self.H, self.W = F, Hs - 2 * edge, Ws - 2 * edge
        dev = inst.device
        self.workspace = _C.workspace(_C.load().cnr_frame_instances_workspace_bytes(F, ID_BOUND), dev, "cnr_frame_instances")
        self.offsets_dev = torch.empty(F + 1, dtype=torch.int64, device=dev)
        _C.call("cnr_frame_instances_count", inst, self.label_i32, F, self.H, self.W, edge, id_shift, ID_BOUND, self.workspace,
                self.offsets_dev)
        self.offsets = self.offsets_dev.cpu().numpy()
        N = int(self.offsets[-1])
        ids = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        stats = torch.empty(max(N, 1), NSTAT, dtype=torch.int32, device=dev)
        _C.call("cnr_frame_instances_emit", inst, cls, self.label_i32, F, self.H, self.W, edge, id_shift, ID_BOUND,
                self.workspace, self.offsets_dev, ids, stats)
        self.ids, self.stats = ids[:N].cpu().numpy(), stats[:N].cpu().numpy()

    def frame(self, f):
        a, b = self.offsets[f], self.offsets[f + 1]
        return self.ids[a:b], self.stats[a:b]

    def finish(self, keep, depth, rgb, edge, depth_scale, max_depth):
        """keep (N,) bool -> (obj_mask (F,W,H) i32, depth (F,W,H) f32, image (F,W,H,3) u8) on the device"""
        dev = self.inst.device
        keep_t = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1)).to(dev)
        if keep_t.numel() == 0:
            keep_t = torch.zeros(1, dtype=torch.uint8, device=dev)
        F, H, W = self.F, self.H, self.W
        obj = torch.empty(F, W, H, dtype=torch.int32, device=dev)
        dep = torch.empty(F, W, H, dtype=torch.float32, device=dev)
        img = torch.empty(F, W, H, 3, dtype=torch.uint8, device=dev)
        _C.call("cnr_frame_finish", self.inst, self.label_i32, self.edge, depth, rgb, F, H, W, edge, self.id_shift, ID_BOUND,
                self.workspace, self.offsets_dev, keep_t, float(depth_scale), float(max_depth), obj, dep, img)
        return obj, dep, img


def resize_linear(src, dh, dw):
    """cv2.resize(frame, (dw, dh), interpolation=INTER_LINEAR) on (F, sh, sw, 3) uint8 device frames"""
    F, sh, sw, _ = src.shape
    out = torch.empty(F, dh, dw, 3, dtype=torch.uint8, device=src.device)
    _C.call("cnr_resize_linear_u8c3", src, F, sh, sw, out, dh, dw)
    return out


def resize_nearest(src, dh, dw):
    """cv2.resize(frame, (dw, dh), interpolation=INTER_NEAREST) on (F, sh, sw) uint16 / int32 device frames"""
    F, sh, sw = src.shape
    out = torch.empty(F, dh, dw, dtype=src.dtype, device=src.device)
    _C.call("cnr_resize_nearest", src, src.element_size(), F, sh, sw, out, dh, dw)
    return out


def _add_frame_info(inst_dict, sem_cls, inst_id, frame, bbox):
    if sem_cls not in inst_dict.keys():
        inst_dict[sem_cls] = {}
    if inst_id not in inst_dict[sem_cls].keys():
        inst_dict[sem_cls][inst_id] = {"frame_info": [{"frame": frame, "bbox": bbox}]}
    else:
        inst_dict[sem_cls][inst_id]["frame_info"].append({"frame": frame, "bbox": bbox})


def _add_background(inst_dict, frame, W, H):
    if frame == 0:
        inst_dict[0] = {"frame_info": []}
    inst_dict[0]["frame_info"].append({"frame": frame, "bbox": torch.from_numpy(np.array([0, W, 0, H]))})


def _bbox_of_mask(r0, r1, c0, c1, scale, W, H):
    """get_bbox2d (src/utils.py:53-67) from a mask's bounds: the bounding rectangle of its contours is its bounding box"""
    from .utils import enlarge_bbox
    x, y, w, h = int(c0), int(r0), int(c1 - c0 + 1), int(r1 - r0 + 1)
    return enlarge_bbox([x, y, x + w, y + h], scale=scale, w=W, h=H)


class _Base:
    def _camera(self, cfg):
        self.W, self.H = cfg.W, cfg.H
        self.fx, self.fy, self.cx, self.cy = cfg.fx, cfg.fy, cfg.cx, cfg.cy
        self.edge = cfg.mw
        self.intrinsic_open3d = PinholeIntrinsics(self.W, self.H, self.fx, self.fy, self.cx, self.cy)
        self.K = np.eye(3)
        self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2] = self.fx, self.fy, self.cx, self.cy

    def _parse_device(self):
        return torch.device(self.device if torch.device(self.device).type == "cuda" else "cuda")

    def __len__(self):
        return self.n_img

    def __getitem__(self, idx):
        return self.sample_dict[idx]


class Replica(_Base):
    def __init__(self, cfg, register=False, pretrain=None, rays_per_step=None):
        self.name = "replica"
        self.register, self.pretrain, self.rays_per_step = register, pretrain, rays_per_step
        self.device = cfg.data_device
        self.root_dir = cfg.dataset_dir
        self.Twc = np.loadtxt(os.path.join(self.root_dir, "traj_w_c.txt"), delimiter=" ").reshape([-1, 4, 4])
        self.depth_scale, self.max_depth = cfg.depth_scale, cfg.max_depth
        self._camera(cfg)
        # the reference's lists (src/dataset.py:55-57)
        self.background_cls_list = [5, 12, 30, 31, 40, 60, 92, 93, 95, 97, 98, 79]
        self.bbox_scale = 0.2
        self.n_img = len(os.listdir(os.path.join(self.root_dir, "depth")))
        self.get_all_frames()
        _load_inst_dict(self, cfg)

    def _decode(self, idx):
        d = lambda sub, stem: os.path.join(self.root_dir, sub, stem + "_" + str(idx) + ".png")
        return (_read_rgb(d("rgb", "rgb")), _read_png16(d("depth", "depth")),
                _read_png16(d("semantic_instance", "semantic_instance")), _read_png16(d("semantic_class", "semantic_class")))

    def get_all_frames(self):
        self.inst_dict, self.sample_dict = {}, {}
        dev = self._parse_device()
        with _pool() as pool:
            for b0 in range(0, self.n_img, BATCH):
                idxs = list(range(b0, min(b0 + BATCH, self.n_img)))
                frames = list(pool.map(self._decode, idxs))
                rgb, depth, inst, obj = [_pinned([fr[k] for fr in frames]).to(dev, non_blocking=True) for k in range(4)]
                table = FrameTable(inst, obj)
                keep = np.zeros(len(table.ids), dtype=bool)
                for f, idx in enumerate(idxs):
                    keep[table.offsets[f]:table.offsets[f + 1]] = self._frame_instances(idx, *table.frame(f), table.W, table.H)
                    _add_background(self.inst_dict, idx, table.W, table.H)
                obj_mask, dep, img = [t.cpu().numpy() for t in table.finish(keep, depth, rgb, 0, self.depth_scale, self.max_depth)]
                for f, idx in enumerate(idxs):
                    self.sample_dict[idx] = {"image": img[f], "depth": dep[f], "obj_mask": obj_mask[f], "T": self.Twc[idx],
                                             "frame_id": idx}

    def _frame_instances(self, idx, ids, stats, W, H):
        """src/dataset.py:117-156 on one frame's table -> keep (n,) bool; fills inst_dict"""
        keep = np.zeros(len(ids), dtype=bool)
        cand = []
        for k in range(len(ids)):
            inst_id, kmin, kmax = np.int32(ids[k]), stats[k, 5], stats[k, 6]
            assert kmin == kmax                                  # sem_cls.shape[0] == 1
            sem_cls = np.int32(kmin)
            if sem_cls in self.background_cls_list:
                continue
            cand.append((k, inst_id + 1000 if sem_cls == 0 and inst_id != 0 else sem_cls, inst_id))
        if not cand:
            return keep
        # get_bbox2d_batch on (n, W, H) masks, unpacked as the reference does: x extent [cmins, cmaxs), y extent [rmins, rmaxs)
        st = torch.from_numpy(stats[[c[0] for c in cand]].astype(np.int64))
        rmins, rmaxs, cmins, cmaxs = st[:, 1], st[:, 2] + 1, st[:, 3], st[:, 4] + 1
        w, h = rmaxs - rmins, cmaxs - cmins
        margin_x = (0.5 * self.bbox_scale * (rmaxs - rmins)).to(torch.int64)     # float32 as the reference's tensors give
        margin_y = (0.5 * self.bbox_scale * (cmaxs - cmins)).to(torch.int64)
        for i, (k, sem_cls, inst_id) in enumerate(cand):
            if w[i] <= 10 or h[i] <= 10:
                continue
            mx, my = int(margin_x[i]), int(margin_y[i])
            # enlarge_bbox([rmins, cmins, rmaxs, cmaxs], w=H, h=W); stored as [e[1], e[3], e[0], e[2]]
            e0 = min(max(int(rmins[i]) - mx, 0), H - 1)
            e2 = min(max(int(rmaxs[i]) + mx, 0), H - 1)
            e1 = min(max(int(cmins[i]) - my, 0), W - 1)
            e3 = min(max(int(cmaxs[i]) + my, 0), W - 1)
            keep[k] = True
            _add_frame_info(self.inst_dict, sem_cls, inst_id, idx, torch.from_numpy(np.array([e1, e3, e0, e2])))
        return keep


def _sorted_by_stem(pattern):
    return sorted(glob.glob(pattern), key=lambda x: int(os.path.basename(x)[:-4]))


class ScanNet(_Base):
    def __init__(self, cfg, register=False, tsdf=False, refine=False, pretrain=None, rays_per_step=None):
        self.name = "scannet"
        self.register, self.tsdf, self.refine = register, tsdf, refine
        self.pretrain, self.rays_per_step = pretrain, rays_per_step
        # the objects' clouds are gathered frame by frame (src/dataset.py:385-400) only when registration is going to run
        self._accumulate = bool(register and tsdf) and not _has_cache(cfg.dataset_dir, cfg)
        self._frame_objects = {}
        self.device = cfg.data_device
        self.root_dir = cfg.dataset_dir
        j = lambda *p: os.path.join(self.root_dir, *p)
        self.color_paths = _sorted_by_stem(j("color", "*.jpg"))
        self.depth_paths = _sorted_by_stem(j("depth", "*.png"))
        self.raw_inst_paths = _sorted_by_stem(j("instance-filt", "*.png"))
        self.raw_sem_paths = _sorted_by_stem(j("label-filt", "*.png"))
        self.use_refined_mask = cfg.use_refined_mask
        self.load_refined_mask = cfg.load_refined_mask
        if self.load_refined_mask:
            self.inst_paths = _sorted_by_stem(j("instance-refined", "*.npy"))
            self.sem_paths = _sorted_by_stem(j("inst_to_cls", "*.pkl"))
        else:
            self.inst_paths, self.sem_paths = self.raw_inst_paths, self.raw_sem_paths
        self.load_poses(j("pose"))
        self.n_img = len(self.color_paths)
        self.max_depth, self.depth_scale = cfg.max_depth, cfg.depth_scale
        self._camera(cfg)
        # from scannetv2-labels.combined.tsv (src/dataset.py:230-232)
        self.background_cls_list = [-1, 0, 1, 3, 16, 41, 232, 21, 161, 128, 21]
        self.bbox_scale = 0.2
        self.inst_dict = {}
        self.get_all_frames()
        _load_inst_dict(self, cfg)

    def load_poses(self, path):
        self.poses = []
        for pose_path in _sorted_by_stem(os.path.join(path, "*.txt")):
            with open(pose_path) as f:
                rows = [list(map(float, line.split(" "))) for line in f.readlines()]
            self.poses.append(np.array(rows).reshape(4, 4))

    def _refined(self, index):
        inst_path = self.inst_paths[index] if len(self.inst_paths) > index else ""
        sem_path = self.sem_paths[index] if len(self.sem_paths) > index else ""
        if self.refine and self.load_refined_mask:
            # by name, where the computed masks are written: the reference's sorted lists pair frame k with the k-th file, which
            # shifts every later frame when one in the middle is missing
            stem = os.path.basename(self.raw_inst_paths[index])[:-4]
            inst_path = os.path.join(self.root_dir, "instance-refined", stem + ".npy")
            sem_path = os.path.join(self.root_dir, "inst_to_cls", stem + ".pkl")
        if self.load_refined_mask and os.path.exists(inst_path) and os.path.exists(sem_path):
            return inst_path, sem_path
        if self.use_refined_mask and not self.refine:
            raise NotImplementedError(f"frame {index}: no refined mask; refining ScanNet's raw masks (open3d "
                                      "geometry_segmentation, src/dataset.py:359-366) is not part of this package")
        return None

    def _wants_refinement(self, index):
        """a frame read from the raw labels that gets its refined mask computed and written (refine=True)"""
        return bool(self.use_refined_mask and self.refine) and self._refined(index) is None

    def _decode(self, index):
        rgb = _read_rgb(self.color_paths[index])
        depth = _read_png16(self.depth_paths[index])
        ref = self._refined(index)
        if ref is not None:
            inst = np.load(ref[0])
            if inst.size and (inst.min() < 0 or inst.max() >= ID_BOUND):
                raise ValueError(f"{ref[0]}: instance ids outside [0, {ID_BOUND})")
            with open(ref[1], "rb") as f:
                inst_to_cls = pickle.load(f)
            return rgb, depth, inst.astype(np.int32), None, inst_to_cls, False
        return (rgb, depth, _read_png16(self.raw_inst_paths[index]), _read_png16(self.raw_sem_paths[index]), None,
                self._wants_refinement(index))

    def get_all_frames(self):
        self.inst_dict, self.sample_dict = {}, {}
        dev = self._parse_device()
        valid = [i for i in range(self.n_img) if not np.any(np.isinf(self.poses[i]))]   # src/dataset.py:292-297
        reduced = {index: k for k, index in enumerate(valid)}
        e = self.edge
        with _pool() as pool:
            b0 = 0
            while b0 < len(valid):
                # a batch holds frames of one label kind (refined or raw) and one set of image sizes
                frames = list(pool.map(self._decode, valid[b0:b0 + BATCH]))
                n = 1
                key = lambda fr: (fr[4] is None, fr[5], fr[0].shape, fr[1].shape, fr[2].shape)
                while n < len(frames) and key(frames[n]) == key(frames[0]):
                    n += 1
                idxs, frames = valid[b0:b0 + n], frames[:n]
                b0 += n
                self._parse_batch(idxs, frames, reduced, dev, e)
        self.n_img = len(valid)                                  # n_img -= the frames skipped

    def _parse_batch(self, idxs, frames, reduced, dev, e):
        rgb = _pinned([fr[0] for fr in frames]).to(dev, non_blocking=True)
        depth = _pinned([fr[1] for fr in frames]).to(dev, non_blocking=True)
        Hd, Wd = depth.shape[1:]
        if rgb.shape[1:3] != (Hd, Wd):
            rgb = resize_linear(rgb, Hd, Wd)                     # src/dataset.py:304
        if frames[0][5]:
            frames = self._refine_batch(idxs, frames, depth, rgb, dev, e)
        refined = frames[0][4] is not None
        if refined:
            table, shift, label_edge = FrameTable(_pinned([fr[2] for fr in frames]).to(dev, non_blocking=True)), 0, 0
        else:
            table, shift, label_edge = self._raw_label_table(frames, dev, Hd, Wd, e), 1, e
        W, H = Wd - 2 * e, Hd - 2 * e
        if (table.H, table.W) != (H, W):
            raise ValueError(f"label frames are {table.H} x {table.W} after the crop, depth {H} x {W}")
        keep = np.zeros(len(table.ids), dtype=bool)
        for f, index in enumerate(idxs):
            ids, stats = table.frame(f)
            keep[table.offsets[f]:table.offsets[f + 1]] = self._frame_instances(reduced[index], ids, stats, frames[f][4], W, H)
            _add_background(self.inst_dict, reduced[index], W, H)
        obj_mask, dep, img = [t.cpu().numpy() for t in table.finish(keep, depth, rgb, e, self.depth_scale, self.max_depth)]
        for f, index in enumerate(idxs):
            r = reduced[index]
            self.sample_dict[r] = {"image": img[f], "depth": dep[f], "obj_mask": obj_mask[f], "T": self.poses[index], "frame_id": r}
            if self._accumulate:
                self._accumulate_objects(r, dev)

    def _raw_label_table(self, frames, dev, Hd, Wd, e):
        """the raw path's instance table (src/dataset.py:327-338): nearest resize to the depth's size, edge crop, ids + 1"""
        inst = _pinned([fr[2] for fr in frames]).to(dev, non_blocking=True)
        sem = _pinned([fr[3] for fr in frames]).to(dev, non_blocking=True)
        if inst.shape[1:] != (Hd, Wd):
            inst = resize_nearest(inst, Hd, Wd)                  # src/dataset.py:330-332
        if sem.shape[1:] != (Hd, Wd):
            sem = resize_nearest(sem, Hd, Wd)
        return FrameTable(inst, sem, edge=e, id_shift=1)

    def _refine_batch(self, idxs, frames, depth, rgb, dev, e):
        """src/dataset.py:327-366 for frames without a refined mask: the raw instance map (background classes -> 0), geometry
        segmentation and the vote on the frame the loader hands on (cropped, metres, max_depth), instance-refined/<n>.npy and
        inst_to_cls/<n>.pkl written -> the frames as refined frames"""
        from .utils import refine_frame
        Hd, Wd = depth.shape[1:]
        table = self._raw_label_table(frames, dev, Hd, Wd, e)
        keep = np.zeros(len(table.ids), dtype=bool)
        maps = []
        for f in range(len(idxs)):
            ids, stats = table.frame(f)
            inst_to_cls = {0: 0}
            for k in range(len(ids)):
                assert stats[k, 5] == stats[k, 6]             # sem_cls.shape[0] == 1
                sem_cls = np.uint16(stats[k, 5])
                if sem_cls in self.background_cls_list:
                    continue
                keep[table.offsets[f] + k] = True
                inst_to_cls[np.int32(ids[k])] = sem_cls
            maps.append(inst_to_cls)
        obj, dep, _ = table.finish(keep, depth, rgb, e, self.depth_scale, self.max_depth)       # (F,W,H): the reference's layout
        for sub in ("instance-refined", "inst_to_cls"):
            os.makedirs(os.path.join(self.root_dir, sub), exist_ok=True)
        out = []
        for f, index in enumerate(idxs):
            refined = refine_frame(dep[f].t().contiguous(), obj[f].t().contiguous(), self.intrinsic_open3d).cpu().numpy()
            stem = os.path.basename(self.raw_inst_paths[index])[:-4]
            np.save(os.path.join(self.root_dir, "instance-refined", stem + ".npy"), refined)
            with open(os.path.join(self.root_dir, "inst_to_cls", stem + ".pkl"), "wb") as fh:
                pickle.dump(maps[f], fh)
            out.append((frames[f][0], frames[f][1], refined, None, maps[f], False))
        return out

    def _accumulate_objects(self, frame, dev):
        """src/dataset.py:385-400: every kept object's pixels of this frame, unprojected, added to its 'pcs'"""
        from .utils import PointCloud, _unproject_frames
        objects = self._frame_objects.pop(frame, [])
        if not objects:
            return
        s = self.sample_dict[frame]
        # one upload of the frame and one read-back for all its objects
        entry = (torch.zeros(s["image"].shape, dtype=torch.uint8, device=dev), torch.from_numpy(s["depth"]).to(dev),
                 torch.from_numpy(s["obj_mask"]).to(dev), s["T"])
        cloud, counts = _unproject_frames([entry] * len(objects), [int(o) for _, o in objects], self.intrinsic_open3d, dev,
                                          return_counts=True)
        at = 0
        for (sem_cls, obj_id), n in zip(objects, counts):
            part = PointCloud(cloud.points_device[at:at + int(n)])
            at += int(n)
            inst = self.inst_dict[sem_cls][obj_id]
            if "pcs" not in inst:
                inst["pcs"] = part
            else:
                inst["pcs"] += part

    def _frame_instances(self, frame, ids, stats, inst_to_cls, W, H):
        """src/dataset.py:339-383 on one frame's table -> keep (n,) bool; fills inst_dict"""
        keep = np.zeros(len(ids), dtype=bool)
        rows = list(range(len(ids)))
        union = None                                          # bounds of the background-class pixels: id 0 after :349
        if inst_to_cls is None:
            inst_to_cls = {0: 0}
            rows = []
            for k in range(len(ids)):
                assert stats[k, 5] == stats[k, 6]             # sem_cls.shape[0] == 1
                sem_cls = np.uint16(stats[k, 5])
                if sem_cls in self.background_cls_list:
                    s = stats[k]
                    union = s[1:5].copy() if union is None else np.array([min(union[0], s[1]), max(union[1], s[2]),
                                                                          min(union[2], s[3]), max(union[3], s[4])])
                    continue
                inst_to_cls[np.int32(ids[k])] = sem_cls
                rows.append(k)
        entries = ([(None, 0, union)] if union is not None else []) + [(k, ids[k], stats[k, 1:5]) for k in rows]
        for k, obj_id, (r0, r1, c0, c1) in entries:
            obj_id = np.int32(obj_id)
            bbox2d = _bbox_of_mask(r0, r1, c0, c1, self.bbox_scale, W, H)
            if bbox2d is None:
                continue                                      # set to background
            if k is not None:
                keep[k] = True
            min_x, min_y, max_x, max_y = bbox2d
            _add_frame_info(self.inst_dict, inst_to_cls[obj_id], obj_id, frame,
                            torch.from_numpy(np.array([min_x, max_x, min_y, max_y])))
            if self._accumulate and obj_id != 0:
                self._frame_objects.setdefault(frame, []).append((inst_to_cls[obj_id], obj_id))
        return keep
