"""The forward-only consumer of the hot path inside category registration: ``get_uncertainty_fields``
(src/category_registration.py:58-177) -- 100 x 100 probe rays on a sphere around each pretrained object, 96 jittered
samples per ray, UniDirsEmbed -> OccupancyMap -> sigmoid(10 sigma) -> non-batch occupancy_to_termination -> ray
entropies -> the per-object count of rays below a threshold that ranks the objects of a class.

Everything between the rays and the count runs on the device through the drop-in modules (cnr_pe_fwd, the dense
kernels, cnr_composite_fwd's termination); the reference moves the occupancies to the host and finishes in numpy.

The rest of that file for Replica sequences is below it: ``get_all_poses`` (point-cloud accumulation), ``align_poses`` (the
reference's bookkeeping around a pluggable solver: the default is the multi-start GPU ICP ``IcpSolver``, and ``TeaserSolver``
is a TEASER-style global solver on the kernels of csrc/teaser.hip) and ``register_dataset`` (the driver behind ``dataset.get_dataset(cfg, register=True)``), on the kernels of
csrc/pointcloud.hip.  ScanNet sequences register on request (``tsdf=True``): their background cloud is a TSDF
fusion on the kernels of csrc/tsdf.hip, their objects' clouds come from the loader.
"""
import math
import os

import numpy as np
import torch

from . import _C, embedding, model, render_rays
from .scene_cateogries import stratified_bins

N_PROBE = 100          # phi x theta grid (src/category_registration.py:96-98)
N_PROBE_BINS = 96      # samples per probe ray (:145)


def calculate_reliability(metric, eta=0.9, m1=0.1, m2=0.15, M1=0.57, M2=0.65):
    """src/utils.py:553-559, on tensors."""
    k = 2 * math.log(eta / (1 - eta))
    a_m, b_m = k / (m2 - m1), (m1 + m2) / 2
    a_M, b_M = k / (M2 - M1), (M1 + M2) / 2
    return 1 / (1 + torch.exp(a_m * (metric - b_m))) + 1 / (1 + torch.exp(-a_M * (metric - b_M)))


def probe_sphere():
    """Unit directions of the probe grid, (10000, 3), in the reference's order (:96-107: meshgrid of linspace(0, pi, 100)
    x linspace(0, 2 pi, 100), transposed, flattened)."""
    phi = torch.linspace(0, np.pi, N_PROBE)
    theta = torch.linspace(0, 2 * np.pi, N_PROBE)
    phi, theta = torch.meshgrid(phi, theta, indexing="ij")
    phi, theta = phi.t(), theta.t()
    return torch.stack([torch.sin(phi) * torch.cos(theta), torch.sin(phi) * torch.sin(theta), torch.cos(phi)], -1).reshape(-1, 3)


def uncertainty_probe(pe, fc_occ_map, center, r, device, z_vals=None, generator=None):
    """One object's probe (:131-156): rays from the sphere of radius ``r`` around ``center`` towards it, far = 2 r.
    -> (termination (N,96), entropies (N,), opacity (N,)) on ``device``.  ``z_vals`` (N,96) replaces the jittered bins
    (tests); ``generator`` seeds them."""
    r = float(r)
    rays_o_o = (r * probe_sphere()).to(device)
    viewdir = -rays_o_o / r
    rays_o = torch.as_tensor(center, dtype=torch.float32, device=device) + rays_o_o
    n = rays_o.shape[0]
    if z_vals is None:
        z_vals = stratified_bins(0, 2 * r, N_PROBE_BINS, n, device=device, z_fixed=True, generator=generator)
    xyz = rays_o[..., None, :] + viewdir[:, None, :] * z_vals.to(device)[..., None]
    with torch.no_grad():
        sigmas, _ = fc_occ_map(pe(xyz))
        occupancies = torch.sigmoid(10 * sigmas.squeeze(-1))
        term = render_rays.occupancy_to_termination(occupancies)
        entropies = torch.sum(-term * torch.log(term + 1e-10), dim=-1)
    return term, entropies, term.sum(-1)


def load_pretrained_fields(inst_dict, bbox3d_dict, pe_dict, fc_occ_map_dict, cfg):
    """The ``load_pretrained`` branch (:64-92): per object the newest file under ``cfg.weight_root/ckpt/<obj_id>/`` with the
    keys FC_state_dict, PE_state_dict, obj_scale, bbox -> an OccupancyMap(hidden_feature_size) + UniDirsEmbed on the data
    device."""
    emb1 = 21 * (3 + 1) + 3
    emb2 = 21 * (5 + 1) + 3 - emb1
    for cls_id, inst_dict_cls in inst_dict.items():
        if cls_id == 0:
            continue
        for d in (fc_occ_map_dict, pe_dict, bbox3d_dict):
            d.setdefault(cls_id, {})
        for obj_id in inst_dict_cls.keys():
            ckpt_dir = os.path.join(cfg.weight_root, "ckpt", str(obj_id))
            ckpt = torch.load(os.path.join(ckpt_dir, sorted(os.listdir(ckpt_dir))[-1]), map_location="cpu", weights_only=False)
            fc = model.OccupancyMap(emb1, emb2, hidden_size=cfg.hidden_feature_size)
            fc.load_state_dict(ckpt["FC_state_dict"])
            pe = embedding.UniDirsEmbed(max_deg=cfg.n_unidir_funcs, scale=ckpt["obj_scale"])
            pe.load_state_dict(ckpt["PE_state_dict"])
            fc_occ_map_dict[cls_id][obj_id] = fc.to(cfg.data_device)
            pe_dict[cls_id][obj_id] = pe.to(cfg.data_device)
            bbox3d_dict[cls_id][obj_id] = ckpt["bbox"]


def _points(pcs):
    return np.asarray(pcs.points if hasattr(pcs, "points") else pcs)


def get_uncertainty_fields(inst_dict, bbox3d_dict, count_dict, pe_dict, fc_occ_map_dict, cfg, name="replica",
                           load_pretrained=False, use_reliability=True, generator=None):
    """src/category_registration.py:58-177 with the reference's arguments: fills ``count_dict[cls_id][obj_id]`` with the
    number of probe rays whose (1 - reliability) is below 0.5 (``use_reliability``) or whose entropy is below 0.8 x the
    smallest per-object maximum.  ``inst_dict[cls_id][obj_id]['pcs']`` is a point cloud (anything with ``.points``, or an
    (n,3) array).  ``generator``: a device generator for the bin jitter (the reference draws from the global one)."""
    if load_pretrained:
        load_pretrained_fields(inst_dict, bbox3d_dict, pe_dict, fc_occ_map_dict, cfg)
    dev = torch.device(cfg.data_device)
    for cls_id in fc_occ_map_dict.keys():
        count_dict.setdefault(cls_id, {})
        # radius per object from its point cloud's half extents, at least 5 cm each (:115-123)
        bounds = []
        for obj_id in inst_dict[cls_id].keys():
            p = _points(inst_dict[cls_id][obj_id]["pcs"])
            bounds.append(torch.from_numpy((np.maximum(p.max(axis=0) - p.min(axis=0), 0.10) / 2).astype(np.float32)))
        rs = 1.2 * torch.sqrt(torch.square(torch.stack(bounds, dim=0)).sum(dim=-1))
        obj_ids = list(fc_occ_map_dict[cls_id].keys())
        ent_max, metrics = [], []
        for idx, obj_id in enumerate(obj_ids):
            p = _points(inst_dict[cls_id][obj_id]["pcs"])
            center = ((p.max(axis=0) + p.min(axis=0)) / 2 if name == "replica" else p.mean(axis=0)).astype(np.float32)
            term, entropies, opacity = uncertainty_probe(pe_dict[cls_id][obj_id], fc_occ_map_dict[cls_id][obj_id],
                                                         center, rs[idx], dev, generator=generator)
            ent_max.append(entropies.max())
            if use_reliability:
                heuristic = opacity * torch.exp(-0.5 * entropies)
                metrics.append(1 - calculate_reliability(heuristic, eta=0.9, m1=0.1, m2=0.15, M1=0.57, M2=0.65))
            else:
                metrics.append(entropies)
        threshold = 0.5 if use_reliability else 0.8 * torch.stack(ent_max).min()
        counts = torch.stack([(m < threshold).sum() for m in metrics]).cpu() if metrics else []   # ONE host sync per class
        for obj_id, n in zip(obj_ids, counts):
            count_dict[cls_id][obj_id] = int(n)


# ---- point clouds, alignment, sub-categorisation (src/category_registration.py:18-56, :179-324) -------------------------
# DESIGN.md §3.9 and §3.10.  align_poses(..., solver=) takes IcpSolver (the default), TeaserSolver or FpfhTeaserSolver.
def get_all_poses(inst_dict, sample_dict, intrinsic_open3d, name="replica", depth_scale=0.001, max_depth=8.0, tsdf=False):
    """:18-56.  Replica: every instance of every class gets 'pcs', its pixels of all its frames as one cloud at 1 cm.  ScanNet
    (only with tsdf=True): an instance's 'pcs' is what the loader gathered frame by frame, down-sampled to 1 cm; an instance
    without one (or with an empty one) gets T_obj = eye(4) and pcs = None.  The background (class 0) gets 'pcs' too -- for
    ScanNet from a TSDF volume (utils.accumulate_pointcloud_tsdf) -- and 'bbox3D', the oriented box of that cloud with its true
    extents (no 10 cm floor)."""
    from . import metrics
    from .utils import BoundingBox, accumulate_pointcloud, accumulate_pointcloud_tsdf
    if name != "replica" and not tsdf:
        raise NotImplementedError("get_all_poses: ScanNet registration fuses the background in a TSDF volume and takes the "
                                  "objects' clouds from refined masks on disk (geometry_segmentation is not part of this "
                                  "package); it runs only on request: tsdf=True")
    for cls_id, entries in inst_dict.items():
        if cls_id != 0:
            for inst_id, entry in entries.items():
                if name == "replica":
                    entry["pcs"] = accumulate_pointcloud(int(inst_id), entry["frame_info"], sample_dict, intrinsic_open3d)
                elif entry.get("pcs") is None or len(entry["pcs"]) == 0:
                    print(f"{inst_id} is not detected from semantically refined geometry segmentations")
                    entry["T_obj"], entry["pcs"] = np.eye(4), None
                else:
                    entry["pcs"] = entry["pcs"].voxel_down_sample(0.01)
            continue
        if name == "replica":
            cloud = accumulate_pointcloud(0, entries["frame_info"], sample_dict, intrinsic_open3d)
        else:
            cloud = accumulate_pointcloud_tsdf(0, entries["frame_info"], sample_dict, intrinsic_open3d, depth_scale=depth_scale,
                                               max_depth=max_depth)
        to_box, extents = metrics.oriented_bounds(cloud.points)
        from_box = np.linalg.inv(to_box)
        box = BoundingBox()
        box.R, box.center, box.extent = from_box[:3, :3], from_box[:3, 3], extents
        entries["bbox3D"], entries["pcs"] = box, cloud


def _rigid_fit(a, b):
    """(n,3) -> the rigid (4,4) T minimising |T a - b| (Kabsch, fp64, host) and the largest residual"""
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, cb - R @ ca
    return T, float(np.abs(a @ R.T + T[:3, 3] - b).max())


def icp_device(source, target, T0, max_corr, max_iteration=100):
    """Point-to-point ICP of (n,3) f32 device `source` against (m,3) f32 device `target` from B starts T0 (B,4,4), all through
    cnr_icp_step / cnr_icp_update together; open3d's convergence test (1e-6 on fitness and rmse), at most max_iteration
    updates.  A converged start freezes on the device; the host reads the flags every 10 iterations.
    -> (T (B,4,4) f64 numpy, state (B,4) numpy: fitness, rmse, flag, updates)"""
    dev = source.device
    T = torch.from_numpy(np.ascontiguousarray(np.asarray(T0, np.float64).reshape(-1, 4, 4))).to(dev)
    B, n, m = len(T), len(source), len(target)
    ws = _C.workspace(_C.load().cnr_icp_workspace_bytes(n, m, B), dev, "cnr_icp_step")
    state = torch.zeros(B, 4, device=dev, dtype=torch.float64)
    sums = torch.zeros(B, 17, device=dev, dtype=torch.float64)
    for it in range(int(max_iteration) + 1):
        _C.call("cnr_icp_step", source, n, target, m, T, B, float(max_corr), state, ws, sums, None, None)
        _C.call("cnr_icp_update", sums, n, B, int(max_iteration), T, state)
        if it % 10 == 9 and bool((state[:, 2] != 0).all()):
            break
    return T.cpu().numpy(), state.cpu().numpy()


class IcpSolver:
    """The default solver of align_poses: both clouds down-sampled to `voxel_size`, one start per template that puts the source's
    oriented box onto the template's, point-to-point ICP (pairs closer than `max_corr`) from every start together.

    The templates must be rigid copies of the first, point for point (align_poses passes the representative rotated by the 24
    box symmetries S_k, or the representative alone).  Template k's box frame is the first template's box moved by S_k with
    its axes relabelled by inv(S_k): F_k = S_k F_0 inv(rot S_k).  The 24 starts are then the 24 ways of laying one box onto the
    other, and all of them run against ONE target cloud in one batch.  Anything else raises a ValueError."""

    FIT_POINTS = 512          # points of the rigid fit, taken with a stride over the whole template

    def __init__(self, voxel_size=0.02, max_corr=0.10, max_iteration=100):
        self.voxel_size, self.max_corr, self.max_iteration = voxel_size, max_corr, max_iteration

    @staticmethod
    def _box_frame(pc, what):
        from .utils import get_bound
        box = get_bound(pc)
        if box is None:
            raise ValueError(f"IcpSolver: the {what} cloud has no 3-D convex hull")
        F = np.eye(4)
        F[:3, :3], F[:3, 3] = box.R, box.center
        return F

    def _copies(self, tm):
        """tm (B,m,3) -> [S_k] with tm[k] = S_k tm[0]: fitted on a strided subset, the residual checked on every point"""
        pick = tm[0][::max(1, tm.shape[1] // self.FIT_POINTS)]
        spread = np.linalg.svd(pick - pick.mean(0), compute_uv=False)
        if len(pick) < 3 or not spread[1] > 1e-9 * max(spread[0], 1e-300):
            raise ValueError("IcpSolver: the template is (nearly) a line; no rigid fit between its copies is unique")
        tol = 1e-5 * (1.0 + float(np.abs(tm[0]).max()))
        rel = [np.eye(4)]
        for k in range(1, len(tm)):
            S, _ = _rigid_fit(pick, tm[k][::max(1, tm.shape[1] // self.FIT_POINTS)])
            res = float(np.abs(tm[0] @ S[:3, :3].T + S[:3, 3] - tm[k]).max())
            if not res < tol:
                raise ValueError(f"IcpSolver: template {k} is no rigid copy of template 0 (residual {res:.3g} m); pass another "
                                 "solver to align_poses for such templates")
            rel.append(S)
        return rel

    def __call__(self, source, templates):
        from .utils import PointCloud
        dev = source.device if torch.is_tensor(source) and source.is_cuda else None
        as_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        src = as_np(source).astype(np.float64)[0].T
        tm = as_np(templates).astype(np.float64).transpose(0, 2, 1)
        rel = self._copies(tm)
        src_ds = PointCloud(src, device=dev).voxel_down_sample(self.voxel_size)
        tgt_ds = PointCloud(tm[0], device=dev).voxel_down_sample(self.voxel_size)
        F_s, F_0 = self._box_frame(src_ds, "source"), self._box_frame(tgt_ds, "template")
        starts = []
        for S in rel:
            Q = np.eye(4)
            Q[:3, :3] = S[:3, :3].T
            starts.append(F_0 @ Q @ np.linalg.inv(F_s))          # = inv(S) F_k inv(F_s)
        T, self.last_state = icp_device(src_ds.points_device, tgt_ds.points_device, np.stack(starts), self.max_corr,
                                        self.max_iteration)
        T = np.stack([S @ Tk for S, Tk in zip(rel, T)])
        return torch.from_numpy(T[:, :3, :3].copy()), torch.from_numpy(T[:, :3, 3:].copy())


# ---- TEASER-style global registration -------------------------------------------------------------------
# The stages of Yang, Shi, Carlone, "TEASER: Fast and Certifiable Point Cloud Registration" (arXiv 2001.07715) with the
# parameters of the reference's get_teaser_solver, in its "simultaneous pose and correspondence" use: all-to-all
# correspondences, compatibility graph, maximum clique, GNC-TLS rotation, voted translation, ICP.  The graph and the clique
# are HIP (csrc/teaser.hip); rotation and translation work on a few hundred 3-vectors and run on the host in fp64.
TEASER_MAX_N = 16384          # CNR_TEASER_MAX_N


def teaser_correspondences(source, template, voxel_size=0.1, max_correspondences=10000, rng=None, device=None):
    """Stage 1.  Both clouds ((n,3) arrays or PointClouds) down-sampled to voxel_size, all n_s n_t pairs, and when there are more
    than max_correspondences that many of them drawn without replacement from `rng` (a numpy Generator; default seed 0), kept
    in ascending pair order.  -> (A (N,3), B (N,3) f32 device tensors with A[i] <-> B[i], the two down-sampled PointClouds,
    pairs (N,2) int64 host: indices into them)"""
    from .utils import PointCloud
    as_cloud = lambda c: c if isinstance(c, PointCloud) else PointCloud(np.asarray(c, np.float64), device=device)
    src_ds, tgt_ds = as_cloud(source).voxel_down_sample(voxel_size), as_cloud(template).voxel_down_sample(voxel_size)
    n_s, n_t = len(src_ds), len(tgt_ds)
    total = n_s * n_t
    if int(max_correspondences) < 1 or int(max_correspondences) > TEASER_MAX_N:
        raise ValueError(f"max_correspondences must lie in [1, {TEASER_MAX_N}]")
    if total > int(max_correspondences):
        rng = np.random.default_rng(0) if rng is None else rng
        flat = np.sort(rng.choice(total, int(max_correspondences), replace=False))
    else:
        flat = np.arange(total)
    pairs = np.stack([flat // n_t, flat % n_t], 1).astype(np.int64)
    dev = src_ds.points_device.device
    A = src_ds.points_device[torch.from_numpy(pairs[:, 0]).to(dev)].contiguous()
    B = tgt_ds.points_device.to(dev)[torch.from_numpy(pairs[:, 1]).to(dev)].contiguous()
    return A, B, src_ds, tgt_ds, pairs


def compatibility_threshold(noise_bound=0.01, cbar2=1.0):
    """2 noise_bound sqrt(cbar2), rounded once to fp32: the bound of the graph's fp32 comparison"""
    return float(np.float32(2.0 * float(noise_bound) * math.sqrt(float(cbar2))))


def compatibility_graph(A, B, noise_bound=0.01, cbar2=1.0):
    """Stage 2 (cnr_teaser_graph).  A, B (N,3) f32 device tensors -> (adj (N, ceil(N/64)) int64 device tensor: bit j & 63 of word
    j >> 6 of row i says i ~ j, i.e. | |B_i - B_j| - |A_i - A_j| | <= 2 noise_bound sqrt(cbar2) in fp32; deg (N,) int32)"""
    N = len(A)
    if not 1 <= N <= TEASER_MAX_N or A.shape != (N, 3) or B.shape != (N, 3):
        raise ValueError(f"compatibility_graph: (N,3) correspondences with 1 <= N <= {TEASER_MAX_N}")
    if not (torch.is_tensor(A) and torch.is_tensor(B) and A.is_cuda and B.device == A.device):
        raise ValueError("compatibility_graph: A and B are tensors on one GPU")
    A, B = A.to(torch.float32).contiguous(), B.to(torch.float32).contiguous()
    adj = torch.empty(N, (N + 63) // 64, device=A.device, dtype=torch.int64)
    deg = torch.empty(N, device=A.device, dtype=torch.int32)
    _C.call("cnr_teaser_graph", A, B, N, compatibility_threshold(noise_bound, cbar2), adj, deg)
    return adj, deg


DEFAULT_SEARCH_BUDGET = 1 << 20          # row ANDs one root vertex may spend


def clique_order(deg):
    """the fixed vertex order of the search: ascending degree, ties by index -> (N,) int32 device tensor"""
    return torch.sort(deg.to(torch.int64), stable=True)[1].to(torch.int32).contiguous()


def max_clique(adj, deg, search_budget=None):
    """Stage 3 (cnr_clique_search).  -> (clique: int64 host array of vertices, ascending in clique_order(deg); info: size, exact,
    steps, find_steps, max_root_steps, roots_out_of_budget, greedy_size, flags).  With exact the clique is the maximum clique
    that is lexicographically smallest in positions of clique_order(deg); without, it is a clique and its size a lower bound."""
    N, dev = len(deg), adj.device
    if not (adj.is_cuda and deg.device == dev and adj.dtype == torch.int64 and adj.shape == (N, (N + 63) // 64)
            and deg.dtype == torch.int32 and deg.dim() == 1 and 1 <= N <= TEASER_MAX_N):
        raise ValueError(f"max_clique: adj (N, ceil(N/64)) int64 and deg (N,) int32 on one GPU, 1 <= N <= {TEASER_MAX_N}")
    adj, deg = adj.contiguous(), deg.contiguous()
    budget = DEFAULT_SEARCH_BUDGET if search_budget is None else int(search_budget)
    if budget < 1 or budget >= 1 << 31:
        raise ValueError("search_budget must lie in [1, 2^31)")
    order = clique_order(deg)
    max_degree = int(deg.max())
    ws = _C.workspace(_C.load().cnr_clique_workspace_bytes(N, max_degree), dev, "cnr_clique_search")
    out = torch.zeros(max_degree + 1, device=dev, dtype=torch.int32)
    info = torch.zeros(8, device=dev, dtype=torch.int64)
    _C.call("cnr_clique_search", adj, order, N, max_degree, budget, ws, out, info)
    v = [int(x) for x in info.cpu()]
    keys = ("size", "exact", "steps", "find_steps", "max_root_steps", "roots_out_of_budget", "greedy_size", "flags")
    res = dict(zip(keys, v))
    res["exact"] = bool(res["exact"])
    return out[:res["size"]].cpu().numpy().astype(np.int64), res


def _weighted_rotation(a, b, w):
    """the proper rotation minimising sum w |b - R a|^2 (no centring: the inputs are translation-free)"""
    U, _, Vt = np.linalg.svd((a * w[:, None]).T @ b)
    return Vt.T @ np.diag([1.0, 1.0, np.linalg.det(Vt.T @ U.T)]) @ U.T


def gnc_tls_rotation(a, b, bound, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12):
    """Stage 4.  Graduated non-convexity on the truncated least squares cost sum min(|b_k - R a_k|^2, bound) over (K,3) fp64
    measurement pairs.  Per iteration: the weighted SVD fit; with r = the squared residuals, on the first iteration mu = 1 /
    (2 max r / bound - 1) (mu <= 0: every residual is inside the bound, done); weights 1 below mu/(mu+1) bound, 0 above
    (mu+1)/mu bound, sqrt(bound mu (mu+1) / r) - mu between; mu *= gnc_factor; stop when the weighted cost moves by less than
    cost_threshold.  -> (R (3,3), iterations, weights (K,))"""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    w = np.ones(len(a))
    if len(a) == 0:
        return np.eye(3), 0, w
    R, mu, prev = np.eye(3), 1.0, math.inf
    it = 0
    for it in range(1, int(max_iterations) + 1):
        R = _weighted_rotation(a, b, w)
        r = ((b - a @ R.T) ** 2).sum(1)
        if it == 1:
            denom = 2.0 * r.max() / bound - 1.0
            if denom <= 0:
                break
            mu = 1.0 / denom
        cost = float((w * r).sum())
        hi, lo = (mu + 1.0) / mu * bound, mu / (mu + 1.0) * bound
        w = np.where(r >= hi, 0.0, np.where(r <= lo, 1.0, np.sqrt(bound * mu * (mu + 1.0) / np.maximum(r, 1e-300)) - mu))
        mu *= gnc_factor
        done = abs(cost - prev) < cost_threshold
        prev = cost
        if done:
            break
    return R, it, w


def tls_scalar(x, bound, cbar2=1.0):
    """TEASER's adaptive voting for one scalar: the minimiser of sum min((x_k - t)^2 / bound^2, cbar2).  Each measurement votes
    for [x_k - bound cbar, x_k + bound cbar]; between two consecutive interval ends the consensus set is constant, its mean the
    candidate, and the candidate of the lowest cost wins (the first of equals).  -> (t, consensus mask)"""
    x = np.asarray(x, np.float64).reshape(-1)
    half = bound * math.sqrt(cbar2)
    ends = np.sort(np.concatenate([x - half, x + half]))
    best = (math.inf, 0.0, np.zeros(len(x), bool))
    for m in (ends[:-1] + ends[1:]) / 2:
        inside = np.abs(x - m) <= half
        if not inside.any():
            continue
        t = float(x[inside].mean())
        cost = float(((x[inside] - t) ** 2).sum() / bound ** 2 + cbar2 * (len(x) - inside.sum()))
        if cost < best[0]:
            best = (cost, t, inside)
    if not best[2].any():
        best = (0.0, float(x.mean()) if len(x) else 0.0, np.ones(len(x), bool))
    return best[1], best[2]


def tls_translation(a, b, R, noise_bound=0.01, cbar2=1.0):
    """Stage 5.  Component-wise adaptive voting on b_k - R a_k with bound noise_bound sqrt(cbar2) -> t (3,)"""
    d = np.asarray(b, np.float64) - np.asarray(a, np.float64) @ np.asarray(R, np.float64).T
    return np.array([tls_scalar(d[:, k], noise_bound, cbar2)[0] for k in range(3)])


class TeaserSolver:
    """A solver for align_poses(..., solver=): TEASER's stages with the reference's parameters as defaults (get_teaser_solver,
    TEASER_FPFH_ICP with spc=True), see the stage functions above.  Templates that are rigid copies of the first (align_poses'
    24 box symmetries) share one graph, one clique and one pose T.  The B starts S_k T are refined the way IcpSolver runs
    its batch: against the ONE down-sampled first template, each start taken back by inv(S_k) -- where all B coincide, so one ICP
    runs and its result is moved by each S_k.  That equals refining S_k T against a down-sampled template k only while
    down-sampling commutes with S_k (every point alone in its voxel); on dense clouds the voxel centroids of a rotated
    template differ, and so would that refinement, by an amount that is not measured.  Other templates are solved one by one.  last_info: per solved template group N, candidates (the correspondences before sub-sampling), edges, clique_size, exact, gnc_iterations, icp_state, the
    search's step counts, and graph_builds for the call."""

    def __init__(self, voxel_size=0.1, noise_bound=0.01, max_correspondences=10000, cbar2=1.0, gnc_factor=1.4,
                 rotation_max_iterations=100, rotation_cost_threshold=1e-12, icp_max_iteration=100, seed=0, search_budget=None,
                 icp_max_corr=None):
        self.voxel_size, self.noise_bound, self.max_correspondences, self.cbar2 = voxel_size, noise_bound, max_correspondences, cbar2
        self.gnc_factor, self.rotation_max_iterations = gnc_factor, rotation_max_iterations
        self.rotation_cost_threshold, self.icp_max_iteration, self.seed = rotation_cost_threshold, icp_max_iteration, seed
        self.search_budget, self.icp_max_corr = search_budget, icp_max_corr
        self.last_info = None

    def solve_pose(self, A, B, clique):
        """stages 4 and 5 on the clique's correspondences -> (T (4,4) source -> template, GNC iterations)"""
        a, b = A[clique].double().cpu().numpy(), B[clique].double().cpu().numpy()
        nxt = np.roll(np.arange(len(clique)), -1)                    # the chain: each member with the next, the last with the first
        k = len(clique) if len(clique) > 2 else len(clique) - 1      # (two members: one measurement, one member: none)
        R, its, _ = gnc_tls_rotation((a[nxt] - a)[:k], (b[nxt] - b)[:k], (2.0 * self.noise_bound) ** 2 * self.cbar2, self.gnc_factor,
                                     self.rotation_max_iterations, self.rotation_cost_threshold)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, tls_translation(a, b, R, self.noise_bound, self.cbar2)
        return T, its

    def correspondences(self, source, template, device=None):
        """stage 1, the one stage a subclass replaces -> what teaser_correspondences returns and a dict that goes into the
        solve's info: candidates = the number of correspondences before any sub-sampling"""
        out = teaser_correspondences(source, template, self.voxel_size, self.max_correspondences,
                                     np.random.default_rng(self.seed), device)
        return out + (dict(candidates=len(out[2]) * len(out[3])),)

    def solve_one(self, source, template, device=None):
        """one source (n,3) against one template (m,3) -> (T (4,4) after ICP, info)"""
        A, B, src_ds, tgt_ds, _, stage1 = self.correspondences(source, template, device)
        adj, deg = compatibility_graph(A, B, self.noise_bound, self.cbar2)
        clique, found = max_clique(adj, deg, self.search_budget)
        T0, its = self.solve_pose(A, B, torch.from_numpy(clique).to(A.device))
        max_corr = self.noise_bound if self.icp_max_corr is None else self.icp_max_corr
        T, state = icp_device(src_ds.points_device, tgt_ds.points_device, T0[None], max_corr, self.icp_max_iteration)
        info = dict(N=len(A), edges=int(deg.sum(dtype=torch.int64)) // 2, clique_size=len(clique), exact=found["exact"],
                    gnc_iterations=its, icp_state=state, T_before_icp=T0, clique=clique, search=found, **stage1)
        return T[0], info

    def __call__(self, source, templates):
        dev = source.device if torch.is_tensor(source) and source.is_cuda else None
        as_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
        src = as_np(source).astype(np.float64)[0].T
        tm = as_np(templates).astype(np.float64).transpose(0, 2, 1)
        try:
            rel = IcpSolver()._copies(tm) if len(tm) > 1 else [np.eye(4)]
        except ValueError:
            rel = None
        if rel is not None:
            T, info = self.solve_one(src, tm[0], dev)
            out, groups = np.stack([S @ T for S in rel]), [info]
            info["icp_state"] = np.repeat(info["icp_state"], len(rel), axis=0)
        else:
            solved = [self.solve_one(src, t, dev) for t in tm]
            out, groups = np.stack([T for T, _ in solved]), [i for _, i in solved]
        self.last_info = dict(groups[0], graph_builds=len(groups), rigid_copies=rel is not None, groups=groups)
        return torch.from_numpy(out[:, :3, :3].copy()), torch.from_numpy(out[:, :3, 3:].copy())


# ---- TEASER's FPFH mode (spc=False; src/teaser_utils/helpers.py) -----------------------------------------------
FEATURE_MAX_D = 64


def compute_fpfh_feature(pcd, radius, max_nn):
    """open3d's compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) for a utils.PointCloud with normals: ONE
    hybrid search, cnr_spfh, cnr_fpfh -> (n,33) f64 device tensor (open3d's fpfh.data transposed)"""
    from .utils import hybrid_search
    if pcd.normals_device is None:
        raise ValueError("compute_fpfh_feature: the cloud has no normals; call estimate_normals first")
    points, n = pcd.points_device, len(pcd)
    spfh = torch.empty(n, 33, device=points.device, dtype=torch.float64)
    fpfh = torch.empty(n, 33, device=points.device, dtype=torch.float64)
    if n:
        idx, d2, count = hybrid_search(points, radius, max_nn)
        _C.call("cnr_spfh", points, pcd.normals_device.contiguous(), n, idx, count, int(max_nn), spfh)
        _C.call("cnr_fpfh", spfh, n, idx, d2, count, int(max_nn), fpfh)
    return fpfh


def feature_nn(q, p):
    """cnr_feature_nn: q (nq,D), p (nr,D) device tensors, rounded to f32 -> (index (nq,) int32: the lowest row of p with the
    least sequential fp32 sum of squared differences, that sum (nq,) f32)"""
    q, p = q.to(torch.float32).contiguous(), p.to(device=q.device, dtype=torch.float32).contiguous()
    if q.dim() != 2 or p.dim() != 2 or q.shape[1] != p.shape[1] or not 1 <= q.shape[1] <= FEATURE_MAX_D or len(p) < 1:
        raise ValueError(f"feature_nn: q (nq,D) and p (nr,D) with 1 <= D <= {FEATURE_MAX_D} and nr >= 1")
    index = torch.empty(len(q), device=q.device, dtype=torch.int32)
    dist = torch.empty(len(q), device=q.device, dtype=torch.float32)
    if len(q):
        ws = _C.workspace(_C.load().cnr_feature_nn_workspace_bytes(len(q), len(p)), q.device, "cnr_feature_nn")
        _C.call("cnr_feature_nn", q, len(q), p, len(p), int(q.shape[1]), index, dist, ws)
    return index, dist


def mutual_correspondences(f0, f1, mutual_filter=True):
    """helpers.find_correspondences on device descriptors (n0,D), (n1,D): i <-> its nearest row of f1 (feature_nn on the f32-rounded
    descriptors), kept, with mutual_filter, iff i is the nearest row of f0 to that row in turn -> (idx0, idx1) int64 device
    tensors, idx0 ascending"""
    if len(f0) == 0 or len(f1) == 0:
        empty = torch.zeros(0, dtype=torch.int64, device=f0.device)
        return empty, empty.clone()
    nn01 = feature_nn(f0, f1)[0].to(torch.int64)
    idx0 = torch.arange(len(f0), device=f0.device)
    if not mutual_filter:
        return idx0, nn01
    nn10 = feature_nn(f1, f0)[0].to(torch.int64)
    keep = nn10[nn01] == idx0
    return idx0[keep], nn01[keep]


def extract_fpfh_device(pcd, voxel_size):
    """helpers.extract_fpfh on the device: normals at 2 voxel_size / 30, FPFH at 5 voxel_size / 100 -> (n,33) f64 device tensor"""
    pcd.estimate_normals(radius=voxel_size * 2, max_nn=30)
    return compute_fpfh_feature(pcd, voxel_size * 5, 100)


class FpfhTeaserSolver(TeaserSolver):
    """TeaserSolver with the reference's spc=False correspondences: both clouds down-sampled to voxel_size, FPFH descriptors
    (extract_fpfh_device), mutual nearest neighbours in descriptor space -- at most min(n_s, n_t) pairs; more than
    max_correspondences are sub-sampled as in teaser_correspondences.  noise_bound=None means voxel_size, as the reference sets
    it in this mode.  Graph, clique, rotation, translation and ICP are TeaserSolver's.  last_info gains n_src, n_tgt and
    correspondences ((N,2) int64: indices into the down-sampled clouds).  No correspondence at all raises a ValueError; between
    two non-empty clouds the closest pair of descriptors is always mutual, so this only guards a search that returned nothing."""

    def __init__(self, voxel_size=0.05, noise_bound=None, **kw):
        super().__init__(voxel_size=voxel_size, noise_bound=voxel_size if noise_bound is None else noise_bound, **kw)

    def correspondences(self, source, template, device=None):
        from .utils import PointCloud
        as_cloud = lambda c: c if isinstance(c, PointCloud) else PointCloud(np.asarray(c, np.float64), device=device)
        src_ds, tgt_ds = as_cloud(source).voxel_down_sample(self.voxel_size), as_cloud(template).voxel_down_sample(self.voxel_size)
        if int(self.max_correspondences) < 1 or int(self.max_correspondences) > TEASER_MAX_N:
            raise ValueError(f"max_correspondences must lie in [1, {TEASER_MAX_N}]")
        i0, i1 = mutual_correspondences(extract_fpfh_device(src_ds, self.voxel_size), extract_fpfh_device(tgt_ds, self.voxel_size))
        pairs = torch.stack([i0, i1], 1).cpu().numpy().astype(np.int64)
        candidates = len(pairs)
        if candidates > int(self.max_correspondences):
            pairs = pairs[np.sort(np.random.default_rng(self.seed).choice(candidates, int(self.max_correspondences), replace=False))]
        if candidates == 0:
            raise ValueError(f"FpfhTeaserSolver: no mutual FPFH correspondence between the {len(src_ds)} source and {len(tgt_ds)} "
                             f"template points at voxel_size {self.voxel_size}")
        dev = src_ds.points_device.device
        A = src_ds.points_device[torch.from_numpy(pairs[:, 0]).to(dev)].contiguous()
        B = tgt_ds.points_device.to(dev)[torch.from_numpy(pairs[:, 1]).to(dev)].contiguous()
        return A, B, src_ds, tgt_ds, pairs, dict(candidates=candidates, n_src=len(src_ds), n_tgt=len(tgt_ds), correspondences=pairs)


def _mean_nn_distance(points_from, points_to):
    """mean distance of the points of one device tensor / host array to the nearest point of another (cnr_nn_dist +
    cnr_dist_stats)"""
    from . import metrics
    d = metrics.nn_dist(points_from, points_to)
    return metrics.dist_stats(d)[0] / len(d)


def _unit_scale(T):
    """(4,4) similarity -> (the same with a pure rotation, its scale)"""
    out = np.array(T, dtype=np.float64)
    scale = np.cbrt(np.linalg.det(out[:3, :3]))
    out[:3, :3] /= scale
    return out, scale


def _best_candidate(source_pts, template_dev, symmetries, R_all, t_all, dev):
    """the solver's answers (source -> template k) undone by the symmetries, each scored by the mean distance of the moved
    source to the template -> (T_rel of the lowest score, that score in metres)"""
    from .utils import transform_pointcloud
    best = None
    for S, R, t in zip(symmetries, R_all, t_all):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, np.reshape(t, 3)
        T = np.linalg.inv(S) @ T
        moved = torch.from_numpy(transform_pointcloud(source_pts, T)).to(dev)
        score = _mean_nn_distance(moved, template_dev)
        if best is None or score < best[1]:          # the first of equal scores, as argmin picks
            best = (T, score)
    return best


def align_poses(inst_dict, bbox3d_dict, count_dict, pe_dict, fc_occ_map_dict, name="replica", multi_init_pose=True, eta1=0.06,
                eta2=0.15, eta3=0.12, device="cuda:0", solver=None):
    """:179-324, the reference's decisions in this package's words.  Classes are taken from bbox3d_dict until it is empty.  Per
    class the instance with the highest count is the representative: T_obj and bbox3D from its own oriented box.  Every other
    instance is aligned to it by ``solver(source (1,3,n), templates (B,3,m)) -> (R (B,3,3), t (B,3,1))`` (the signature of
    TEASER_FPFH_ICP(source).forward(template); default IcpSolver()), where the templates are the representative under the 24
    box symmetries (one template without multi_init_pose).  The candidate whose moved source lies closest to the template wins;
    that distance over the source's half extent is the chamfer value c.  c < eta1 accepts, c > eta2 rejects, and in between
    the opposite distance (template to moved source, over the representative's scale) decides against eta3.  An accepted
    instance gets T_obj = inv(T_rel) T_obj_representative and its box from get_obb; a rejected one moves, with its entries in
    all five dicts, to class cls_id + 100 (10000 for ScanNet ids), which is registered like a class on a later pass.
    -> {"chamfer", "chamfer_opposite", "representative"}: what each decision saw."""
    from .utils import get_obb, get_pose_from_pointcloud, get_possible_transform_from_bbox, transform_pointcloud
    solver = IcpSolver() if solver is None else solver
    dev = torch.device(device)
    sub_offset = 100 if name == "replica" else 10000
    per_class = (inst_dict, count_dict, bbox3d_dict, pe_dict, fc_occ_map_dict)
    symmetries = get_possible_transform_from_bbox() if multi_init_pose else [np.eye(4)]
    seen = {"chamfer": {}, "chamfer_opposite": {}, "representative": {}}
    while bbox3d_dict:
        for cls_id in list(bbox3d_dict.keys()):
            members = list(bbox3d_dict[cls_id].keys())
            counts = list(count_dict[cls_id].values())
            rep_at = int(np.argmax(counts)) if len(counts) > 1 else 0
            rep_id = members[rep_at]
            rep = inst_dict[cls_id][rep_id]
            rep["T_obj"], rep["bbox3D"] = get_pose_from_pointcloud(rep["pcs"], inst_id=rep_id)
            seen["representative"][cls_id] = rep_id
            seen["chamfer"][cls_id], seen["chamfer_opposite"][cls_id] = {}, {}
            others = members[:rep_at] + members[rep_at + 1:]
            if others:
                rep_frame, rep_scale = _unit_scale(rep["T_obj"])
                rep_pts = np.array(rep["pcs"].points)
                rep_dev = torch.from_numpy(rep_pts).to(dev)
                templates = torch.from_numpy(np.stack([transform_pointcloud(rep_pts, S).T for S in symmetries])).to(dev)
            for obj_id in others:
                src_pts = np.array(inst_dict[cls_id][obj_id]["pcs"].points)
                half_extent = float((src_pts.max(axis=0) - src_pts.min(axis=0)).max()) / 2
                R_all, t_all = solver(torch.from_numpy(src_pts.T[None].copy()).to(dev), templates)
                T_rel, dist = _best_candidate(src_pts, rep_dev, symmetries, R_all.detach().cpu().numpy(),
                                              t_all.detach().cpu().numpy(), dev)
                chamfer = dist / half_extent
                seen["chamfer"][cls_id][obj_id] = chamfer
                if eta1 <= chamfer <= eta2:
                    moved = torch.from_numpy(transform_pointcloud(src_pts, T_rel)).to(dev)
                    opposite = _mean_nn_distance(rep_dev, moved) / rep_scale
                    seen["chamfer_opposite"][cls_id][obj_id] = opposite
                    rejected = bool(opposite > eta3)
                else:
                    rejected = bool(chamfer > eta2)
                if rejected:
                    for d in per_class:
                        d.setdefault(cls_id + sub_offset, {})[obj_id] = d[cls_id].pop(obj_id)
                else:
                    entry = inst_dict[cls_id][obj_id]
                    entry["T_obj"] = np.linalg.inv(T_rel) @ rep_frame
                    get_obb(entry)
            del bbox3d_dict[cls_id]
    return seen


class _RegistrationPickler:
    """pickle.dump with utils.BoundingBox written under the reference's global name ``utils.BoundingBox``, so that the
    reference -- and dataset.load_registration_result -- can read the file"""

    @staticmethod
    def dump(obj, f):
        import pickle
        import sys
        import types
        from .utils import BoundingBox
        proxy = type("BoundingBox", (), {"__module__": "utils", "__qualname__": "BoundingBox"})
        mod = types.ModuleType("utils")
        mod.BoundingBox = proxy

        class P(pickle.Pickler):
            def reducer_override(self, o):
                if type(o) is BoundingBox:
                    return proxy, (), dict(o.__dict__)
                return NotImplemented

        saved = sys.modules.get("utils")
        sys.modules["utils"] = mod
        try:
            P(f, protocol=pickle.DEFAULT_PROTOCOL).dump(obj)
        finally:
            if saved is None:
                del sys.modules["utils"]
            else:
                sys.modules["utils"] = saved


def write_registration_result(inst_dict, path):
    """the cache file <dataset_dir>/inst_dict.pkl (src/dataset.py:87-88)"""
    with open(path, "wb") as f:
        _RegistrationPickler.dump(inst_dict, f)


def pretrain_fields(dataset, cfg, iters, boxes, encoders, fields, rays_per_step=None, seed=0):
    """The fields ``get_uncertainty_fields`` probes, trained here instead of loaded: every instance's OccupancyMap(32) +
    UniDirsEmbed for ``iters`` steps (object_fields.ObjectFieldTrainer, all objects per launch), written under
    ``cfg.weight_root/ckpt`` when that is set, and filled into the three dicts the way ``load_pretrained_fields`` fills them
    (``bbox`` = the oriented box of the instance's cloud).  -> the trainer"""
    from .object_fields import ObjectFieldTrainer
    from .utils import get_bound
    tr = ObjectFieldTrainer.from_dataset(dataset, cfg, rays_per_step=rays_per_step, seed=seed)
    tr.run(int(iters))
    for cls_id, entries in dataset.inst_dict.items():
        if cls_id == 0:
            continue
        for obj_id, entry in entries.items():
            pe, fc = tr.modules(obj_id)
            boxes.setdefault(cls_id, {})[obj_id] = get_bound(entry["pcs"]) if entry.get("pcs") is not None else None
            encoders.setdefault(cls_id, {})[obj_id] = pe.to(cfg.data_device)
            fields.setdefault(cls_id, {})[obj_id] = fc.to(cfg.data_device)
    if getattr(cfg, "weight_root", None):
        tr.save_checkpoints(cfg.weight_root, {o: b for per_cls in boxes.values() for o, b in per_cls.items()})
    return tr


def register_dataset(dataset, cfg, solver=None, tsdf=False, pretrain=None, rays_per_step=None):
    """src/dataset.py:72-88 for a dataset whose frames are loaded: get_all_poses -> get_uncertainty_fields -> align_poses, the
    'pcs' entries deleted, the result written to <root_dir>/inst_dict.pkl.  A ScanNet dataset needs tsdf=True, here and when it
    was loaded (get_dataset(cfg, register=True, tsdf=True): the loader gathers the objects' clouds only then).
    ``pretrain``: with registration.load_pretrained false, train the per-object fields for that many steps (``rays_per_step``
    rays each, default cfg.n_per_optim) instead of loading them (pretrain_fields); without it that case raises, as before."""
    if dataset.name != "replica" and not tsdf:
        raise NotImplementedError("registration of ScanNet sequences (TSDF fusion of the background, objects from refined "
                                  "masks on disk) runs only on request: tsdf=True")
    if dataset.name != "replica" and not getattr(dataset, "_accumulate", False):
        raise ValueError("register_dataset(tsdf=True): the ScanNet dataset was loaded without the objects' clouds; load it with "
                         "get_dataset(cfg, register=True, tsdf=True)")
    load_pretrained = bool(getattr(cfg, "load_pretrained", False))
    if not load_pretrained and pretrain is None:
        raise NotImplementedError("get_uncertainty_fields: registration.load_pretrained is false; only per-object checkpoints "
                                  "under registration.weight_root give the fields that rank a class's instances (the "
                                  "reference registers nothing in this case, without saying so)")
    inst_dict = dataset.inst_dict
    boxes, counts, encoders, fields = {}, {}, {}, {}
    get_all_poses(inst_dict, dataset.sample_dict, dataset.intrinsic_open3d, name=dataset.name, depth_scale=cfg.depth_scale,
                  max_depth=cfg.max_depth, tsdf=tsdf)
    if not load_pretrained:
        pretrain_fields(dataset, cfg, pretrain, boxes, encoders, fields, rays_per_step=rays_per_step)
    get_uncertainty_fields(inst_dict, boxes, counts, encoders, fields, cfg, name=dataset.name, load_pretrained=load_pretrained)
    etas = {k: getattr(cfg, k) for k in ("eta1", "eta2", "eta3") if hasattr(cfg, k)}
    align_poses(inst_dict, boxes, counts, encoders, fields, name=dataset.name,
                multi_init_pose=getattr(cfg, "multi_init_pose", True), device=dataset._parse_device(), solver=solver, **etas)
    for cls_id, entries in inst_dict.items():          # the clouds are intermediate results: not part of the cache
        for entry in ([entries] if cls_id == 0 else entries.values()):
            entry.pop("pcs", None)
    write_registration_result(inst_dict, os.path.join(dataset.root_dir, "inst_dict.pkl"))
