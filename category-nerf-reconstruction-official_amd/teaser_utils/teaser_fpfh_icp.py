"""The names and shapes of the reference's teaser_utils.teaser_fpfh_icp: down-sample, correspondences (FPFH and mutual nearest
neighbours, or with spc=True all pairs sub-sampled to 10 000), the TEASER stages and ICP of
category_registration.FpfhTeaserSolver / TeaserSolver."""
import numpy as np
import torch

from .. import category_registration as CR
from .helpers import Rt2T, extract_fpfh, find_correspondences, pcd2xyz  # noqa: F401  (the reference's module exports them too)


def _solver(voxel_size, spc):
    # spc: the reference's noise bound is 0.01 whatever the voxel size, and 10 000 correspondences; otherwise voxel_size
    return CR.TeaserSolver(voxel_size=voxel_size, noise_bound=0.01, max_correspondences=10000) if spc else \
        CR.FpfhTeaserSolver(voxel_size=voxel_size)


def _host_columns(points):
    """(3,n) tensor or array -> (n,3) float64 numpy"""
    a = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    return np.ascontiguousarray(a.astype(np.float64).T)


def _solve(source_points, target_points, voxel_size, spc, visualize):
    """-> (T (4,4) float64 numpy: source -> target, the solver's info)"""
    solver = _solver(voxel_size, spc)
    on_gpu = torch.is_tensor(source_points) and source_points.is_cuda
    T, info = solver.solve_one(_host_columns(source_points), _host_columns(target_points), source_points.device if on_gpu else None)
    if visualize:                     # the count before any sub-sampling, as the reference prints it; nothing is drawn
        print(f"FPFH generates {info.get('candidates', info['N'])} putative correspondences.")
    return np.asarray(T, np.float64), info


def teaser_fpfh_icp(source_points, target_points, voxel_size=0.05, spc=False, visualize=False):
    """source_points (3,n), target_points (3,m) -> (rotation (3,3), translation (3,1)) float64 tensors: source -> target.
    visualize=True prints the number of putative correspondences."""
    T = torch.from_numpy(_solve(source_points, target_points, voxel_size, spc, visualize)[0])
    return T[:3, :3], T[:3, 3:4]


class TEASER_FPFH_ICP():
    """TEASER (correspondences from FPFH, or all pairs with spc=True) + ICP of one source against a batch of targets:
    TEASER_FPFH_ICP(source (1,3,m)).forward(targets (B,3,n)) -> (R (B,3,3), t (B,3,1)), float32 on the source's device as the
    reference returns them.  A target column with a coordinate that is exactly 0 counts as padding and is dropped, which is the
    reference's rule.  last_info: after forward, the solver's info per target (N, clique_size, correspondences, ...)."""

    def __init__(self, source_points, voxel_size=0.05, spc=False, visualize=False):
        self.source_points, self.voxel_size, self.spc, self.visualize = source_points, voxel_size, spc, visualize
        self.last_info = None

    def forward(self, target_points):
        source = self.source_points.reshape(3, -1)
        poses, self.last_info = [], []
        for target in target_points:
            kept = target[:, (target != 0).all(dim=0)]
            T, info = _solve(source, kept, self.voxel_size, self.spc, self.visualize)
            poses.append(T)
            self.last_info.append(info)
        T = torch.from_numpy(np.stack(poses) if poses else np.zeros((0, 4, 4))).to(device=self.source_points.device, dtype=torch.float32)
        return T[:, :3, :3].contiguous(), T[:, :3, 3:4].contiguous()
