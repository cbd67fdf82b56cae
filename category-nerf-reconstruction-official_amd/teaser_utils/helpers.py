"""The names of the reference's teaser_utils.helpers, on csrc/fpfh.hip.  Descriptors and correspondences come
back as numpy arrays, as the reference's do; category_registration holds the device-side forms."""
import numpy as np
import torch

from .. import category_registration as CR


def pcd2xyz(pcd):
    """a cloud's points as a (3,n) float64 numpy array, one point per column"""
    return np.ascontiguousarray(np.asarray(pcd.points, np.float64).T)


def extract_fpfh(pcd, voxel_size):
    """normals from the neighbours within 2 voxel_size (at most 30), FPFH from those within 5 voxel_size (at most 100); fills
    pcd.normals -> (n,33) float64 numpy"""
    return CR.extract_fpfh_device(pcd, voxel_size).cpu().numpy()


def find_correspondences(feats0, feats1, mutual_filter=True):
    """-> (idx0, idx1) int64 numpy: feats0[idx0[k]] <-> feats1[idx1[k]], mutual nearest neighbours with mutual_filter"""
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda f: f if torch.is_tensor(f) and f.is_cuda else torch.as_tensor(np.ascontiguousarray(f)).to(dev)
    i0, i1 = CR.mutual_correspondences(up(feats0), up(feats1), mutual_filter=mutual_filter)
    return i0.cpu().numpy(), i1.cpu().numpy()


def Rt2T(R, t):
    """(3,3) rotation and 3 translation values -> the (4,4) float64 rigid transform [R | t]"""
    return np.block([[np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)],
                     [np.zeros((1, 3)), np.ones((1, 1))]])
