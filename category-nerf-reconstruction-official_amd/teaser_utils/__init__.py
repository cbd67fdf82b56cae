"""The reference's ``src/teaser_utils`` surface on this package's kernels: ``helpers`` (pcd2xyz, extract_fpfh,
find_correspondences, Rt2T) and ``teaser_fpfh_icp`` (teaser_fpfh_icp, TEASER_FPFH_ICP).  DESIGN.md §3.9."""
from . import helpers, teaser_fpfh_icp  # noqa: F401
