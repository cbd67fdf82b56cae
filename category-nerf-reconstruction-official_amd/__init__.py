"""MI355X-native volumetric-rendering train-step hot path for category-level neural fields.

Mirrors the reference's call surface (flat modules of /src): ``trainer``, ``scene_cateogries``,
``embedding``, ``model``, ``render_rays``, ``loss``, ``utils.update_vmap`` -- backed by hand-written
gfx950 HIP kernels behind a C-ABI (include/cnr_hip.h, libcnr_hip.so).  ``fused`` holds the
single-launch fast path, ``stepgraph`` the one scheduler of its hipGraph launches, ``background`` the capturable background branch / whole-iteration graph, ``parallel`` the
multi-GPU sharding, ``category_registration`` the forward-only uncertainty probe and ``vis`` the GPU marching cubes, ``metrics`` the mesh evaluation, ``dataset`` the Replica / ScanNet loaders, ``teaser_utils`` the reference's TEASER + FPFH + ICP surface, ``view`` the scene view renderer, ``devmesh`` the one upload and index check of a triangle mesh, ``raster`` the mesh rasteriser,``meshops`` the mesh clean-up (welding, connected components, floaters), ``image_metrics`` the image-space view scores (PSNR, SSIM, depth L1, mask IoU).  Import as ``cnr_amd`` (see
cnr_amd.py at the repo root; the directory name carries a hyphen).
"""
from . import _C, ops  # noqa: F401
from . import cfg, embedding, model, render_rays, loss, trainer, utils, scene_cateogries, stepgraph, fused, parallel, background, category_registration, vis, metrics, dataset, teaser_utils, view, pool_step, object_fields, code_fit, devmesh, raster, meshops, image_metrics  # noqa: F401

__version__ = "0.1.0"
