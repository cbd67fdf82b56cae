#!/usr/bin/env python3
"""Record what the reference's own refine_inst_data (src/utils.py:696-721) returns on the cases of tests/geoseg_cpu.py
refine_cases() -> tests/golden/geoseg/refine_cases.npz.  Build container only: the reference's utils module is imported from
the directory given on the command line (or $CNR_REFERENCE_SRC), with the five packages it imports at module scope and never
touches on this path (cv2, imgviz, open3d, trimesh, plotly) replaced by MagicMock.  Only arrays are written.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_geoseg_golden.py <reference>/src
"""
import contextlib
import io
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.dont_write_bytecode = True


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.environ["CNR_REFERENCE_SRC"]
    sys.path.insert(0, src)
    for m in ["cv2", "imgviz", "open3d", "trimesh", "plotly", "plotly.graph_objs", "plotly.subplots"]:
        sys.modules[m] = MagicMock()
    import utils as ref_utils
    import geoseg_cpu as G
    out = {}
    for name, (inst, masks) in G.refine_cases().items():
        with contextlib.redirect_stdout(io.StringIO()):
            refined = ref_utils.refine_inst_data(inst.copy(), [m.copy() for m in masks])
        assert refined.dtype == inst.dtype and refined.shape == inst.shape
        out[name + "__inst"], out[name + "__masks"], out[name + "__refined"] = inst, masks, refined
        print(name, "ids", np.unique(refined).tolist(), "assigned pixels", int((refined != 0).sum()))
    path = os.path.join(HERE, "geoseg", "refine_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
