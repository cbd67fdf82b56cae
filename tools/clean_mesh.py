"""Drop the floaters of a mesh on the GPU (cnr_amd.meshops.clean_mesh) and print its component table.

    python tools/clean_mesh.py in.{obj,ply} out.obj [--weld CELL] [--connectivity edge|vertex] [--keep_largest K]
                               [--min_faces N] [--min_area A] [--min_diag D] [--min_area_fraction Q] [--largest_by area|faces|diag]
                               [--orient]

--orient then makes the winding of what is kept consistent and every patch outward (cnr_amd.meshops.orient) and
prints the patch table.  --weld 0 welds bit-equal vertices first, --weld CELL those that round to the same point of a grid of that pitch.  A component is
kept when it passes every threshold (>=) and, with --keep_largest K, is among the K largest of those; ties go to the lower
component id, and the output is never empty unless the input is.  A file written by Mesh.export keeps its colours and normals;
any other .obj / .ply is read for its geometry."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load(cnr, path):
    """a Mesh.export file with its colours and normals, anything else through load_mesh"""
    import numpy as np
    if path.lower().endswith(".obj"):
        try:
            v, col, vn, f = cnr.vis.load_obj(path)
            if len(vn) == len(v) and len(v):
                mesh = cnr.vis.Mesh(v, f, vn)
                mesh.visual.vertex_colors = np.rint(col * 255.0)
                return mesh
        except (ValueError, IndexError):
            pass
    return cnr.vis.load_mesh(path)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--weld", type=float, default=None)
    ap.add_argument("--connectivity", default="edge", choices=("edge", "vertex"))
    ap.add_argument("--keep_largest", type=int, default=None)
    ap.add_argument("--min_faces", type=int, default=0)
    ap.add_argument("--min_area", type=float, default=0.0)
    ap.add_argument("--min_diag", type=float, default=0.0)
    ap.add_argument("--min_area_fraction", type=float, default=0.0)
    ap.add_argument("--largest_by", default="area", choices=("area", "faces", "diag"))
    ap.add_argument("--orient", action="store_true", help="repair the orientation of what is kept: consistent winding per patch, "
                                                          "patches outward (meshops.orient); prints the patch table")
    a = ap.parse_args(argv)
    import cnr_amd as cnr
    mesh = load(cnr, a.src)
    out, report = cnr.meshops.clean_mesh(mesh, weld=a.weld, connectivity=a.connectivity, keep_largest=a.keep_largest,
                                         min_faces=a.min_faces, min_area=a.min_area, min_diag=a.min_diag,
                                         min_area_fraction=a.min_area_fraction, largest_by=a.largest_by, orient=a.orient)
    table = report["components"]
    print(table.table())
    print("components: %d  kept: %d (%s)" % (report["n_components"], report["n_kept"],
                                             " ".join(str(c) for c in report["kept"].nonzero()[0])))
    print("boundary edges: %d  non-manifold edges: %d" % (table.boundary_edges, table.nonmanifold_edges))
    print("faces %d -> %d, vertices %d -> %d" % (report["faces_in"], report["faces_out"], report["vertices_in"], report["vertices_out"]))
    if a.orient:
        patches = report["orientation"]
        print(patches.table())
        print("patches: %d  not orientable: %d  faces flipped: %d" % (patches.n, int((~patches.orientable).sum()),
                                                                      int(patches.n_flipped.sum())))
    out.export(a.dst)


if __name__ == "__main__":
    main()
