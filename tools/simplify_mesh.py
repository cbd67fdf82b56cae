"""Make a mesh smaller on the GPU: uniform vertex clustering with quadric placement (cnr_amd.meshops.simplify_mesh; DESIGN.md
§3.19), and print the report.

    python tools/simplify_mesh.py in.{obj,ply} out.obj (--cell C | --faces N) [--placement quadric|mean|representative] [--tau T]
                                  [--deviation [N] [--index]]

--cell C clusters the vertices on a grid of pitch C; --faces N bisects the pitch until at most N faces are left.  An output
vertex is placed by its cluster's quadric (the default), at the cluster mean, or at the cluster's lowest input vertex; it takes
that vertex's colour, and its normal from the output faces.  --deviation [N] (default off) also measures the output against
the input: the two-sided mean / RMS / Hausdorff distance (cnr_amd.meshops.deviation_mesh: both meshes' vertices and N
area-weighted samples each, default 100 000, to the other surface), absolute and as a fraction of the input's diagonal."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clean_mesh import load  # noqa: E402


def print_report(report):
    print("cell: %.9g  clusters: %d  clamped: %d" % (report["cell"], report["clusters"], report["clamped"]))
    print("faces %d -> %d (collapsed %d, duplicate %d), vertices out: %d" % (report["faces_in"], report["faces_out"], report["faces_collapsed"],
                                                                            report["faces_duplicate"], report["vertices_out"]))
    print("quadric error: %.9g" % report["quadric_error"])
    for cell, n in report["search"]:
        print("  tried cell %.9g -> %d faces" % (cell, n))


def print_deviation(dev):
    diag = dev["diag"] or 1.0
    for key, name in (("a_to_b", "input -> output"), ("b_to_a", "output -> input")):
        d = dev[key]
        print("deviation %s: mean %.6g  rms %.6g  max %.6g  (%d points; of the diagonal: %.4g %.4g %.4g)"
              % (name, d["mean"], d["rms"], d["max"], d["n"], d["mean"] / diag, d["rms"] / diag, d["max"] / diag))
    print("hausdorff: %.6g  (%.4g of the diagonal %.6g)" % (dev["hausdorff"], dev["hausdorff"] / diag, dev["diag"]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--cell", type=float, default=None)
    how.add_argument("--faces", type=int, default=None)
    ap.add_argument("--placement", default="quadric", choices=("quadric", "mean", "representative"))
    ap.add_argument("--tau", type=float, default=1e-3)
    ap.add_argument("--deviation", type=int, nargs="?", const=100000, default=None, metavar="N",
                    help="measure the output against the input with N samples per side (default: off)")
    ap.add_argument("--index", action="store_true",
                    help="with --deviation: distances through a tile-box index of each mesh; the same numbers (default: off)")
    a = ap.parse_args(argv)
    import cnr_amd as cnr
    mesh = load(cnr, a.src)
    out, report = cnr.meshops.simplify_mesh(mesh, cell=a.cell, target_faces=a.faces, placement=a.placement, tau=a.tau)
    print_report(report)
    if a.deviation is not None and len(out.faces) and len(mesh.faces):
        print_deviation(cnr.meshops.deviation_mesh(mesh, out, samples=a.deviation, index=a.index))
    out.export(a.dst)


if __name__ == "__main__":
    main()
