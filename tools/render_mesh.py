"""Renders triangle meshes (.obj / .ply, as vis.load_mesh reads them; an .obj written by Mesh.export keeps its colours and
normals) from one camera pose on the GPU (cnr_amd.raster, csrc/raster.hip) and writes rgb.png, depth.png (16 bit,
millimetres), instance.png (16 bit, the mesh's place on the command line, 65535 = nothing), normal.png (world-frame normal of the
winning face towards the camera, n * 0.5 + 0.5 in 8 bits) and shade.png (a grey headlight Lambert image) into --out.

The pose is camera-to-world: --pose FILE with a 4 x 4 matrix in text form, or --look-at EX EY EZ TX TY TZ (the camera at E,
its axis to T, world z up), or --config CFG --frame K, which takes the pose of dataset frame K and the intrinsics of the config.

    python tools/render_mesh.py --mesh rec.obj gt.ply --look-at 2 2 1.5 0 0 0 --intrinsics 640 480 500 500 319.5 239.5 --out view0
    python tools/render_mesh.py --mesh logs/room0/mesh.obj --config configs/Replica/config_replica_room0.json --frame 0 --out view0
        [--depth-range 0.05 20] [--normal face|vertex] [--cull-backfaces]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """T_wc of a camera at ``eye`` whose optical axis (+z) points at ``target``: x to the right, y down"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-9:                 # looking along `up`
        x = np.cross(z, np.array([0.0, 1.0, 0.0]))
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def load(path):
    """vis.load_mesh, or for an .obj with `v x y z r g b` / `vn` lines (Mesh.export) the mesh with its colours and normals"""
    from cnr_amd import vis
    if path.lower().endswith(".obj"):
        with open(path) as fh:
            first = next((line.split() for line in fh if line.startswith("v ")), [])
        if len(first) == 7:                      # x y z r g b
            v, c, n, f = vis.load_obj(path)
            m = vis.Mesh(v, f, n if len(n) == len(v) else None)
            m.visual.vertex_colors = np.round(np.clip(c, 0, 1) * 255)
            return m
    return vis.load_mesh(path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", nargs="+", required=True)
    ap.add_argument("--pose", help="a text file with T_wc (4 x 4)")
    ap.add_argument("--look-at", nargs=6, type=float, metavar=("EX", "EY", "EZ", "TX", "TY", "TZ"))
    ap.add_argument("--intrinsics", nargs=6, type=float, metavar=("W", "H", "FX", "FY", "CX", "CY"))
    ap.add_argument("--config", help="take the intrinsics and depth limits (and with --frame the pose) from this config's dataset")
    ap.add_argument("--frame", type=int, default=None)
    ap.add_argument("--depth-range", nargs=2, type=float, default=None, metavar=("ZMIN", "ZMAX"))
    ap.add_argument("--normal", choices=("face", "vertex"), default="face")
    ap.add_argument("--cull-backfaces", action="store_true")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import cnr_amd as cnr
    from cnr_amd import raster
    assert torch.cuda.is_available(), "render_mesh needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    T_wc = None
    if a.config:
        cfg = cnr.cfg.Config(a.config)
        W, H, fx, fy, cx, cy = cfg.W, cfg.H, cfg.fx, cfg.fy, cfg.cx, cfg.cy
        zmin, zmax = a.depth_range or (cfg.min_depth, cfg.max_depth)
        if a.frame is not None:
            T_wc = np.asarray(cnr.dataset.get_dataset(cfg).sample_dict[a.frame]["T"], np.float64)
    elif a.intrinsics:
        W, H, fx, fy, cx, cy = a.intrinsics
        zmin, zmax = a.depth_range or (0.05, 100.0)
    else:
        raise SystemExit("give --intrinsics W H FX FY CX CY or --config CFG")
    if a.pose:
        T_wc = np.loadtxt(a.pose).reshape(4, 4)
    elif a.look_at:
        T_wc = look_at(a.look_at[:3], a.look_at[3:])
    if T_wc is None:
        raise SystemExit("give --pose FILE, --look-at EX EY EZ TX TY TZ or --config CFG --frame K")
    rast = raster.MeshRasterizer.from_intrinsics(int(W), int(H), fx, fy, cx, cy, zmin, zmax, device=dev)
    scene = raster.MeshScene([load(p) for p in a.mesh], device=dev)
    result = rast.render(scene, T_wc, normal=a.normal, cull_backfaces=a.cull_backfaces)
    cnr.view.render_to_files(result, a.out)
    from PIL import Image
    grey = (cnr.view.shade(result, T_wc).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy().transpose(1, 0, 2)
    Image.fromarray(np.ascontiguousarray(grey), "RGB").save(os.path.join(a.out, "shade.png"))
    hit = int((result["face"] >= 0).sum())
    print("wrote rgb.png, depth.png, instance.png, normal.png, shade.png to {}; {} faces, {} of {} pixels hit".format(
        a.out, scene.n_faces, hit, int(W) * int(H)))


if __name__ == "__main__":
    main()
