"""3-D metrics of the reconstructed meshes (metric/eval_3D_obj.py's command line and output files), on cnr_amd.metrics:

    python tools/eval_3d_obj.py --data_dir Datasets/Replica --log_dir logs/Replica [--log_dir_ref DIR] [--iteration 10000]
                                [--clean keep_largest=1,...] [--surface [--index]] [--volume [N] [--repair]]

For every scene of the dataset (the last component of --data_dir: Replica or ScanNet) whose <log_dir>/<scene>/scene_mesh exists,
every object mesh iteration_<it>_obj<id>.obj written by train.py is scored against its ground-truth mesh in
<data_dir>/<scene>/habitat (Replica: mesh_semantic.ply_<id>.ply; ScanNet: <scene>_vh_clean_2.ply_<id>.ply): accuracy and
completion in cm, completion ratio at 5 cm in %.  Written: <log_dir>/<scene>/eval_mesh/metric_obj<id>.npy ((3,1)) and
metrics_3D_obj.npy ((3, objects, 1)).  N = 10 000 samples per object, 200 000 for the background (id 0, whose ground truth is
the union of the background classes' meshes) -- as in the reference, id 0 is left out where the ids are parsed from the file
names.  A --log_dir_ref mesh it_<it>_obj<id>.obj, where present, sets the crop box instead of the ground truth.
Differences from the reference: only the meshes of --iteration are listed (the reference lists every .obj and then opens
the --iteration one), scenes without a scene_mesh directory are skipped, and the samples are seeded (cnr_amd.metrics).
--clean (default off; the reference scores the mesh as it is) drops the reconstruction's floaters first: the options of
cnr_amd.meshops.clean_mesh as name=value pairs, e.g. keep_largest=1 or min_area_fraction=0.01,weld=0.
--surface (default off) adds cnr_amd.metrics.calc_3d_metric_surface per object and in the mean: the same samples measured
against the other MESH (accuracy, completion, completion ratio), precision / recall / F-score at 5 cm and normal
consistency; written to <log_dir>/<scene>/eval_mesh/metrics_3D_obj_surface.json.
--volume [N] (default off; N = 100 000 points when not given) adds cnr_amd.metrics.volume_iou of the reconstruction and the
ground truth per object and in the mean, counted in mesh_ref's oriented box, the one accuracy is clipped to (so what the
reconstruction has outside that box counts for nothing); each mesh's orientation is found by mesh_orientation, or with
--repair each mesh's bit-equal vertices are welded and it goes through cnr_amd.meshops.orient (consistent winding per patch,
patches outward; volume_iou's orientation "repair").  Written to
<log_dir>/<scene>/eval_mesh/metrics_3D_obj_volume.json.  An object with no point inside either mesh has no IoU: it is printed
as "none", written as null and left out of the mean (objects_in_mean counts the rest).  The background (id 0), a room seen
from inside, has no volume to compare; it is never listed (see above), so it gets no IoU either."""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPLICA_BG = [5, 12, 30, 31, 40, 60, 92, 93, 95, 97, 98, 79]
REPLICA_SCENES = ["room_0", "room_1", "room_2", "office_0", "office_1", "office_2", "office_3", "office_4"]
SCANNET_BG = [-1, 0, 1, 3, 16, 41, 232, 21, 161, 128, 21]
SCANNET_SCENES = ["scene0013_02", "scene0059_00", "scene0066_00", "scene0281_00"]
SURFACE_COLUMNS = ["accuracy_cm", "completion_cm", "completion_ratio", "precision", "recall", "fscore",
                   "normal_consistency_acc", "normal_consistency_comp", "normal_consistency"]
VOLUME_COLUMNS = ["iou", "volume_a", "volume_b"]


def _fmt(value):
    return "none" if value is None else "%.4f" % value


def concatenate(meshes):
    from cnr_amd.vis import Mesh
    v, f, n = [], [], 0
    for m in meshes:
        v.append(m.vertices)
        f.append(m.faces + n)
        n += len(m.vertices)
    return Mesh(np.concatenate(v) if v else np.zeros((0, 3)), np.concatenate(f) if f else np.zeros((0, 3), np.int64))


def get_gt_bg_mesh(gt_dir, background_cls_list):
    from cnr_amd.vis import load_mesh
    with open(os.path.join(gt_dir, "info_semantic.json")) as f:
        objects = json.load(f)["objects"]
    return concatenate([load_mesh(os.path.join(gt_dir, "mesh_semantic.ply_%d.ply" % int(o["id"])))
                        for o in objects if int(o["class_id"]) in background_cls_list])


def read_label_mapping(filename, label_from="raw_category", label_to="id"):
    mapping = {}
    with open(filename) as f:
        for row in csv.DictReader(f, delimiter="\t"):
            mapping[row[label_from]] = int(row[label_to])
    try:
        return {int(k): v for k, v in mapping.items()}
    except ValueError:
        return mapping


def get_gt_bg_mesh_scannet(gt_dir, exp, background_cls_list, label_map_file):
    from cnr_amd.vis import load_mesh
    label_map = read_label_mapping(label_map_file)
    with open(os.path.join(gt_dir, exp + ".aggregation.json")) as f:
        groups = json.load(f)["segGroups"]
    meshes = [load_mesh(os.path.join(gt_dir, "%s_vh_clean_2.ply_%d.ply" % (exp, int(g["id"]) + 2)))
              for g in groups if label_map[g["label"]] in background_cls_list]
    # the label table has no row for "unknown" (instance 0): always part of the background
    meshes.append(load_mesh(os.path.join(gt_dir, exp + "_vh_clean_2.ply_0.ply")))
    return concatenate(meshes)


def get_obj_ids(obj_dir, iteration):
    ids = set()
    for name in os.listdir(obj_dir):
        m = re.fullmatch(r"iteration_%d_obj(\d+)\.obj" % iteration, name)
        if m and int(m.group(1)) != 0:
            ids.add(int(m.group(1)))
    return sorted(ids)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_dir", default="Datasets/Replica", type=str)
    ap.add_argument("--log_dir", default="logs/Replica", type=str)
    ap.add_argument("--log_dir_ref", default="", type=str)
    ap.add_argument("--iteration", default=10000, type=int)
    ap.add_argument("--clean", default=None, help="drop floaters first: clean_mesh options as name=value,... e.g. keep_largest=1,min_faces=20 (default: off)")
    ap.add_argument("--surface", action="store_true", help="also score against the meshes themselves: point-to-mesh distances, F-score, normal consistency (default: off)")
    ap.add_argument("--index", action="store_true", help="with --surface: take the point-to-mesh distances through a tile-box index of each mesh; the same numbers, faster on large meshes (default: off)")
    ap.add_argument("--volume", nargs="?", type=int, const=100000, default=None, metavar="N", help="also the volumetric IoU of reconstruction and ground truth from N points (100000 when N is not given) in the crop box, by winding numbers (default: off)")
    ap.add_argument("--repair", action="store_true", help="with --volume: repair both meshes' orientation first (consistent winding per patch, patches outward) instead of trusting it (default: off)")
    args = ap.parse_args(argv)
    if args.repair and args.volume is None:
        ap.error("--repair goes with --volume")
    from cnr_amd.meshops import clean_mesh, parse_clean_options
    from cnr_amd.metrics import calc_3d_metric, calc_3d_metric_surface, oriented_bounds, volume_iou
    clean = parse_clean_options(args.clean) if args.clean else None
    from cnr_amd.vis import load_mesh

    dataset = os.path.basename(os.path.normpath(args.data_dir))
    if dataset == "Replica":
        bg_cls, scenes = REPLICA_BG, REPLICA_SCENES
    elif dataset == "ScanNet":
        bg_cls, scenes = SCANNET_BG, SCANNET_SCENES
        label_map_file = os.path.join(args.data_dir, "scannetv2-labels.combined.tsv")
    else:
        raise SystemExit(f"Dataset {dataset} is not supported (Replica, ScanNet)")

    for exp in scenes:
        gt_dir = os.path.join(args.data_dir, exp, "habitat")
        exp_dir = os.path.join(args.log_dir, exp)
        mesh_dir = os.path.join(exp_dir, "scene_mesh")
        mesh_dir_ref = os.path.join(args.log_dir_ref, exp, "scene_mesh")
        if not os.path.isdir(mesh_dir):
            print(f"skip {exp}: no {mesh_dir}")
            continue
        output_path = os.path.join(exp_dir, "eval_mesh")
        os.makedirs(output_path, exist_ok=True)
        metrics_3D = [[] for _ in range(3)]
        surface, volume = {}, {}
        for obj_id in get_obj_ids(mesh_dir, args.iteration):
            if obj_id == 0:
                N = 200000
                mesh_gt = (get_gt_bg_mesh(gt_dir, bg_cls) if dataset == "Replica"
                           else get_gt_bg_mesh_scannet(gt_dir, exp, bg_cls, label_map_file))
            else:
                N = 10000
                mesh_gt = load_mesh(os.path.join(gt_dir, "mesh_semantic.ply_%d.ply" % obj_id) if dataset == "Replica"
                                    else os.path.join(gt_dir, "%s_vh_clean_2.ply_%d.ply" % (exp, obj_id)))
            mesh_rec = load_mesh(os.path.join(mesh_dir, "iteration_%d_obj%d.obj" % (args.iteration, obj_id)))
            if clean is not None:
                mesh_rec, report = clean_mesh(mesh_rec, **clean)
                print("obj %d: kept %d of %d components, %d of %d faces" % (obj_id, report["n_kept"], report["n_components"],
                                                                           report["faces_out"], report["faces_in"]))
            ref_file = os.path.join(mesh_dir_ref, "it_%d_obj%d.obj" % (args.iteration, obj_id))
            mesh_ref = load_mesh(ref_file) if os.path.exists(ref_file) else mesh_gt
            metrics = calc_3d_metric(mesh_rec, mesh_ref, N=N, mesh_gt=mesh_gt)
            if metrics is None:
                continue
            np.save(os.path.join(output_path, "metric_obj%d.npy" % obj_id), np.array(metrics))
            for k in range(3):
                metrics_3D[k].append(metrics[k])
            if args.surface:
                row = calc_3d_metric_surface(mesh_rec, mesh_ref, N=N, mesh_gt=mesh_gt, index=args.index)
                if row is not None:
                    surface[obj_id] = row
                    print("surface obj %d: " % obj_id + "  ".join("%s %.4f" % (k, row[k]) for k in SURFACE_COLUMNS))
            if args.volume is not None:
                pair, orientation = (mesh_rec, mesh_gt), ("auto", "auto")
                if args.repair:                 # a file holds a vertex once per polygon side: weld, or every side is a patch
                    pair, orientation = [clean_mesh(m, weld=0.0)[0] for m in pair], ("repair", "repair")
                volume[obj_id] = row = volume_iou(*pair, N=args.volume, box=oriented_bounds(mesh_ref), orientation=orientation)
                if row["union"] == 0:           # no point inside either mesh: no IoU (None: JSON has no nan), not in the mean
                    row["iou"] = None
                print("volume obj %d: " % obj_id + "  ".join("%s %s" % (k, _fmt(row[k])) for k in VOLUME_COLUMNS))
        metrics_3D = np.array(metrics_3D)
        np.save(os.path.join(output_path, "metrics_3D_obj.npy"), metrics_3D)
        print("metrics 3D obj \n Acc | Comp | Comp Ratio 5cm \n", metrics_3D.mean(axis=1) if metrics_3D.size else metrics_3D)
        if args.surface:
            mean = {k: float(np.mean([r[k] for r in surface.values()])) for k in SURFACE_COLUMNS} if surface else {}
            with open(os.path.join(output_path, "metrics_3D_obj_surface.json"), "w") as f:
                json.dump(dict(objects={str(k): v for k, v in surface.items()}, mean=mean), f, indent=1)
            print("surface mean: " + "  ".join("%s %.4f" % (k, mean[k]) for k in SURFACE_COLUMNS))
        if args.volume is not None:
            scored = [r for r in volume.values() if r["iou"] is not None]
            mean = {k: float(np.mean([r[k] for r in scored])) for k in VOLUME_COLUMNS} if scored else {}
            with open(os.path.join(output_path, "metrics_3D_obj_volume.json"), "w") as f:
                json.dump(dict(points=args.volume, objects={str(k): v for k, v in volume.items()}, mean=mean,
                               objects_in_mean=len(scored)), f, indent=1, allow_nan=False)
            print("volume mean: " + ("  ".join("%s %.4f" % (k, mean[k]) for k in VOLUME_COLUMNS) if scored else "no objects"))
        print("-----------------------------------------")
        print("finish exp ", exp)


if __name__ == "__main__":
    main()
