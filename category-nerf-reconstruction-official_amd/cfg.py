"""Config reader, same attribute names as the reference's ``cfg.Config`` (src/cfg.py:6-97).  The dataset, distortion and
registration keys are read when present (the dataset loaders use them); a JSON without them gives the hot path's keys only."""
import json
import os

import numpy as np


class Config:
    def __init__(self, config_file):
        with open(config_file) as f:
            config = json.load(f)
        tr, rd, md, op = config["trainer"], config["render"], config["model"], config["optimizer"]["args"]
        self.training_device, self.data_device = tr["train_device"], tr["data_device"]
        self.max_n_models, self.max_iter = tr["n_models"], tr["max_iter"]
        self.save_iter, self.log_iter = tr["save_iter"], tr["log_iter"]
        self.depth_scale = 1 / tr["scale"]
        self.min_depth, self.max_depth = rd["depth_range"][0], rd["depth_range"][1]
        cam = config["camera"]
        self.mh, self.mw, self.height, self.width = cam["mh"], cam["mw"], cam["h"], cam["w"]
        self.H, self.W = self.height - 2 * self.mh, self.width - 2 * self.mw
        if "fx" in cam:
            self.fx, self.fy = cam["fx"], cam["fy"]
            self.cx, self.cy = cam["cx"] - self.mw, cam["cy"] - self.mh
        ds = config.get("dataset", {})
        if "format" in ds:
            self.dataset_format = ds["format"]
        if "path" in ds:
            self.dataset_dir = ds["path"]
            intrinsic_file = os.path.join(self.dataset_dir, "intrinsic/intrinsic_depth.txt")
            if "fx" not in cam and os.path.exists(intrinsic_file):     # ScanNet (src/cfg.py:38-43)
                from .utils import load_matrix_from_txt
                intrinsic = load_matrix_from_txt(intrinsic_file)
                self.fx, self.fy = intrinsic[0, 0], intrinsic[1, 1]
                self.cx, self.cy = intrinsic[0, 2] - self.mw, intrinsic[1, 2] - self.mh
        if "distortion" in cam:
            self.distortion_array = np.array(cam["distortion"])
        elif "k1" in cam:
            self.distortion_array = np.array([cam[k] for k in ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")])
        else:
            self.distortion_array = None
        if getattr(self, "dataset_format", None) == "ScanNet" and "use_refined_mask" in ds:
            self.use_refined_mask = ds["use_refined_mask"]
            self.load_refined_mask = ds["load_refined_mask"] and self.use_refined_mask
        reg = config.get("registration", {})
        for key in ("load_registration_result", "load_pretrained", "weight_root", "multi_init_pose", "eta1", "eta2", "eta3"):
            if key in reg:
                setattr(self, key, reg[key])
        self.n_per_optim, self.n_per_optim_bg = rd["n_per_optim"], rd["n_per_optim_bg"]
        self.obj_scale, self.bg_scale = md["obj_scale"], md["bg_scale"]
        self.hidden_feature_size, self.hidden_feature_size_bg = md["hidden_feature_size"], md["hidden_feature_size_bg"]
        self.n_bins_cam2surface, self.n_bins_cam2surface_bg = rd["n_bins_cam2surface"], rd["n_bins_cam2surface_bg"]
        self.n_bins = rd["n_bins"]
        self.n_unidir_funcs = md["n_unidir_funcs"]
        self.surface_eps, self.stop_eps = md["surface_eps"], md["other_eps"]
        self.net_hyperparams = md["net_hyperparams"]
        self.learning_rate, self.code_learning_rate = op["lr"], op["code_lr"]
        self.weight_decay, self.code_weight_decay = op["weight_decay"], op["code_weight_decay"]
        vis = config.get("vis", {})           # meshing cadence and resolution (src/cfg.py:81-83), when present
        for key in ("live_voxel_size", "grid_dim", "mesh_it"):
            if key in vis:
                setattr(self, key, vis[key])


def synthetic_config(device="cuda:0", latent_dim=256, obj_scale=2.0, n_bins_cam2surface=8, n_bins=56):
    """The Replica room_0 model/optimiser settings (configs/Replica/config_replica_room0.json) with the
    sample split of a synthetic scale-up; no file needed."""
    c = object.__new__(Config)
    c.training_device = c.data_device = device
    c.max_n_models, c.max_iter, c.save_iter, c.log_iter = 100, 10001, 2000, 100
    c.min_depth, c.max_depth = 0.0, 8.0
    c.W, c.H, c.fx, c.fy, c.cx, c.cy = 1200, 680, 600.0, 600.0, 599.5, 339.5
    c.n_per_optim, c.n_per_optim_bg = 120, 1200
    c.obj_scale, c.bg_scale = obj_scale, 5.0
    c.hidden_feature_size, c.hidden_feature_size_bg = 32, 128
    c.n_bins_cam2surface, c.n_bins_cam2surface_bg, c.n_bins = n_bins_cam2surface, 5, n_bins
    c.n_unidir_funcs = 5
    c.surface_eps, c.stop_eps = 0.1, 0.05
    c.net_hyperparams = dict(shape_blocks=2, texture_blocks=1, W=32, latent_dim=latent_dim)
    c.learning_rate = c.code_learning_rate = 0.001
    c.weight_decay = c.code_weight_decay = 0.013
    c.grid_dim, c.live_voxel_size, c.mesh_it = 256, 0.005, 10000
    return c
