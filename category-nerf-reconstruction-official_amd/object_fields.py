"""Registration's per-object fields, trained here: one vMAP-style ``OccupancyMap(hidden 32)`` + ``UniDirsEmbed`` per object -- the
fields ``category_registration.get_uncertainty_fields`` probes to rank the instances of a class, which the reference only ever
loads from ``<weight_root>/ckpt/<obj_id>/*.pth`` (its README points to a download for them).

Per object the step is the reference's background branch (train.py:113-121,172-184; ``sample_3d_points``, ``step_batch_loss`` with
one class, AdamW) at width 32 on the object's own ray pool.  All objects of a scene train together: ONE launch of cnr_obj_train
(csrc/obj_fused.hip) is one step of every object -- one workgroup per object, rows, draws, cursor, epoch and optimiser step on the
device -- so a captured graph of steps replays unchanged for ever and nothing in a step waits for the host.

Coordinates: the fields take WORLD coordinates divided by ``cfg.obj_scale``, which is what the probe feeds them
(src/category_registration.py:143-148); vMAP itself centres its objects ("Per-object fields")."""
import copy
import os

import torch

from . import _C, pool_step
from .pool_step import next_state          # (the state rule: one definition for both kernels' trainers)  # noqa: F401

HIDDEN = 32
PARAM_NAMES = ["in_layer.0.weight", "in_layer.0.bias", "mid1.0.0.weight", "mid1.0.0.bias", "cat_layer.0.weight",
               "cat_layer.0.bias", "mid2.0.0.weight", "mid2.0.0.bias", "out_alpha.weight", "out_alpha.bias",
               "color_linear.0.weight", "color_linear.0.bias", "out_color.weight", "out_color.bias"]
PARAM_COUNT = 11363          # cnr_obj_param_count(): the 14 tensors above at width 32, then B_layer.weight (21,3)
CKPT_KEYS = ("FC_state_dict", "PE_state_dict", "obj_scale", "bbox")


def checkpoint_path(weight_root, obj_id, steps):
    return os.path.join(weight_root, "ckpt", str(obj_id), "obj_{}_it_{:05d}.pth".format(obj_id, int(steps)))


def checkpoint_dict(pe, fc_occ_map, obj_scale, bbox):
    """what ``category_registration.load_pretrained_fields`` reads (src/category_registration.py:64-92)"""
    cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
    return {"FC_state_dict": cpu(fc_occ_map.state_dict()), "PE_state_dict": cpu(pe.state_dict()), "obj_scale": float(obj_scale),
            "bbox": bbox}


def _check(cfg, pools, obj_ids, R):
    if int(cfg.hidden_feature_size) != HIDDEN:
        raise NotImplementedError(f"ObjectFieldTrainer: cnr_obj_train is built for hidden_feature_size {HIDDEN} (the per-object "
                                  f"fields of every shipped config), not {cfg.hidden_feature_size}")
    if not obj_ids:
        raise ValueError("ObjectFieldTrainer: no object")
    if cfg.n_bins_cam2surface + cfg.n_bins > 64:
        raise NotImplementedError("ObjectFieldTrainer: at most 64 samples per ray")
    for obj_id in obj_ids:
        rows = int(pools[obj_id]["depth"].shape[0])
        if rows < R:
            raise ValueError(f"ObjectFieldTrainer: object {obj_id} has a pool of {rows} rows, fewer than the {R} rays of a step")


class ObjectFieldTrainer(pool_step.StepBranch):
    def __init__(self, cfg, pools, obj_ids, rays_per_step=None, seed=0, device=None):
        """``pools``: {obj_id: {rgbs (n,4) u8 [r,g,b,state], depth (n,), dirs (n,3), T_wc (n,4,4)}}, any lengths >= the rays of
        a step (default ``cfg.n_per_optim``).  Initialisation is ``Trainer``'s (xavier-normal weights, nn.Linear's biases, the
        icosahedral B), drawn per object from a generator seeded with (seed, obj_id): an object's start does not depend on what
        else is trained beside it."""
        from . import trainer as trainer_mod
        self.cfg, self.obj_ids = cfg, list(obj_ids)
        self.R = int(rays_per_step or cfg.n_per_optim)
        _check(cfg, pools, self.obj_ids, self.R)
        self.device = dev = torch.device(device or cfg.training_device)
        self.n1, self.n2 = int(cfg.n_bins_cam2surface), int(cfg.n_bins)
        self.S = self.n1 + self.n2
        self.N = N = len(self.obj_ids)
        self.seed = int(seed)
        self.index = {obj_id: i for i, obj_id in enumerate(self.obj_ids)}
        # ---- the pools, concatenated; object o owns rows [pool_off[o], pool_off[o + 1])
        self.pool, self.rows, self.pool_off = pool_step.concat_pools([pools[i] for i in self.obj_ids], "T_wc", dev)
        self.ids = torch.tensor([int(i) & 0x7FFFFFFF for i in self.obj_ids], dtype=torch.int32, device=dev)
        # ---- parameters, moments, state: flat (N, ...) device buffers; the modules' tensors are views of theta
        lib = _C.load()
        assert int(lib.cnr_obj_param_count()) == PARAM_COUNT
        self.theta = torch.empty(N, PARAM_COUNT, device=dev)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.d_state = torch.zeros(N, 4, device=dev, dtype=torch.int64)
        self._losses = torch.zeros(3, N, device=dev)
        self.flags = torch.zeros(N, device=dev, dtype=torch.int32)
        self.ws = _C.workspace(lib.cnr_obj_workspace_bytes(N, self.R, self.S), dev, "cnr_obj_train")
        tcfg = copy.copy(cfg)
        tcfg.training_device = "cpu"
        self._modules = {}
        for o, obj_id in enumerate(self.obj_ids):
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(pool_step.instance_seed(self.seed, obj_id))
                t = trainer_mod.Trainer(tcfg, 0, [0])
            fc, pe = t.fc_occ_map, t.pe
            assert [k for k, _ in fc.named_parameters()] == PARAM_NAMES and [tuple(p.shape) for p in pe.parameters()] == [(21, 3)]
            fc.to(dev), pe.to(dev)
            off = 0
            for p in list(fc.parameters()) + list(pe.parameters()):
                k = p.numel()
                self.theta[o, off:off + k].copy_(p.data.reshape(-1))
                p.data = self.theta[o, off:off + k].view_as(p)
                off += k
            assert off == PARAM_COUNT
            self._modules[obj_id] = (pe, fc)
        self._init_steps()

    # ---- one launch = one step of every object ---------------------------------------------------------------------------------
    def launch(self, rows=None, u=None, g=None, grad=None, sigma=None, rgb=None, z=None, rows_out=None):
        """cnr_obj_train on this trainer's buffers.  ``rows`` (N,R) i32 segment-relative, ``u`` (N,R,S), ``g`` (N,R,n2): the step's
        rows and draws given (all three or none); the other arguments are optional outputs (include/cnr_hip.h)."""
        cfg, p = self.cfg, self.pool
        _C.call("cnr_obj_train", p["rgbs"], p["depth"], p["dirs"], p["T"], self.pool_off, min(self.rows), self.ids, self.N, self.R,
                self.n1, self.n2, float(cfg.surface_eps), float(cfg.stop_eps), float(cfg.min_depth), float(cfg.obj_scale),
                self.seed, rows, u, g, self.d_state, self.theta, self.exp_avg, self.exp_avg_sq, float(cfg.learning_rate), 0.9,
                0.999, 1e-8, float(cfg.weight_decay), 5.0, 10.0, self._losses, self.flags, grad, sigma, rgb, z, rows_out, self.ws,
                self.ws.numel())

    @property
    def losses(self):
        """(3, N): the depth / colour / opacity terms of every object's last step (src/loss.py:18-74), on the device"""
        return self._losses

    def modules(self, obj_id):
        """(UniDirsEmbed, OccupancyMap) of one object; their parameters are views of the live flat buffer (no copy-back)"""
        return self._modules[obj_id]

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------
    def save_checkpoints(self, weight_root, bboxes=None):
        """``<weight_root>/ckpt/<obj_id>/obj_<obj_id>_it_<steps>.pth`` per object with the keys FC_state_dict, PE_state_dict,
        obj_scale, bbox -- the file ``category_registration.load_pretrained_fields`` reads.  ``bboxes``: {obj_id: the oriented
        box of the object's cloud} (the reference only passes it through)."""
        files = []
        for obj_id in self.obj_ids:
            pe, fc = self._modules[obj_id]
            path = checkpoint_path(weight_root, obj_id, self.steps_done)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            torch.save(checkpoint_dict(pe, fc, self.cfg.obj_scale, None if bboxes is None else bboxes.get(obj_id)), path)
            files.append(path)
        return files

    # ---- from a loaded dataset ---------------------------------------------------------------------------------------------------
    crops_of = staticmethod(pool_step.crops_of)

    @staticmethod
    def pool_rows(inst_dict):
        """{obj_id: rows of its pool} = the summed areas of its crops (host arithmetic: what ``rays_per_step`` must not exceed)"""
        return {obj_id: sum((w1 - w0) * (h1 - h0) for _, w0, w1, h0, h1 in crops)
                for obj_id, crops in ObjectFieldTrainer.crops_of(inst_dict)}

    @classmethod
    def pools_from_dataset(cls, dataset, cfg, device=None):
        """{obj_id: pool} by the gather ``sceneCategory`` uses for a single-instance class (src/scene_cateogries.py:164-260): world
        frame (every row carries its frame's T_wc), the crops of ``frame_info``, this / other / unknown pixel states -- ONE
        cnr_gather_pool launch for all objects.  No global shuffle: the kernel's per-epoch bijection orders the rows."""
        per_obj = [(obj_id, [c + (idx,) for idx, c in enumerate(cr)]) for obj_id, cr in cls.crops_of(dataset.inst_dict)]
        return pool_step.gather_pools(dataset, cfg, per_obj, lambda obj_id, T_wc: T_wc, "T_wc",
                                      torch.device(device or dataset._parse_device()))

    @classmethod
    def from_dataset(cls, dataset, cfg, rays_per_step=None, seed=0, device=None):
        pools = cls.pools_from_dataset(dataset, cfg, device)
        return cls(cfg, pools, list(pools.keys()), rays_per_step=rays_per_step, seed=seed, device=device)
