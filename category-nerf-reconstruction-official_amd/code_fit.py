"""Fitting the codes of NEW instances to a trained, frozen category: the stage the reference shipped only as bytecode
(``reconstruct``, ``editing``: load a model, mesh with averaged or interpolated codes).  A category-level field is a prior: one
CodeNeRF per category, one shape code and one texture code per instance.  ``CodeFitter`` takes trained categories, freezes them and
solves for the two codes of instances they have not seen, each from several starting codes at once.

A CANDIDATE is one (instance, starting code) pair.  ONE launch of cnr_code_fit (csrc/code_fit.hip) is one optimisation step of every
candidate -- one workgroup per candidate; rows, draws, cursor, epoch and optimiser step on the device -- so a captured graph of steps
replays unchanged and nothing in a step waits for the host.  Per candidate the step is the reference's object step with a
one-object class and the network held fixed (train.py:123-167): the candidates of one instance share its pool, see the same rays and
the same draws, and differ only in their codes."""
import math

import numpy as np
import torch

from . import _C, pool_step
from .fused import ParamLayout
from .pool_step import next_state          # (the state rule: one definition for both kernels' trainers)  # noqa: F401
from .ops import LATENT_LAYERS, TRUNK_LAYERS

LOSS_NAMES = ("depth", "color", "opacity", "shape_norm", "texture_norm")
COLOR_SCALING, OPACITY_SCALING = 5.0, 10.0
SCORE_SEED = 0x5C0DE          # score(): one fixed key for rows and draws, whatever the fit's own seed and state


def check_hyperparams(hp):
    """the one network cnr_code_fit is built for: width 32, two shape blocks, one texture block"""
    if int(hp.get("W", 32)) != 32:
        raise NotImplementedError(f"CodeFitter: cnr_code_fit is built for W 32, not {hp.get('W')}")
    blocks = (int(hp.get("shape_blocks", 2)), int(hp.get("texture_blocks", 1)))
    if blocks != (2, 1):
        raise NotImplementedError(f"CodeFitter: cnr_code_fit is built for (shape, texture) blocks (2, 1), not {blocks}")
    return int(hp["latent_dim"])


def pack_net(trainer, lay, out):
    """the frozen parameters of one category's modules into ``out``: a row of fused.ParamLayout with no code rows"""
    fc, off = trainer.fc_occ_map, 0
    with torch.no_grad():
        for n, o, i in TRUNK_LAYERS:
            lin = fc._linear(n)
            out[off:off + o * i].copy_(lin.weight.reshape(-1)); off += o * i
            out[off:off + o].copy_(lin.bias.reshape(-1)); off += o
        assert off == lay.trunk[1]
        v = lay.views(out[None])
        for k, n in enumerate(LATENT_LAYERS):
            v["latW"][0, k].copy_(fc._linear(n).weight)
            v["latb"][0, k].copy_(fc._linear(n).bias)
        v["B"][0].copy_(trainer.pe.B_layer.weight)


def random_codes(m, L, seed, inst_id):
    """``m`` (2, L) starts from ``Trainer.load_codes``' distribution, randn / sqrt(L / 2), seeded by (seed, inst_id)"""
    gen = torch.Generator().manual_seed(pool_step.instance_seed(seed, inst_id))
    return torch.randn(m, 2, L, generator=gen) / math.sqrt(L / 2)


def build_starts(spec, shape_table, texture_table, seed, inst_id):
    """The starting codes of one instance, (M, 2, L) on the CPU.  ``spec``: "mean" (the mean of the category's trained codes),
    "objects" (one start per trained object), ("random", m), an explicit (M, 2, L) tensor, or a list combining these."""
    L = shape_table.shape[1]
    table = torch.stack([shape_table, texture_table], 1).detach().float().cpu()          # (n_obj, 2, L)
    if isinstance(spec, str) or torch.is_tensor(spec) or (isinstance(spec, tuple) and len(spec) == 2 and spec[0] == "random"):
        spec = [spec]
    out, n_random = [], 0
    for s in spec:
        if isinstance(s, str) and s == "mean":
            out.append(table.mean(0, keepdim=True))
        elif isinstance(s, str) and s == "objects":
            out.append(table.clone())
        elif isinstance(s, tuple) and len(s) == 2 and s[0] == "random":
            # (a second ("random", m) of one list continues the stream of the first)
            draws = random_codes(n_random + int(s[1]), L, seed, inst_id)
            out.append(draws[n_random:])
            n_random += int(s[1])
        elif torch.is_tensor(s):
            if s.dim() != 3 or tuple(s.shape[1:]) != (2, L):
                raise ValueError(f"CodeFitter: explicit starts are (M, 2, {L}), got {tuple(s.shape)}")
            out.append(s.detach().float().cpu())
        else:
            raise ValueError(f"CodeFitter: unknown start {s!r}")
    out = torch.cat(out) if out else torch.zeros(0, 2, L)
    if out.shape[0] == 0:
        raise ValueError(f"CodeFitter: instance {inst_id} has no start")
    return out.contiguous()


def attach_codes(trainer, inst_id, shape_code, texture_code, extent=None):
    """Make ``Trainer.meshing(inst_id)`` and ``Trainer.eval_points(..., inst_id=)`` work for a new instance without retraining:
    the codes become new rows of the trainer's tables.

    ``extent`` (3,): the instance's box extent.  ``Trainer.meshing`` of a category of several instances reads
    ``extent_dict[inst_id]``, so without it the new instance can be evaluated (``eval_points``) but not meshed.  A category
    trained with a SINGLE instance is refused: it lives in the world frame and meshes from ``bound_dict``; a second row would
    switch its own instance to the ``extent_dict`` branch, which it has no entry for.

    The two ``nn.Embedding`` tables are REPLACED by longer ones: whatever holds the old parameters -- an optimiser, a
    ``FusedCategoryTrainer`` built from them -- keeps the old tables and does not see the new row."""
    if inst_id in trainer.inst_id_to_index:
        raise ValueError(f"attach: instance {inst_id} is already in this category")
    if trainer.n_obj == 1:
        raise NotImplementedError("attach: a category trained with a single instance is world-frame and meshes from bound_dict; "
                                  "a second code row would break the meshing of the instance it has")
    for name, code in (("shape_codes", shape_code), ("texture_codes", texture_code)):
        emb = getattr(trainer, name)
        w = emb.weight.data
        new = torch.nn.Embedding(w.shape[0] + 1, w.shape[1])
        new.weight = torch.nn.Parameter(torch.cat([w, code.detach().to(w.device, w.dtype).reshape(1, -1)]))
        setattr(trainer, name, new.to(w.device))
    trainer.inst_id_to_index[inst_id] = trainer.n_obj
    trainer.n_obj += 1
    if extent is not None:
        if trainer.extent_dict is None:
            trainer.extent_dict = {}
        trainer.extent_dict[inst_id] = np.asarray(extent, dtype=np.float64)


def load_category(cfg, ckpt_file, allow_pickle=False):
    """A ``Trainer`` holding the category of a checkpoint in the reference's schema (``sceneCategory.save_checkpoints``:
    ``cls_<id>_iteration_<it>.pth``): network, embedding, the trained codes, ``inst_id_to_index`` and ``extent_dict``.  Read
    with ``weights_only=True`` unless ``allow_pickle`` (only for files you trust)."""
    from . import trainer as trainer_mod
    from .scene_cateogries import sceneCategory
    if allow_pickle:
        ck = torch.load(ckpt_file, map_location="cpu", weights_only=False)
    else:
        try:
            import numpy._core.multiarray as _ma
        except ImportError:                                       # numpy < 2
            import numpy.core.multiarray as _ma
        with torch.serialization.safe_globals([_ma._reconstruct, np.ndarray, np.dtype, type(np.dtype(np.float64)),
                                               type(np.dtype(np.float32)), type(np.dtype(np.int64))]):
            ck = torch.load(ckpt_file, map_location="cpu", weights_only=True)
    missing = [k for k in sceneCategory.CKPT_KEYS_OBJ if k not in ck]
    if missing or ck["cls_id"] == 0:
        raise KeyError(f"{ckpt_file}: not an object category's checkpoint (missing {missing}, cls_id {ck.get('cls_id')})")
    index = ck["instance_id_to_index"]
    t = trainer_mod.Trainer(cfg, ck["cls_id"], sorted(index, key=index.get))
    dev = cfg.training_device
    t.fc_occ_map.load_state_dict(ck["FC_state_dict"])
    t.pe.load_state_dict(ck["PE_state_dict"])
    t.shape_codes.load_state_dict(ck["shape_code_state_dict"])
    t.texture_codes.load_state_dict(ck["texture_code_state_dict"])
    for m in (t.fc_occ_map, t.pe, t.shape_codes, t.texture_codes):
        m.to(dev)
    t.inst_id_to_index, t.obj_scale, t.extent_dict = dict(index), ck["obj_scale"], ck["bound"]
    return t


class CodeFitter(pool_step.StepBranch):
    def __init__(self, cfg, nets, instances, starts="mean", rays_per_step=None, seed=0, reg_scaling=0.0005, device=None):
        """``nets``: {cls_id: Trainer} of CodeNeRF categories; their parameters are snapshotted into one flat buffer here
        (``refresh()`` snapshots again) and the modules are never written.  ``instances``: a list of dict(inst_id, cls_id,
        pool={rgbs (n,4) u8 [r,g,b,state], depth (n,), dirs (n,3), T (n,4,4)}, world_frame=False): ``T`` rows are T_CO, or T_WC
        with ``world_frame``.  ``starts``: see ``build_starts``; every instance gets the same recipe."""
        self.cfg = cfg
        self.L = L = check_hyperparams(cfg.net_hyperparams)
        self.R = R = int(rays_per_step or cfg.n_per_optim)
        self.n1, self.n2 = int(cfg.n_bins_cam2surface), int(cfg.n_bins)
        self.S = self.n1 + self.n2
        if self.S > 64:
            raise NotImplementedError("CodeFitter: at most 64 samples per ray")
        if not instances:
            raise ValueError("CodeFitter: no instance")
        for cls_id in nets:
            if cls_id == 0:
                raise ValueError("CodeFitter: class 0 is the background, which has no codes")
        if not 0 <= int(seed) < 2 ** 63:
            raise ValueError(f"CodeFitter: seed {seed} is outside [0, 2^63): it keys the kernel's rows and draws as an unsigned word")
        for inst in instances:
            # (the id keys the instance's rows and draws as an i32: two ids that differ above bit 30 would share them)
            if not 0 <= int(inst["inst_id"]) < 2 ** 31:
                raise ValueError(f"CodeFitter: instance id {inst['inst_id']} is outside [0, 2^31)")
            if inst["cls_id"] == 0:
                raise ValueError("CodeFitter: class 0 is the background, which has no codes")
            if inst["cls_id"] not in nets:
                raise ValueError(f"CodeFitter: instance {inst['inst_id']} is of class {inst['cls_id']}, which has no network here")
            rows = int(inst["pool"]["depth"].shape[0])
            if rows < R:
                raise ValueError(f"CodeFitter: instance {inst['inst_id']} has a pool of {rows} rows, fewer than the {R} rays of a step")
        for cls_id, t in nets.items():
            if int(t.shape_codes.weight.shape[1]) != L:
                raise ValueError(f"CodeFitter: class {cls_id} has codes of length {t.shape_codes.weight.shape[1]}, the config {L}")
        self.device = dev = torch.device(device or cfg.training_device)
        self.seed, self.reg_scaling = int(seed), float(reg_scaling)
        self.nets, self.cls_ids = dict(nets), list(nets.keys())
        self.lay = ParamLayout(L, 0)
        self.theta = torch.zeros(len(self.cls_ids), self.lay.total, device=dev)
        self.refresh()
        # ---- the pools, concatenated; instance p owns rows [pool_off[p], pool_off[p + 1])
        self.instances = list(instances)
        self.inst_ids = [inst["inst_id"] for inst in instances]
        if len(set(self.inst_ids)) != len(self.inst_ids):
            raise ValueError("CodeFitter: an instance id occurs twice")
        self.pool, self.rows, self.pool_off = pool_step.concat_pools([inst["pool"] for inst in instances], "T", dev)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.pool_ids = i32([int(i) for i in self.inst_ids])
        self.pool_world_frame = i32([1 if inst.get("world_frame", False) else 0 for inst in instances])
        # ---- the candidates: every start of every instance
        codes, cand_net, cand_pool, self.slices = [], [], [], {}
        for p, inst in enumerate(instances):
            t = nets[inst["cls_id"]]
            st = build_starts(starts, t.shape_codes.weight.data, t.texture_codes.weight.data, self.seed, inst["inst_id"])
            self.slices[inst["inst_id"]] = (len(cand_net), len(cand_net) + st.shape[0])
            codes.append(st)
            cand_net += [self.cls_ids.index(inst["cls_id"])] * st.shape[0]
            cand_pool += [p] * st.shape[0]
        self.K = K = len(cand_net)
        self.cand_net, self.cand_pool = i32(cand_net), i32(cand_pool)
        self._codes = torch.cat(codes).to(dev).contiguous()
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self._codes), torch.zeros_like(self._codes)
        self.d_state = torch.zeros(K, 4, device=dev, dtype=torch.int64)
        self._losses = torch.zeros(5, K, device=dev)
        self.flags = torch.zeros(K, device=dev, dtype=torch.int32)
        self._score_state = torch.zeros(K, 4, device=dev, dtype=torch.int64)
        self._score_losses = torch.zeros(5, K, device=dev)
        self._score_flags = torch.zeros(K, device=dev, dtype=torch.int32)
        self.ws = _C.workspace(_C.load().cnr_code_fit_workspace_bytes(K, R, self.S), dev, "cnr_code_fit")
        self._init_steps()

    def refresh(self):
        """snapshot the categories' parameters again (after more joint training); captured graphs read the same buffer"""
        for n, cls_id in enumerate(self.cls_ids):
            pack_net(self.nets[cls_id], self.lay, self.theta[n])

    # ---- one launch = one step of every candidate ------------------------------------------------------------------------------
    def launch(self, update=1, seed=None, d_state=None, losses=None, flags=None, rows=None, u=None, g=None, grad=None, sigma=None,
               rgb=None, z=None, rows_out=None):
        """cnr_code_fit on this fitter's buffers (include/cnr_hip.h).  ``rows`` (K,R) i32 segment-relative, ``u`` (K,R,S), ``g``
        (K,R,n2): the step's rows and draws given (all three or none); the remaining arguments are optional outputs."""
        cfg, p, lay = self.cfg, self.pool, self.lay
        _C.call("cnr_code_fit", self.theta, lay.total, lay.trunk[0], lay.latW[0], lay.latb[0], lay.B[0], len(self.cls_ids), self.L,
                p["rgbs"], p["depth"], p["dirs"], p["T"], self.pool_off, min(self.rows), self.pool_ids, self.pool_world_frame,
                len(self.rows), self.cand_net, self.cand_pool, self.K, self.R, self.n1, self.n2, float(cfg.surface_eps),
                float(cfg.stop_eps), float(cfg.min_depth), float(cfg.obj_scale), self.seed if seed is None else int(seed), rows, u, g,
                self.d_state if d_state is None else d_state, self._codes, self.exp_avg, self.exp_avg_sq, int(update),
                float(cfg.code_learning_rate), 0.9, 0.999, 1e-8, float(cfg.code_weight_decay), COLOR_SCALING, OPACITY_SCALING,
                self.reg_scaling, self._losses if losses is None else losses, self.flags if flags is None else flags, grad, sigma,
                rgb, z, rows_out, self.ws, self.ws.numel())

    @property
    def losses(self):
        """(5, K): depth / colour / opacity terms and the two code norms of every candidate's last step, on the device"""
        return self._losses

    def total(self, losses):
        """(K,) the loss a step descends: depth + 5 colour + 10 opacity + reg_scaling (||shape|| + ||texture||)"""
        return losses[0] + COLOR_SCALING * losses[1] + OPACITY_SCALING * losses[2] + self.reg_scaling * (losses[3] + losses[4])

    def score(self):
        """(K,) total loss of every candidate by ONE evaluation-only launch with a fixed key: cursor 0 of epoch 0 under
        SCORE_SEED, so every start of an instance is scored on the same rows and the same draws, now and after any number of
        steps.  Codes, moments and state are untouched."""
        self.launch(update=0, seed=SCORE_SEED, d_state=self._score_state, losses=self._score_losses, flags=self._score_flags)
        return self.total(self._score_losses).clone()

    def best(self, inst_id):
        """(start index, shape code, texture code) of the instance's start with the lowest ``score()``"""
        a, b = self.slices[inst_id]
        k = int(torch.argmin(self.score()[a:b]))
        return k, self._codes[a + k, 0].clone(), self._codes[a + k, 1].clone()

    def codes(self, inst_id, start=None):
        """(M, 2, L) codes of every start of the instance, or (2, L) of one; views of the live buffer"""
        a, b = self.slices[inst_id]
        return self._codes[a:b] if start is None else self._codes[a + int(start)]

    def attach(self, trainer, inst_id, extent=None):
        """The best codes of ``inst_id`` become new rows of ``trainer.shape_codes`` / ``trainer.texture_codes`` (``attach_codes``);
        ``extent`` (3,): the instance's box extent, which ``Trainer.meshing`` reads for a category of several instances."""
        k, shape_code, texture_code = self.best(inst_id)
        attach_codes(trainer, inst_id, shape_code, texture_code, extent)
        return k

    # ---- from a loaded dataset ---------------------------------------------------------------------------------------------------
    @staticmethod
    def pools_from_dataset(dataset, cfg, poses, frames=None, device=None):
        """{inst_id: pool} of the instances named in ``poses`` = {inst_id: T_obj (4,4)} -- the pose registration found -- by the
        gather ``sceneCategory`` uses for a class of several instances (src/scene_cateogries.py:164-260): the crops of the instance's
        ``frame_info``, this / other / unknown pixel states, every row carrying T_CO = inv(T_wc) @ T_obj of its frame -- ONE
        cnr_gather_pool launch for all of them.  ``frames``: only crops of these frames (the partially observed case)."""
        dev = torch.device(device or dataset._parse_device())
        keep = None if frames is None else set(frames)
        per_inst = [(inst_id, [c + (idx,) for idx, c in enumerate(cr) if keep is None or c[0] in keep])
                    for inst_id, cr in pool_step.crops_of(dataset.inst_dict) if inst_id in poses]
        missing = set(poses) - {i for i, _ in per_inst}
        if missing:
            raise ValueError(f"pools_from_dataset: no instance {sorted(missing)} in the dataset's inst_dict")
        if not any(crops for _, crops in per_inst):
            raise ValueError("pools_from_dataset: no crop left in the given frames")
        T_obj = {i: torch.as_tensor(np.asarray(poses[i]), dtype=torch.float32).to(dev) for i, _ in per_inst}
        return pool_step.gather_pools(dataset, cfg, per_inst, lambda inst_id, T_wc: torch.linalg.inv(T_wc) @ T_obj[inst_id], "T", dev)
