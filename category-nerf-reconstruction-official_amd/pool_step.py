"""What the two trainers built on a workgroup-owned step kernel share -- ``ObjectFieldTrainer`` (object_fields.py, cnr_obj_train)
and ``CodeFitter`` (code_fit.py, cnr_code_fit): ONE launch is one step of every owner (an object, a candidate), with rows, draws,
cursor, epoch and optimiser step on the device (csrc/pool_step_common.h).  Here: the host mirror of the state rule, the
per-instance seed, the concatenated pools, the branch interface of ``stepgraph.StepGraphs`` and the gather of pools from a loaded
dataset."""
import numpy as np
import torch

from . import _C, stepgraph


def next_state(state, rows, R):
    """The host mirror of the kernels' state rule: state = [cursor, rng step, optimiser step, epoch] of one owner after one
    more step of R rays on a pool of ``rows`` rows (src/scene_cateogries.py:439-449: the epoch ends when fewer than R rows are
    left behind the next slice)."""
    cursor, rng, opt, epoch = state
    cursor += R
    if cursor >= rows - R:
        cursor, epoch = 0, epoch + 1
    return [cursor, rng + 1, opt + 1, epoch]


def instance_seed(seed, inst_id):
    """the seed of what is drawn per instance on the host (an object's initialisation, a candidate's random starts): it depends
    on (seed, inst_id) alone, not on what else is trained beside the instance"""
    return (int(seed) * 7919 + 104729 * (int(inst_id) + 1)) & 0x7FFFFFFFFFFF


def concat_pools(pools, T_key, dev):
    """(pool, rows, pool_off): the pools {rgbs (n,4) u8, depth (n,), dirs (n,3), <T_key> (n,4,4)} concatenated on ``dev``, their
    lengths, and the (len + 1,) i64 offsets: pool p owns rows [pool_off[p], pool_off[p + 1])"""
    cat = lambda key, dt: torch.cat([p[key].to(dev, dt) for p in pools]).contiguous()
    pool = dict(rgbs=cat("rgbs", torch.uint8), depth=cat("depth", torch.float32), dirs=cat("dirs", torch.float32),
                T=cat(T_key, torch.float32))
    rows = [int(p["depth"].shape[0]) for p in pools]
    return pool, rows, torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int64, device=dev)


class StepBranch:
    """The branch interface of ``stepgraph.StepGraphs`` for a trainer whose step is one ``self.launch()`` that depends on nothing
    the host changes; ``self.d_state`` is the (owners, 4) device state."""
    parity = 0                # one state copy

    def _init_steps(self):
        self.steps_done = 0
        self._sched = stepgraph.StepGraphs([self], 3, 8)

    def record(self, slot=None, par=0):
        self.launch()

    def before_step(self):
        return 1 << 30        # every owner ends its epochs on the device: no step ever waits for the host

    def advance(self, U=1):
        self.steps_done += U

    def step(self, use_graph=True):
        """One step of every owner; after three eager steps it is captured and replayed."""
        self._sched.step(use_graph)

    def run(self, n, unroll=8, use_graph=True):
        """``n`` steps, the same arithmetic as ``n`` calls of ``step()``, in graphs of up to ``unroll`` steps."""
        self._sched.run(n, unroll, use_graph)

    def state(self):
        """(owners, 4) host list of [cursor, rng step, optimiser step, epoch]; synchronises"""
        return self.d_state.cpu().tolist()


def crops_of(inst_dict):
    """[(obj_id, [(frame, w0, w1, h0, h1), ...])] of every instance of every object class of a dataset's ``inst_dict``"""
    out = []
    for cls_id, entries in inst_dict.items():
        if cls_id == 0:
            continue
        for obj_id, info in entries.items():
            out.append((obj_id, [(fi["frame"],) + tuple(int(v) for v in fi["bbox"]) for fi in info["frame_info"]]))
    return out


def gather_pools(dataset, cfg, per_inst, pose_of_crop, T_name, dev):
    """{inst_id: {rgbs, depth, dirs, <T_name>}} by the gather ``sceneCategory`` uses (src/scene_cateogries.py:164-260): the crops of
    ``per_inst`` = [(inst_id, [(frame, w0, w1, h0, h1, index in frame_info), ...])], this / other / unknown pixel states, every
    row carrying ``pose_of_crop(inst_id, T_wc of its frame)`` -- ONE cnr_gather_pool launch for all instances; the pools are views
    of its outputs.  No global shuffle: the kernels' per-epoch bijection orders the rows."""
    from .scene_cateogries import cameraInfo
    sample_dict = dataset.sample_dict
    frames = sorted({c[0] for _, crops in per_inst for c in crops})
    slot = {f: i for i, f in enumerate(frames)}
    stack = lambda key, dt: torch.from_numpy(np.stack([np.asarray(sample_dict[f][key]) for f in frames])).to(dt)
    images = stack("image", torch.uint8).to(dev).contiguous()
    depths = stack("depth", torch.float32).to(dev).contiguous()
    masks = stack("obj_mask", torch.int32).to(dev).contiguous()
    T_wc = stack("T", torch.float32).to(dev)
    W, H = images.shape[1:3]
    rays = cameraInfo(cfg, device=dev).rays_dir_cache.contiguous()
    crops, areas, T_crop = [], [], []
    for inst_id, cr in per_inst:
        for frame, w0, w1, h0, h1, idx in cr:
            crops.append([slot[frame], int(inst_id), 0, w0, w1, h0, h1, idx])
            areas.append((w1 - w0) * (h1 - h0))
            T_crop.append(pose_of_crop(inst_id, T_wc[slot[frame]]))
    N = int(sum(areas))
    crops_t = torch.tensor(crops, dtype=torch.int32, device=dev)
    off_t = torch.tensor(np.concatenate([[0], np.cumsum(areas)]), dtype=torch.int64, device=dev)
    T_crop = torch.stack(T_crop).contiguous()
    rgbs = torch.empty(N, 4, dtype=torch.uint8, device=dev)
    depth, dirs, T_rows = torch.empty(N, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, 4, 4, device=dev)
    _C.call("cnr_gather_pool", images, depths, masks, rays, T_crop, crops_t, off_t, None, int(W), int(H), len(crops), N,
            rgbs, depth, dirs, T_rows, None, None)
    pools, at = {}, 0
    for inst_id, cr in per_inst:
        n = sum((w1 - w0) * (h1 - h0) for _, w0, w1, h0, h1, _ in cr)
        pools[inst_id] = {"rgbs": rgbs[at:at + n], "depth": depth[at:at + n], "dirs": dirs[at:at + n], T_name: T_rows[at:at + n]}
        at += n
    return pools
