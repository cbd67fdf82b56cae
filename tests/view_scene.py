"""TEST INFRASTRUCTURE for the scene view renderer: the box scenes of the segment tests, a small synthetic scene made of real
``Trainer`` objects behind the attributes ``SceneRenderer`` reads from a ``sceneCategory`` (obj_ids, trainer,
object_tensor_dict), and the fields of such a scene evaluated by oracle/ref_cpu.py on the CPU."""
import copy
from types import SimpleNamespace

import numpy as np
import torch

import view_cpu as V

ZMIN, ZMAX = 0.07, 8.0


def scene_a(with_bg=True):
    """-> T_wc (4,4), dirs (432,3) f32, to_box (E,3,4) f64: five boxes, up to three per pixel, camera inside the first"""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = V.rot((0.2, 1, 0.1), 0.35), (0.1, -0.2, -2.5)
    boxes = [((0, 0, 0), V.rot((0, 0, 1), 0.2), (3, 2.5, 3.2)),
             ((0.3, 0.1, 0), V.rot((1, 1, 0), 0.7), (0.5, 0.4, 0.6)),
             ((-0.2, 0, 0.6), V.rot((0, 1, 0), -0.4), (0.45, 0.7, 0.35)),
             ((0.1, -0.2, -4), np.eye(3), (0.5, 0.5, 0.5)),
             ((2.2, 1.4, 0.5), V.rot((1, 0, 0), 1.0), (0.3, 0.3, 0.3))]
    if not with_bg:
        boxes = boxes[1:]
    return T, V.pinhole_dirs(24, 18, 20, 11.5, 8.5), np.stack([V.box_affine(*b) for b in boxes])


def scene_b():
    """axis-parallel rays: identity pose, unrotated boxes, 41 rays with an exactly zero direction component"""
    boxes = [((0, 0, 3), np.eye(3), (0.52, 0.47, 0.5)), ((2, 0, 3), np.eye(3), (0.52, 0.47, 0.5)), ((0, 0, 0), np.eye(3), (1, 1, 1))]
    return np.eye(4), V.pinhole_dirs(24, 18, 20, 12, 9), np.stack([V.box_affine(*b) for b in boxes])


def scene_nested(n=9):
    """n nested boxes about the optical axis at depth 3 that cover the middle pixel columns only"""
    boxes = [((0, 0, 3), np.eye(3), (0.2 + 0.02 * k, 4.0, 0.3 + 0.1 * k)) for k in range(n)]
    return np.eye(4), V.pinhole_dirs(24, 18, 20, 11.5, 8.5), np.stack([V.box_affine(*b) for b in boxes])


def _sim3(scale, axis, angle, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = scale * V.rot(axis, angle), t
    return T


def small_camera(cfg, W=24, H=18, f=20.0):
    cfg.W, cfg.H, cfg.fx, cfg.fy, cfg.cx, cfg.cy = W, H, f, f, (W - 1) / 2.0, (H - 1) / 2.0
    cfg.min_depth, cfg.max_depth = ZMIN, ZMAX
    return cfg


def camera_pose():
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = V.rot((0.2, 1, 0.1), 0.35), (0.1, -0.2, -2.5)
    return T


def _trainer(cnr, cfg, cls_id, ids):
    """a Trainer whose random initial weights are drawn on the CPU (the same on every machine), then moved to cfg's device"""
    cpu_cfg = copy.copy(cfg)
    cpu_cfg.training_device = "cpu"
    t = cnr.trainer.Trainer(cpu_cfg, cls_id, ids)
    t.device = cfg.training_device
    t.fc_occ_map, t.pe = t.fc_occ_map.to(t.device), t.pe.to(t.device)
    if cls_id != 0:
        t.shape_codes, t.texture_codes = t.shape_codes.to(t.device), t.texture_codes.to(t.device)
    return t


def make_scene(cnr, cfg, seed=0, n_multi=1, n_obj=2, single=True, bg_hidden=32, with_bg=True, spread=0.25):
    """(cls_dict, scene_bg): `n_multi` categories of `n_obj` objects each (seeded sim3 poses, scales between 0.6 and 0.9, around
    the origin so their screen footprints overlap), one single-object world-frame category if `single`, and a background
    OccupancyMap(bg_hidden) if `with_bg`.  Random-init weights, seeded."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    cls_dict, next_id = {}, 1
    for k in range(n_multi):
        ids = list(range(next_id, next_id + n_obj))
        next_id += n_obj
        t = _trainer(cnr, cfg, 10 + k, ids)
        t.extent_dict, tensors = {}, {}
        for j, i in enumerate(ids):
            scale = 0.6 + 0.3 * j / max(n_obj - 1, 1)
            T_obj = _sim3(scale, rng.normal(size=3), rng.uniform(0, 3), rng.uniform(-spread, spread, 3) + (0.4 * k, 0, 0.3 * j))
            tensors[i] = cnr.utils.get_tensor_from_transform_sim3(T_obj)
            t.extent_dict[i] = np.array([1.0, 1.4, 0.8]) + 0.1 * j
        cls_dict[10 + k] = SimpleNamespace(cls_id=10 + k, obj_ids=ids, trainer=t, object_tensor_dict=tensors, world_frame=False)
    if single:
        i = next_id
        t = _trainer(cnr, cfg, 30, [i])
        t.bound_dict = {i: SimpleNamespace(extent=np.array([0.9, 0.7, 1.1]), center=np.array([-0.5, 0.2, 0.4]),
                                          R=V.rot((1, 0.5, 0), 0.6))}
        cls_dict[30] = SimpleNamespace(cls_id=30, obj_ids=[i], trainer=t, object_tensor_dict={}, world_frame=True)
    scene_bg = None
    if with_bg:
        bg_cfg = copy.copy(cfg)
        bg_cfg.hidden_feature_size, bg_cfg.obj_scale = bg_hidden, cfg.bg_scale
        t = _trainer(cnr, bg_cfg, 0, [0])
        t.bound = SimpleNamespace(extent=np.array([6.0, 5.0, 6.4]), center=np.zeros(3), R=V.rot((0, 0, 1), 0.2))
        scene_bg = SimpleNamespace(cls_id=0, obj_ids=[0], trainer=t, world_frame=True)
    return cls_dict, scene_bg


def oracle_fields(cls_dict, scene_bg, entities, seg_entity, pts64):
    """sigma (N,S), colour (N,S,3) in float64 of the entities' fields at pts64 (N,S,3), by oracle/ref_cpu.py on the CPU"""
    from oracle import ref_cpu as O
    N, S = pts64.shape[:2]
    sigma, color = np.zeros((N, S)), np.zeros((N, S, 3))
    cats = list(cls_dict.values())
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            for e, ent in enumerate(entities):
                m = np.nonzero(seg_entity == e)[0]
                if len(m) == 0:
                    continue
                x = torch.from_numpy(pts64[m])[None]                                          # (1,n,S,3)
                t = scene_bg.trainer if ent.cat < 0 else cats[ent.cat].trainer
                p = {k: v.detach().cpu().double() for k, v in t.fc_occ_map.state_dict().items()}
                B = t.pe.B_layer.weight.detach().cpu().double()[None]
                emb = O.unidirs_embed(x, B, float(t.pe._scale))
                if ent.cat < 0:
                    s, c = O.occupancy_map_forward(p, emb[0])
                else:
                    cs = t.shape_codes.weight[ent.row].detach().cpu().double().view(1, 1, 1, -1)
                    ct = t.texture_codes.weight[ent.row].detach().cpu().double().view(1, 1, 1, -1)
                    s, c = O.codenerf_forward({k: v[None] for k, v in p.items()}, emb, cs, ct)
                sigma[m], color[m] = s.reshape(len(m), S).numpy(), c.reshape(len(m), S, 3).numpy()
    finally:
        torch.set_default_dtype(old)
    return sigma, color


def restated_render(renderer, cls_dict, scene_bg, T_wc, S, dtype, transforms=None, hidden=(), thr=0.5):
    """The whole render by tests/view_cpu.py in `dtype`, field values from the oracle at the restatement's own points (always
    evaluated in float64, then cast: the fields are not what this restatement is about)."""
    import cnr_amd
    ents = cnr_amd.view.edited(renderer.entities, transforms, hidden)
    r32 = lambda a: np.asarray(a, np.float32)                       # what the kernels are handed
    to_box, to_field = r32(np.stack([e.to_box for e in ents])), r32(np.stack([e.to_field for e in ents]))
    dirs = V.pinhole_dirs(renderer.W, renderer.H, renderer.cfg.fx, renderer.cfg.cx, renderer.cfg.cy)
    assert renderer.cfg.fx == renderer.cfg.fy
    seg = V.segments(r32(T_wc), dirs, to_box, renderer.zmin, renderer.zmax, dtype)
    z, pts = V.points(r32(T_wc), dirs, to_field, seg["seg_pixel"], seg["seg_entity"], seg["seg_z"], S, dtype)
    sigma, color = oracle_fields(cls_dict, scene_bg, ents, seg["seg_entity"], np.asarray(pts, np.float64))
    inst = np.array([e.inst_id for e in ents], np.int32)
    out = V.composite(sigma, color, z, seg["pix_segs"], seg["seg_entity"], inst, thr, dtype)
    out.update(seg=seg, z=z, pts=pts, sigma=sigma, color=color)
    return out
