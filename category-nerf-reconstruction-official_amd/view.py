"""Scene view rendering: a camera pose in, an image of the composed scene out -- colour, depth, opacity,
depth variance and an instance label per pixel -- with two edits that leave the trained state alone: move an entity by a
world-to-world similarity, or hide it.

An *entity* is one field with the box ``Trainer.meshing`` evaluates for it: the background, or one object of a category.
Rays are cut against every box (``cnr_view_segments_*``), each segment gets uniform midpoint samples in its field's frame
(``cnr_view_points``), the fields are evaluated by the kernels meshing uses (``cnr_field_fwd`` on the precise geometry
branch, one launch per category; the background through ``eval_points``' three paths), and ``cnr_view_composite`` merges the
samples of all segments of a pixel by camera depth into one alpha composite -- for one segment exactly the per-ray formulas
of the training renderer (src/render_rays.py:25-50, src/loss.py:41-48).  There is no reference renderer to compare a whole
image against: the composite is pinned to those per-ray formulas and the volumes to ``Trainer.meshing``'s.

Empty-space skipping is opt-in: per-entity occupancy grids over the boxes (``build_grids`` / ``set_grids``; ``cnr_view_grid_*``)
and ``render(..., skip_empty=True)``, which lists the samples in set cells (``cnr_view_active_count`` / ``_emit`` in place of
``cnr_view_points``), evaluates the fields on that list alone and scatters the values back (``cnr_view_scatter_active``)."""
import os

import numpy as np
import torch

from . import _C, ops
from .utils import get_transform_from_tensor_sim3

KMAX, SMAX = 8, 128


class Entity:
    """inst_id, to_box / to_field (3,4) float64, and where its field lives: ``cat`` = -1 for the background, else the index of
    its category in cls_dict order, ``row`` = the object's row in the category's code tables, ``index`` = its place in the
    scene's un-edited entity list, which an edit keeps."""

    def __init__(self, inst_id, to_box, to_field, cat, row, index=-1):
        self.inst_id, self.to_box, self.to_field, self.cat, self.row = int(inst_id), to_box, to_field, cat, row
        self.index = int(index)          # its place in the un-edited list of scene_entities: the slot of its occupancy grid


def _box_affine(center, R, half):
    """diag(1/h) R^T [I | -c] (float64)"""
    A = np.diag(1.0 / np.asarray(half, np.float64)) @ np.asarray(R, np.float64).T
    return np.concatenate([A, -(A @ np.asarray(center, np.float64).reshape(3))[:, None]], 1)


def _sim3_matrix(vec):
    return get_transform_from_tensor_sim3(torch.as_tensor(vec).detach().cpu().double()).numpy()


def scene_entities(cls_dict, scene_bg):
    """The entity list of a scene: the background first, if present, then the categories in ``cls_dict`` order with their
    objects in ``obj_ids`` order.  The volumes are the ones ``Trainer.meshing`` evaluates (trainer.py)."""
    ident = np.eye(4)[:3]
    out = []
    if scene_bg is not None:
        t = scene_bg.trainer
        b = t.bound
        out.append(Entity(0, _box_affine(b.center, b.R, np.asarray(b.extent, np.float64) / (2.0 * t.bound_extent)), ident.copy(), -1, 0))
    for k, sc in enumerate(cls_dict.values()):
        t = sc.trainer
        for inst_id in sc.obj_ids:
            if t.n_obj == 1:               # world frame
                b = t.bound_dict[inst_id]
                h = np.asarray(b.extent, np.float64) / (2.0 * t.bound_extent)
                out.append(Entity(inst_id, _box_affine(b.center, b.R, h), ident.copy(), k, 0))
            else:
                extent = np.asarray(t.extent_dict[inst_id], np.float64)
                h = (extent / np.max(extent / 2)) / (2.0 * t.bound_extent)
                to_field = np.linalg.inv(_sim3_matrix(sc.object_tensor_dict[inst_id]))[:3]
                out.append(Entity(inst_id, np.diag(1.0 / h) @ to_field, to_field, k, t.inst_id_to_index[inst_id]))
    for i, e in enumerate(out):
        e.index = i
    return out


def edited(entities, transforms=None, hidden=()):
    """The entities a render launches for: ``hidden`` dropped, ``transforms`` {inst_id: E (4,4) world -> world} applied as
    to_box <- to_box E^-1, to_field <- to_field E^-1.  Every entity keeps its ``index``."""
    transforms, hidden = dict(transforms or {}), set(hidden)
    ids = [e.inst_id for e in entities]
    for i in list(transforms) + list(hidden):
        if ids.count(i) != 1:        # (a dataset may give an object the background's id 0: such an id cannot address an edit)
            raise ValueError("inst_id {} names {} entities".format(i, ids.count(i)))
    out = []
    for e in entities:
        if e.inst_id in hidden:
            continue
        if e.inst_id in transforms:
            Einv = np.linalg.inv(np.asarray(transforms[e.inst_id], np.float64).reshape(4, 4))
            e = Entity(e.inst_id, e.to_box @ Einv, e.to_field @ Einv, e.cat, e.row, e.index)
        out.append(e)
    return out


def _bg_logits(t, pts, chunk_size=500000):
    """sigma (x10 logit) and colour of the background field at pts (M,3): the three paths of Trainer.eval_points"""
    sig, col = [], []
    fused = t.eval_precision == "fused" and t.hidden_feature_size == 128
    if fused:
        flat = torch.cat([p.reshape(-1) for p in t.fc_occ_map.parameters()] + [t.pe.B_layer.weight.reshape(-1)]).contiguous()
        assert flat.numel() == int(_C.load().cnr_bg_param_count())
        packed = torch.empty(int(_C.load().cnr_bg_pack_bytes()), device=flat.device, dtype=torch.uint8)
        _C.call("cnr_bg_pack", flat, packed)
    for k in range(0, pts.shape[0], chunk_size):
        p = pts[k:k + chunk_size].contiguous()
        if fused:
            s, c = torch.empty(p.shape[0], device=p.device), torch.empty(p.shape[0], 3, device=p.device)
            _C.call("cnr_bg_forward", p, flat, packed, float(t.pe._scale), p.shape[0], s, c, None, None)
        else:
            s, c = t.fc_occ_map(t.pe(p[:, None, :]))
        sig.append(s.reshape(-1))
        col.append(c.reshape(-1, 3))
    return torch.cat(sig), torch.cat(col)


def _check_resolution(G):
    if isinstance(G, bool) or int(G) != G or not 4 <= G <= 128 or G % 4:
        raise ValueError("the grid resolution must be a multiple of 4 in 4 .. 128, not {}".format(G))
    return int(G)


def pack_grid_bits(bits):
    """(E,G,G,G) bool -> (E, G^3/32) int32: cell (ix,iy,iz) at l = (ix G + iy) G + iz is bit l & 31 of word l >> 5"""
    E = bits.shape[0]
    b = bits.reshape(E, -1, 32).to(torch.int64)
    w = (b << torch.arange(32, device=bits.device, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def unpack_grid_words(words, G):
    """the inverse of pack_grid_bits: (E, G^3/32) int32 -> (E,G,G,G) bool"""
    w = words.to(torch.int64)[..., None] >> torch.arange(32, device=words.device, dtype=torch.int64)
    return (w & 1).bool().reshape(words.shape[0], G, G, G)


class SceneRenderer:
    """``SceneRenderer(cls_dict, scene_bg, cfg)``: the arguments of ``FullStepTrainer.from_scene``.  Reads the modules'
    parameters at every ``render`` -- after fused training run ``sync_to_modules()`` first, as for meshing.

    Empty-space skipping (opt-in): ``build_grids`` or ``set_grids`` gives every entity of ``self.entities`` one bit per cell of
    a G^3 grid over its box, and ``render(..., skip_empty=True)`` evaluates the fields only at the samples whose cell is set;
    every other sample has occupancy zero.  The grids are a snapshot of the parameters ``build_grids`` read: rebuild them after
    further training.  They live in box coordinates, so ``transforms=`` and ``hidden=`` need no rebuild."""

    def __init__(self, cls_dict, scene_bg, cfg):
        self.cls_dict, self.scene_bg, self.cfg = cls_dict, scene_bg, cfg
        self.categories = list(cls_dict.values())
        self.entities = scene_entities(cls_dict, scene_bg)
        self.device = torch.device(cfg.training_device)
        self.W, self.H = int(cfg.W), int(cfg.H)
        self.zmin, self.zmax = float(cfg.min_depth), float(cfg.max_depth)
        self._dirs = None
        self.active_samples = (0, 0)   # of the last skip_empty render: (samples evaluated, samples of all segments)
        self._grids = None             # (G, words (len(entities), G^3/32) int32, [has a grid] per entity): build_grids / set_grids
        self.stage_events = None       # a list: render appends (stage name, device event) after every stage (tools/time_view.py)

    def _mark(self, name):
        if self.stage_events is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.stage_events.append((name, ev))

    def dirs(self):
        """the cameraInfo cache rows (W*H, 3), pixel w * H + h"""
        if self._dirs is None:
            from .scene_cateogries import cameraInfo
            self._dirs = cameraInfo(self.cfg, device=self.device).rays_dir_cache.reshape(-1, 3).contiguous()
        return self._dirs

    def _category_operands(self, cats):
        """{category index: (B, packed, packed_lo, bias rows (n_obj,4,32), scale, trunk)} of the categories in use"""
        out = {}
        for k in cats:
            t = self.categories[k].trainer
            rows = [t._codenerf_rows(i) for i in self.categories[k].obj_ids]
            trunk, B = rows[0][0], rows[0][1]
            brows = torch.cat([r[2] for r in rows], 0).contiguous()
            out[k] = (B, ops.pack_weights(trunk), ops.pack_weights_lo(trunk), brows, float(t.pe._scale), trunk)
        return out

    def _surface_normals(self, T, dirs, to_field, runs, row_of, operands, thr, depth, opacity, mass, pix_segs, seg_entity, normal):
        """The normal image of one chunk, after its composite: surface points bucketed by field run (cnr_view_surface_points),
        one gradient launch per run (cnr_field_grad / cnr_occmap_grad), then n = -A^T g / |A^T g| per pixel (cnr_view_normals).
        -> (surf_entity (P,), surf_pts (P,3))"""
        dev, P, R = self.device, dirs.shape[0], len(runs)
        ent_run = torch.empty(to_field.shape[0], dtype=torch.int32)
        for r, (_, a, b) in enumerate(runs):
            ent_run[a:b] = r
        ent_run = ent_run.to(dev)
        ws = _C.workspace(_C.load().cnr_view_surface_workspace_bytes(P, R), dev, "cnr_view_surface")
        run_off = torch.empty(R + 1, device=dev, dtype=torch.int64)
        surf_entity, surf_slot = torch.empty(P, device=dev, dtype=torch.int32), torch.empty(P, device=dev, dtype=torch.int32)
        surf_pts, list_pts = torch.empty(P, 3, device=dev), torch.empty(P, 3, device=dev)
        list_row = torch.empty(P, device=dev, dtype=torch.int32)
        _C.call("cnr_view_surface_points", T, dirs, to_field, depth, opacity, float(thr), mass, pix_segs, seg_entity, ent_run, row_of,
                P, R, ws, run_off, surf_entity, surf_slot, surf_pts, list_pts, list_row)
        self._mark("surface points")
        off = run_off.tolist()
        M = off[R]
        grad_c = torch.empty(max(M, 1), 3, device=dev)
        for r, (cat, _, _) in enumerate(runs):
            m0, m1 = off[r], off[r + 1]
            if m1 == m0:
                continue
            if cat < 0:
                t = self.scene_bg.trainer
                _, g = ops.occmap_grad(t.fc_occ_map, t.pe, list_pts[m0:m1])
            else:
                B, _, _, brows, scale, trunk = operands[cat]
                _, g = ops.field_grad(list_pts[m0:m1], B, trunk, brows, list_row[m0:m1], scale)
            grad_c[m0:m1] = g
            self._mark("gradient background" if cat < 0 else "gradient category {}".format(cat))
        _C.call("cnr_view_normals", grad_c, surf_slot, surf_entity, to_field, P, M, normal)
        self._mark("normals")
        return surf_entity, surf_pts

    # ---- occupancy grids -------------------------------------------------------------------------------------------------
    def lattice_occupancy(self, index, dim):
        """Occupancy (dim,dim,dim) of entity ``self.entities[index]`` on the lattice ``Trainer.meshing`` forms for it at
        grid_dim = dim, by the kernels meshing evaluates it with: the precise cnr_field_fwd launch of ``_grid_occupancy`` for a
        category object, ``eval_points``' background paths (``eval_precision``) for the background."""
        from . import render_rays
        ent = self.entities[index]
        t = self.scene_bg.trainer if ent.cat < 0 else self.categories[ent.cat].trainer
        with torch.no_grad(), torch.cuda.device(self.device):
            if ent.cat < 0 or t.n_obj == 1:                # trainer.py, meshing: the box of the bound
                bound = t.bound if ent.cat < 0 else t.bound_dict[ent.inst_id]
                scale = torch.from_numpy(np.asarray(bound.extent / (2.0 * t.bound_extent))).float().to(self.device)
                tr = np.eye(4, dtype=np.float32)
                tr[:3, 3], tr[:3, :3] = bound.center, bound.R
                grid = render_rays.make_3D_grid(occ_range=[-1., 1.], dim=dim, device=self.device, scale=scale,
                                                transform=torch.from_numpy(tr).to(self.device)).view(-1, 3)
            else:
                extent = t.extent_dict[ent.inst_id]
                extent = extent / np.max(extent / 2)
                scale = torch.from_numpy(np.asarray(extent / (2.0 * t.bound_extent))).float().to(self.device)
                grid = render_rays.make_3D_grid(occ_range=[-1., 1.], dim=dim, device=self.device, scale=scale).view(-1, 3)
            if ent.cat < 0:
                step = 1 << 22                             # the colours of a slice are dropped before the next one
                sig = torch.cat([_bg_logits(t, grid[k:k + step])[0] for k in range(0, grid.shape[0], step)])
            else:
                trunk, B, brows = t._codenerf_rows(ent.inst_id)
                row = torch.zeros(1, 1, device=self.device, dtype=torch.int32)
                sig, _ = ops.field_fwd(grid.contiguous().view(1, 1, -1, 3), B, ops.pack_weights(trunk), brows, row, t.pe._scale,
                                       packed_lo=ops.pack_weights_lo(trunk))
            return render_rays.occupancy_activation(sig.reshape(-1)).reshape(dim, dim, dim).contiguous()

    def build_grids(self, resolution=64, sub=2, threshold=1e-3, dilate=1):
        """One occupancy grid per entity from the modules' current parameters: occupancy on meshing's lattice of
        ``resolution * sub + 1`` points per axis (``lattice_occupancy``), a cell set iff a lattice value on it or on its faces
        is not below ``threshold`` (cnr_view_grid_cells), then grown by ``dilate`` cells (cnr_view_grid_dilate).  One entity
        at a time, so one lattice is alive.  With m skipped samples on a ray, and the field below ``threshold`` wherever the
        lattice is, the transmittance changes by at most 1 - (1 - threshold)^m; between lattice points nothing is known."""
        G = _check_resolution(resolution)
        if isinstance(sub, bool) or int(sub) != sub or not 1 <= sub <= 4:
            raise ValueError("sub must be in 1 .. 4")
        if isinstance(dilate, bool) or int(dilate) != dilate or not 0 <= dilate <= 2:
            raise ValueError("dilate must be in 0 .. 2")
        sub, dilate = int(sub), int(dilate)
        words = torch.empty(len(self.entities), G ** 3 // 32, device=self.device, dtype=torch.int32)
        tmp = torch.empty(G ** 3 // 32, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            for i in range(len(self.entities)):
                occ = self.lattice_occupancy(i, G * sub + 1)
                _C.call("cnr_view_grid_cells", occ, G, sub, float(threshold), tmp)
                _C.call("cnr_view_grid_dilate", tmp, G, dilate, words[i])
                del occ
        self._grids = (G, words, [True] * len(self.entities))

    def set_grids(self, bits):
        """Caller-supplied grids: ``bits`` (len(self.entities), G, G, G) bool, axis order (x, y, z) of the box; or a sequence
        of (G,G,G) bool arrays with None for an entity without a grid, which counts as all set.  None drops the grids."""
        if bits is None:
            self._grids = None
            return
        E = len(self.entities)
        if not torch.is_tensor(bits) and not isinstance(bits, np.ndarray):
            bits = list(bits)
            if len(bits) != E:
                raise ValueError("{} grids for {} entities".format(len(bits), E))
            has = [b is not None for b in bits]
            given = [torch.as_tensor(b) for b in bits if b is not None]
            if not given:
                raise ValueError("no grid at all")
            if any(g.shape != given[0].shape for g in given):
                raise ValueError("the grids must share one resolution")
            it = iter(given)
            bits = torch.stack([next(it) if h else torch.ones_like(given[0]) for h in has])
        else:
            bits, has = torch.as_tensor(bits), [True] * E
        if bits.dim() != 4 or bits.shape[0] != E or not bits.shape[1] == bits.shape[2] == bits.shape[3]:
            raise ValueError("grids must have the shape ({}, G, G, G), not {}".format(E, tuple(bits.shape)))
        if bits.dtype != torch.bool:
            raise ValueError("grids must be bool, not {}".format(bits.dtype))
        G = _check_resolution(bits.shape[1])
        self._grids = (G, pack_grid_bits(bits.to(self.device)), has)

    def grids(self):
        """(E,G,G,G) bool of the grids in use (all set where an entity has none), or None"""
        if self._grids is None:
            return None
        G, words, has = self._grids
        bits = unpack_grid_words(words, G)
        bits[[i for i, h in enumerate(has) if not h]] = True
        return bits

    def render(self, T_wc, n_samples=64, transforms=None, hidden=(), chunk=65536, opacity_threshold=0.5, return_samples=False,
               skip_empty=False, normals=False):
        """-> {rgb (W,H,3), depth, opacity, var (W,H) float32, instance (W,H) int32 (-1: nothing opaque enough)}; (W,H,...) as
        every image here.  Pixels go through in chunks of ``chunk``; the result does not depend on it.  A pixel met by more
        than 8 boxes raises ValueError.  ``return_samples``: also the intermediate arrays (single chunk only).
        ``skip_empty``: evaluate the fields only where the occupancy grids are set (ValueError without grids): the same
        render with the occupancy of every other sample set to zero.  ``self.active_samples`` then holds (samples evaluated,
        samples of all segments), and the returned samples' ``pts`` is the compact list (M,3) that ``active_idx`` indexes.
        ``normals``: the result gains ``normal`` (W,H,3): the world-frame unit vector out of the surface (towards decreasing
        occupancy) at the rendered depth, from the gradient of the field whose segment gave the pixel its label, taken through
        the *edited* entity's transform; exactly zero where ``instance`` is -1 or the gradient vanishes.  The samples then
        gain ``surface_pts`` (P,3), field frame, and ``surface_entity`` (P,), -1 for none."""
        S, dev = int(n_samples), self.device
        if not 1 <= S <= SMAX:
            raise ValueError("n_samples must be in 1 .. {}".format(SMAX))
        if skip_empty and self._grids is None:
            raise ValueError("skip_empty wants occupancy grids: call build_grids() or set_grids() first")
        ents = edited(self.entities, transforms, hidden)
        P_all = self.W * self.H
        out = dict(rgb=torch.zeros(P_all, 3, device=dev), depth=torch.zeros(P_all, device=dev),
                   opacity=torch.zeros(P_all, device=dev), var=torch.zeros(P_all, device=dev),
                   instance=torch.full((P_all,), -1, device=dev, dtype=torch.int32))
        if normals:
            out["normal"] = torch.zeros(P_all, 3, device=dev)
        shape = lambda r: {k: v.reshape(self.W, self.H, *v.shape[1:]) for k, v in r.items()}
        if not ents:
            return shape(out)
        if return_samples and chunk < P_all:
            raise ValueError("return_samples wants the whole image in one chunk")
        E = len(ents)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        T = f32(np.asarray(T_wc.detach().cpu() if torch.is_tensor(T_wc) else T_wc, np.float64).reshape(4, 4))
        to_box, to_field = f32(np.stack([e.to_box for e in ents])), f32(np.stack([e.to_field for e in ents]))
        inst = torch.tensor([e.inst_id for e in ents], dtype=torch.int32, device=dev)
        # entity runs that share a field evaluation: the background alone, a category's objects together
        runs, e0 = [], 0
        while e0 < E:
            e1 = e0
            while e1 < E and ents[e1].cat == ents[e0].cat:
                e1 += 1
            runs.append((ents[e0].cat, e0, e1))
            e0 = e1
        row_of = torch.tensor([e.row for e in ents], dtype=torch.int32, device=dev)
        if skip_empty:
            G, grid_words, has = self._grids
            ent_grid = torch.tensor([e.index if has[e.index] else -1 for e in ents], dtype=torch.int32, device=dev)
        dirs_all = self.dirs()
        if skip_empty:
            self.active_samples = (0, 0)
        with torch.no_grad(), torch.cuda.device(dev):
            operands = self._category_operands([c for c, _, _ in runs if c >= 0])
            for p0 in range(0, P_all, int(chunk)):
                self._mark("start")
                dirs = dirs_all[p0:p0 + int(chunk)]
                P = dirs.shape[0]
                ws = _C.workspace(_C.load().cnr_view_segments_workspace_bytes(P, E), dev, "cnr_view_segments")
                meta = torch.empty(2 * E + 3, device=dev, dtype=torch.int64)   # entity_offset | active_offset | active samples
                ent_off, act_off, n_active = meta[:E + 1], meta[E + 1:2 * E + 2], meta[2 * E + 2:]
                counts = torch.empty(2, device=dev, dtype=torch.int64)
                _C.call("cnr_view_segments_count", T, dirs, to_box, P, E, self.zmin, self.zmax, ws, ent_off, counts[0:1], counts[1:2])
                N, overflow = (int(v) for v in counts.tolist())
                if overflow > 0:
                    raise ValueError("{} pixels are met by more than {} entity boxes".format(overflow, KMAX))
                pix_segs = torch.empty(P, KMAX, device=dev, dtype=torch.int32)
                seg_pixel = torch.empty(max(N, 1), device=dev, dtype=torch.int32)
                seg_entity = torch.empty(max(N, 1), device=dev, dtype=torch.int32)
                seg_z = torch.empty(max(N, 1), 2, device=dev)
                _C.call("cnr_view_segments_emit", T, dirs, to_box, P, E, self.zmin, self.zmax, ws, seg_pixel, seg_entity, seg_z, pix_segs)
                self._mark("segments")
                if N == 0:
                    continue
                z = torch.empty(N, S, device=dev)
                sigma, color = torch.empty(N, S, device=dev), torch.empty(N, S, 3, device=dev)
                if skip_empty:
                    aws = _C.workspace(_C.load().cnr_view_active_workspace_bytes(N, S, E), dev, "cnr_view_active")
                    _C.call("cnr_view_active_count", T, dirs, to_box, seg_pixel, seg_entity, seg_z, ent_off, N, S, E, grid_words,
                            ent_grid, G, aws, act_off, n_active)
                    vals = meta.tolist()
                    aoff, M = vals[E + 1:2 * E + 2], vals[2 * E + 1]
                    active_idx = torch.empty(max(M, 1), device=dev, dtype=torch.int64)
                    pts = torch.empty(max(M, 1), 3, device=dev)
                    block_row = torch.empty(max(M // 64, 1), device=dev, dtype=torch.int32)
                    _C.call("cnr_view_active_emit", T, dirs, to_field, seg_pixel, seg_entity, seg_z, N, S, E, row_of, aws, act_off, M,
                            z, active_idx, pts, block_row)
                    self._mark("points")
                    sigma_c, color_c = torch.empty(max(M, 1), device=dev), torch.empty(max(M, 1), 3, device=dev)
                    for cat, a, b in runs:
                        m0, m1 = aoff[a], aoff[b]
                        if m1 == m0:
                            continue
                        if cat < 0:
                            sg, cl = _bg_logits(self.scene_bg.trainer, pts[m0:m1])
                        else:
                            B, packed, lo, brows, scale, _ = operands[cat]
                            sg, cl = ops.field_fwd(pts[m0:m1].reshape(1, (m1 - m0) // 64, 64, 3), B, packed, brows,
                                                   block_row[m0 // 64:m1 // 64].reshape(1, -1), scale, packed_lo=lo)
                        sigma_c[m0:m1], color_c[m0:m1] = sg.reshape(-1), cl.reshape(-1, 3)
                        self._mark("field background" if cat < 0 else "field category {}".format(cat))
                    _C.call("cnr_view_scatter_active", sigma_c, color_c, active_idx, M, N * S, sigma, color)
                    self._mark("scatter")
                    self.active_samples = (self.active_samples[0] + vals[2 * E + 2], self.active_samples[1] + N * S)
                else:
                    pts = torch.empty(N, S, 3, device=dev)
                    _C.call("cnr_view_points", T, dirs, to_field, seg_pixel, seg_entity, seg_z, N, S, z, pts)
                    self._mark("points")
                    off = ent_off.tolist()
                    for cat, a, b in runs:
                        s0, s1 = off[a], off[b]
                        if s1 == s0:
                            continue
                        if cat < 0:
                            sg, cl = _bg_logits(self.scene_bg.trainer, pts[s0:s1].reshape(-1, 3))
                        else:
                            B, packed, lo, brows, scale, _ = operands[cat]
                            ray_row = row_of[seg_entity[s0:s1].long()].reshape(1, -1).contiguous()
                            sg, cl = ops.field_fwd(pts[s0:s1].reshape(1, s1 - s0, S, 3), B, packed, brows, ray_row, scale, packed_lo=lo)
                        sigma[s0:s1], color[s0:s1] = sg.reshape(-1, S), cl.reshape(-1, S, 3)
                        self._mark("field background" if cat < 0 else "field category {}".format(cat))
                mass = torch.empty(P, KMAX, device=dev)
                sl = slice(p0, p0 + P)
                _C.call("cnr_view_composite", sigma, color, z, pix_segs, seg_entity, inst, P, S, float(opacity_threshold),
                        out["rgb"][sl], out["depth"][sl], out["opacity"][sl], out["var"][sl], mass, out["instance"][sl])
                self._mark("composite")
                if normals:
                    surf_entity, surf_pts = self._surface_normals(T, dirs, to_field, runs, row_of, operands, opacity_threshold,
                                                                  out["depth"][sl], out["opacity"][sl], mass, pix_segs, seg_entity,
                                                                  out["normal"][sl])
                if return_samples:
                    out["samples"] = dict(seg_pixel=seg_pixel[:N], seg_entity=seg_entity[:N], seg_z=seg_z[:N], entity_offset=ent_off,
                                          pix_segs=pix_segs, z=z, pts=pts, sigma=sigma, color=color, mass=mass,
                                          to_box=to_box, to_field=to_field, inst_ids=inst)
                    if skip_empty:
                        out["samples"].update(active_idx=active_idx[:M], active_offset=act_off, block_row=block_row[:M // 64])
                    if normals:
                        out["samples"].update(surface_pts=surf_pts, surface_entity=surf_entity)
        samples = out.pop("samples", None)
        res = shape(out)
        if samples is not None:
            res["samples"] = samples
        return res


def render_to_files(result, out_dir):
    """rgb.png (8 bit), depth.png (16 bit, millimetres) and instance.png (16 bit, -1 as 65535), transposed back to H x W; with a
    ``normal`` image in the result also normal.png (8 bit, n * 0.5 + 0.5)."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    rgb = (result["rgb"].detach().clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy().transpose(1, 0, 2)
    Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(os.path.join(out_dir, "rgb.png"))
    mm = (result["depth"].detach().double() * 1000).round().clamp(0, 65535).cpu().numpy().astype(np.uint16).T
    Image.fromarray(np.ascontiguousarray(mm)).save(os.path.join(out_dir, "depth.png"))
    inst = result["instance"].detach().cpu().numpy().astype(np.int64).T
    if inst.max(initial=-1) >= 65535:
        raise ValueError("instance ids above 65534 do not fit a 16-bit image")
    Image.fromarray(np.ascontiguousarray(np.where(inst < 0, 65535, inst).astype(np.uint16))).save(os.path.join(out_dir, "instance.png"))
    if "normal" in result:
        Image.fromarray(encode_normals(result["normal"]), "RGB").save(os.path.join(out_dir, "normal.png"))


def encode_normals(normal):
    """normal (W,H,3) in [-1,1] -> (H,W,3) uint8 = round((n * 0.5 + 0.5) * 255); the zero vector (no surface) is grey 128"""
    n = (normal.detach().float().cpu().clamp(-1, 1) * 0.5 + 0.5) * 255
    return np.ascontiguousarray(n.round().to(torch.uint8).numpy().transpose(1, 0, 2))


def shade(result, T_wc):
    """A grey headlight Lambert image (W,H,3) float32 in [0,1] from a render made with ``normals=True``: max(0, -n . v), v the
    view direction = the camera's optical axis in the world frame (the third column of ``T_wc``'s rotation, normalised: a
    light at the camera, parallel rays).  Zero where the normal is zero or faces away."""
    if "normal" not in result:
        raise ValueError("shade wants a render made with normals=True")
    n = result["normal"].detach().float()
    T = np.asarray(T_wc.detach().cpu() if torch.is_tensor(T_wc) else T_wc, np.float64).reshape(4, 4)
    v = T[:3, 2] / np.linalg.norm(T[:3, 2])
    lam = (-(n * torch.as_tensor(v, dtype=torch.float32, device=n.device)).sum(-1)).clamp(min=0.0)
    return lam[..., None].expand(*lam.shape, 3).contiguous()
