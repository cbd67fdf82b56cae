"""Model holder with the reference's surface (src/trainer.py:11-60,125-151): ``.pe``,
``.fc_occ_map``, ``.shape_codes``, ``.texture_codes``, ``.inst_id_to_index``, ``.n_obj``,
``.obj_scale``, ``.emb_size1/2``, ``.eval_points``, ``.meshing`` (the grid evaluation, marching cubes and colour pass
on the GPU; returns a :class:`vis.Mesh`)."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import embedding, meshops, model, render_rays, vis


class Trainer:
    def __init__(self, cfg, cls_id, inst_ids):
        self.cls_id = cls_id
        self.inst_id_to_index = {inst_id: inst_ids.index(inst_id) for inst_id in inst_ids}
        self.n_obj = len(inst_ids)
        self.device = cfg.training_device
        self.obj_scale = cfg.obj_scale
        self.n_unidir_funcs = cfg.n_unidir_funcs
        self.emb_size1 = 21 * (3 + 1) + 3
        self.emb_size2 = 21 * (5 + 1) + 3 - self.emb_size1
        if cls_id == 0:      # background: vMAP OccupancyMap, no codes (src/trainer.py:23-25)
            self.hidden_feature_size = cfg.hidden_feature_size
            self.load_NeRF()
        else:
            self.net_hyperparams = cfg.net_hyperparams
            self.load_codeNeRF()
            self.load_codes()
        self.extent_dict = None
        self.bound_extent = 0.995 if cls_id == 0 else 0.9
        self.scale_template = None
        # eval_points of the BACKGROUND field: "fp32" = the exact modules (2e-5 of the reference; the default), "fused" = the f16-MFMA
        # forward of csrc/bg_fused.hip (hidden size 128: occupancy 1e-6, colour 2e-4 on trained weights -- inside north_star's 1e-3 --
        # and an order of magnitude faster: the reference's own note on this function is "2s/it 1000000 pts", src/trainer.py:134)
        self.eval_precision = "fp32"

    def load_NeRF(self):
        self.fc_occ_map = model.OccupancyMap(self.emb_size1, self.emb_size2,
                                             hidden_size=self.hidden_feature_size).to(self.device)
        self.fc_occ_map.apply(model.init_weights).to(self.device)
        self.pe = embedding.UniDirsEmbed(max_deg=self.n_unidir_funcs, scale=self.obj_scale).to(self.device)

    def load_codeNeRF(self):
        self.fc_occ_map = model.CodeNeRF(self.emb_size1, self.emb_size2, **self.net_hyperparams).to(self.device)
        self.fc_occ_map.apply(model.init_weights).to(self.device)
        self.pe = embedding.UniDirsEmbed(max_deg=self.n_unidir_funcs, scale=self.obj_scale).to(self.device)

    def load_codes(self):
        embdim = self.net_hyperparams['latent_dim']
        d = self.n_obj
        self.shape_codes = nn.Embedding(d, embdim)
        self.texture_codes = nn.Embedding(d, embdim)
        self.shape_codes.weight = nn.Parameter(torch.randn(d, embdim) / math.sqrt(embdim / 2))
        self.texture_codes.weight = nn.Parameter(torch.randn(d, embdim) / math.sqrt(embdim / 2))
        self.shape_codes = self.shape_codes.to(self.device)
        self.texture_codes = self.texture_codes.to(self.device)

    def meshing(self, inst_id=None, grid_dim=256, normals="grid", clean=None, simplify=None):
        """src/trainer.py:62-123: occupancy on a grid_dim^3 grid over the object's box, marching cubes at 0.5 ('ascent'),
        back to scene coordinates, vertex colours from eval_points.  None where the reference returns None.
        normals: "grid" = the lattice differences marching cubes interpolates (skimage's, faceted on a coarse grid); "field" =
        the field's own gradient at every vertex (eval_gradient), normalised, pointing towards increasing occupancy as the grid
        normals do (vis.py); a vertex whose gradient is exactly zero keeps its grid normal.
        clean: None, or a dict of meshops.clean_mesh options (keep_largest=1, min_faces=..., weld=...): the floaters are dropped on
        the device, in scene coordinates, BEFORE the colour pass, so the field is never evaluated at a dropped vertex; the report is
        left in self.last_clean_report.
        simplify: None, or a dict of meshops.simplify options (cell=... or target_faces=..., placement=..., tau=...): vertex
        clustering with quadric placement on the device, in scene coordinates, AFTER clean and BEFORE the colour pass, so the
        colours are the field's at the new vertices; normals="grid" then means meshops.vertex_normals of the output faces.  The
        report is left in self.last_simplify_report; None when no face survives."""
        if normals not in ("grid", "field"):
            raise ValueError("normals must be 'grid' or 'field', not {!r}".format(normals))
        occ_range = [-1., 1.]
        range_dist = occ_range[1] - occ_range[0]
        boxed = self.cls_id == 0 or self.n_obj == 1
        if boxed:
            bound = self.bound if self.cls_id == 0 else self.bound_dict[inst_id]
            scale_np = bound.extent / (range_dist * self.bound_extent)
            scale = torch.from_numpy(np.asarray(scale_np)).float().to(self.device)
            transform_np = np.eye(4, dtype=np.float32)
            transform_np[:3, 3] = bound.center
            transform_np[:3, :3] = bound.R
            transform = torch.from_numpy(transform_np).to(self.device)
            grid_pc = render_rays.make_3D_grid(occ_range=occ_range, dim=grid_dim, device=self.device,
                                               scale=scale, transform=transform).view(-1, 3)
        else:
            extent = self.extent_dict[inst_id]
            extent = extent / np.max(extent / 2)
            scale_np = extent / (range_dist * self.bound_extent)
            scale = torch.from_numpy(np.asarray(scale_np)).float().to(self.device)
            grid_pc = render_rays.make_3D_grid(occ_range=occ_range, dim=grid_dim, device=self.device, scale=scale).view(-1, 3)
        if self.cls_id == 0:
            ret = self.eval_points(grid_pc)
            occ = None if ret is None else ret[0]
        else:
            occ = self._grid_occupancy(grid_pc, inst_id)
        if occ is None:
            return None
        mesh = vis.marching_cubes(occ.view(grid_dim, grid_dim, grid_dim))
        if mesh is None:
            print("marching cube failed")
            return None
        mesh.apply_translation([-0.5, -0.5, -0.5])      # to [-1, 1]
        mesh.apply_scale(2)
        mesh.apply_scale(scale_np)                       # to scene coordinates
        if boxed:
            mesh.apply_transform(transform_np)
        if clean is not None:
            mesh, self.last_clean_report = meshops.clean_mesh(mesh, device=self.device, **dict(clean))
        if simplify is not None:
            # the lattice normals do not exist at moved vertices: "grid" takes the output faces' own (simplify_mesh's), "field"
            # replaces them below
            mesh, self.last_simplify_report = meshops.simplify_mesh(mesh, device=self.device, **dict(simplify))
            if len(mesh.faces) == 0:
                print("simplification left no face")
                return None
        vertices_pts = torch.from_numpy(np.array(mesh.vertices)).float().to(self.device)
        ret = self.eval_points(vertices_pts) if self.cls_id == 0 else self.eval_points(vertices_pts, inst_id=inst_id)
        if ret is None:
            return None
        _, color = ret
        mesh.visual.vertex_colors = (color * 255).detach().squeeze(0).cpu().numpy().astype(np.uint8)
        if normals == "field":
            # the mesh has been moved to the coordinates the field takes (eval_points reads its vertices as they are), so the
            # map from vertex to field point is the identity and M^T grad sigma is grad sigma itself
            _, g = self.eval_gradient(vertices_pts, inst_id=inst_id)
            g = g.double().cpu().numpy()
            ln = np.linalg.norm(g, axis=1, keepdims=True)
            ok = (ln > 0) & np.isfinite(ln)
            mesh.vertex_normals = np.where(ok, g / np.where(ok, ln, 1.0), mesh.vertex_normals)
        return mesh

    def eval_gradient(self, points, inst_id=None, chunk_size=500000):
        """The companion of eval_points: (sigma (N,), grad (N,3)) at (N,3) points in the frame eval_points takes them in --
        sigma the x10 occupancy logit (occupancy = sigmoid(sigma)), grad = d sigma / d points.  One cnr_field_grad /
        cnr_occmap_grad launch per chunk (exact fp32, forward mode: DESIGN.md section 3.15); no autograd graph is built."""
        from . import ops
        sigma, grad = [], []
        with torch.no_grad():
            if self.cls_id != 0:
                trunk, B, brows = self._codenerf_rows(inst_id)
            for k in range(0, max(points.shape[0], 1), chunk_size):
                pts = points[k:k + chunk_size].float().contiguous()
                if self.cls_id != 0:
                    s, g = ops.field_grad(pts, B, trunk, brows, None, self.pe._scale)
                else:
                    s, g = ops.occmap_grad(self.fc_occ_map, self.pe, pts)
                sigma.append(s)
                grad.append(g)
        return torch.cat(sigma), torch.cat(grad)

    def _codenerf_rows(self, inst_id):
        """(trunk (1,13892), B (1,21,3), bias rows (1,4,32)) of one object of this CodeNeRF category"""
        from . import ops
        fc = self.fc_occ_map
        obj_idx = torch.tensor(self.inst_id_to_index[inst_id], device=self.device)
        shape_code, texture_code = self.shape_codes(obj_idx), self.texture_codes(obj_idx)
        trunk = torch.cat([t.reshape(1, -1) for n, _, _ in ops.TRUNK_LAYERS
                           for t in (fc._linear(n).weight, fc._linear(n).bias)], dim=1).contiguous()
        zlat = fc.latent_rows(shape_code.view(1, 1, -1), texture_code.view(1, 1, -1))       # (1,4,32)
        brows = ops.bias_rows(trunk, zlat[None]).reshape(1, 4, 32).contiguous()
        B = self.pe.B_layer.weight.reshape(1, 21, 3).contiguous()
        return trunk, B, brows

    def _grid_occupancy(self, grid_pc, inst_id):
        """Occupancy of a whole meshing grid in ONE cnr_field_fwd launch on the precise geometry branch (packed_lo: the
        split-weight products of DESIGN.md §3.3, 2e-6 of the exact occupancy on trained weights where plain f16 gives 1.8e-3 and
        moves surface vertices).  None when nothing is occupied, as eval_points."""
        from . import ops
        with torch.no_grad():
            trunk, B, brows = self._codenerf_rows(inst_id)
            row = torch.zeros(1, 1, device=grid_pc.device, dtype=torch.int32)
            sig, _ = ops.field_fwd(grid_pc.float().contiguous().view(1, 1, -1, 3), B, ops.pack_weights(trunk), brows, row,
                                   self.pe._scale, packed_lo=ops.pack_weights_lo(trunk))
            occ = render_rays.occupancy_activation(sig.reshape(-1))
        if occ.max() == 0:
            print("no occ")
            return None
        return occ

    def eval_points(self, points, inst_id=None, chunk_size=500000):
        """Forward-only occupancy / colour of (N,3) points for one object (src/trainer.py:125-151) -> (occ (N,),
        color (N,3)) or None when nothing is occupied.

        CodeNeRF categories run the fused f16-MFMA forward (cnr_field_fwd: PE + the ten layers in one launch per chunk,
        12 B in / 16 B out per point; the reference materialises a 516 B embedding per point and runs ten GEMMs): the
        object's code reaches the kernel as ONE effective bias row, the chunk is a single "ray" of n samples.  The
        background OccupancyMap keeps the exact-fp32 modules (PE kernel + dense kernels)."""
        n_chunks = int(np.ceil(points.shape[0] / chunk_size))
        alpha, color = [], []
        with torch.no_grad():
            if self.cls_id != 0:
                from . import ops
                trunk, B, brows = self._codenerf_rows(inst_id)
                packed = ops.pack_weights(trunk)
                row = torch.zeros(1, 1, device=points.device, dtype=torch.int32)
                for k in range(n_chunks):
                    pts = points[k * chunk_size:(k + 1) * chunk_size].float().contiguous()
                    sig, rgb = ops.field_fwd(pts.view(1, 1, -1, 3), B, packed, brows, row, self.pe._scale)
                    alpha.append(sig.reshape(-1))
                    color.append(rgb.reshape(-1, 3))
            elif self.eval_precision == "fused" and self.hidden_feature_size == 128:
                from . import _C
                flat = torch.cat([p.reshape(-1) for p in self.fc_occ_map.parameters()] + [self.pe.B_layer.weight.reshape(-1)]).contiguous()
                assert flat.numel() == int(_C.load().cnr_bg_param_count())
                packed = torch.empty(int(_C.load().cnr_bg_pack_bytes()), device=flat.device, dtype=torch.uint8)
                _C.call("cnr_bg_pack", flat, packed)
                for k in range(n_chunks):
                    pts = points[k * chunk_size:(k + 1) * chunk_size].float().contiguous()
                    M = pts.shape[0]
                    sig, rgb = torch.empty(M, device=pts.device), torch.empty(M, 3, device=pts.device)
                    _C.call("cnr_bg_forward", pts, flat, packed, float(self.pe._scale), M, sig, rgb, None, None)
                    alpha.append(sig)
                    color.append(rgb)
            else:
                for k in range(n_chunks):
                    emb = self.pe(points[k * chunk_size:(k + 1) * chunk_size, None, :])
                    a_k, c_k = self.fc_occ_map(emb)
                    alpha.append(a_k.reshape(-1))
                    color.append(c_k.reshape(-1, 3))
        alpha, color = torch.cat(alpha), torch.cat(color)
        occ = render_rays.occupancy_activation(alpha).detach()
        if occ.max() == 0:
            print("no occ")
            return None
        return (occ, color)
