"""TEST INFRASTRUCTURE: the occupancy grids of the scene view renderer's empty-space skipping restated (include/cnr_hip.h,
cnr_view_grid_* and cnr_view_active_*): bit packing, cells and dilation as torch max-pools, and the sample -> cell lookup in
float64 on top of tests/view_cpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

import view_cpu as V


def pack(bits):
    """(..., G, G, G) bool numpy -> (..., G^3/32) int32: cell l = (ix G + iy) G + iz is bit l & 31 of word l >> 5"""
    b = np.asarray(bits, bool)
    flat = b.reshape(b.shape[:-3] + (-1, 32)).astype(np.uint64)
    w = (flat << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return w.view(np.int32)


def unpack(words, G):
    w = np.ascontiguousarray(words, np.int32).view(np.uint32)
    bits = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.astype(bool).reshape(w.shape[:-1] + (G, G, G))


def cells(occ, G, sub, tau):
    """cnr_view_grid_cells: (D,D,D) float32 -> (G,G,G) bool; a cell owns [i sub, (i+1) sub] per axis; set iff some !(v < tau)"""
    v = torch.as_tensor(occ, dtype=torch.float32)
    assert v.shape == (G * sub + 1,) * 3
    hot = (~(v < np.float32(tau))).float()[None, None]
    return F.max_pool3d(hot, kernel_size=sub + 1, stride=sub)[0, 0].bool().numpy()


def dilate(bits, r):
    """cnr_view_grid_dilate: Chebyshev radius r, clamped at the faces (max_pool3d pads with -inf)"""
    b = torch.as_tensor(np.asarray(bits, bool)).float()[None, None]
    return F.max_pool3d(b, kernel_size=2 * r + 1, stride=1, padding=r)[0, 0].bool().numpy()


def cell_of(b, G):
    """box coordinates (...,3) float64 -> (cell indices (...,3) int, near (...) bool: within 1e-3 cell of a cell face)"""
    u = (np.asarray(b, np.float64) + 1.0) * 0.5 * G
    c = np.clip(np.floor(u), 0, G - 1).astype(np.int64)
    near = (np.abs(u - np.round(u)) < 1e-3).any(-1)
    return c, near


def lookup(T_wc, dirs, to_box, seg_pixel, seg_entity, seg_z, S, bits, entity_grid):
    """The active set in float64.  bits (grids,G,G,G) bool, entity_grid (E,) the grid of every entity or -1 (none: all set)
    -> active (N,S) bool, near (N,S) bool (the samples a float32 lookup may place in the neighbouring cell)."""
    G = bits.shape[-1]
    r32 = lambda a: np.asarray(a, np.float32)
    _, b = V.points(r32(T_wc), r32(dirs), r32(to_box), seg_pixel, seg_entity, r32(seg_z), S, np.float64)
    c, near = cell_of(b, G)
    g = np.asarray(entity_grid)[seg_entity][:, None]                            # (N,1)
    active = np.asarray(bits, bool)[np.maximum(g, 0), c[..., 0], c[..., 1], c[..., 2]] | (g < 0)
    return active, near & (g >= 0)


def masked_composite_inputs(sigma, color, active):
    """the specification of a skipped render: the full render's samples with sigma = -inf, colour = 0 where inactive"""
    a = torch.as_tensor(active, device=sigma.device)
    return (torch.where(a, sigma, torch.full_like(sigma, float("-inf"))).contiguous(),
            torch.where(a[..., None], color, torch.zeros_like(color)).contiguous())
