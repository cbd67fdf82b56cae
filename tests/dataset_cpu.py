"""TEST INFRASTRUCTURE: numpy restatement of csrc/frames.hip.

``CpuFrameTable`` has the interface of ``cnr_amd.dataset.FrameTable`` and builds each frame's instance table the way the
reference's get_all_frames does, one full-frame mask comparison per instance (O(instances x pixels)); ``finish`` writes the
frame arrays.  ``resize_linear`` / ``resize_nearest`` restate OpenCV's INTER_LINEAR (8-bit, 3 channels) and INTER_NEAREST.
``cpu_loader()`` swaps these in for the device kernels, so the loaders' host logic runs on a machine without a GPU."""
import contextlib

import numpy as np
import torch

ID_BOUND = 65537


def _np(t):
    return t.numpy() if torch.is_tensor(t) else np.asarray(t)


class CpuFrameTable:
    def __init__(self, inst, cls=None, edge=0, id_shift=0):
        self.inst, self.cls, self.edge, self.id_shift = _np(inst), None if cls is None else _np(cls), edge, id_shift
        F, Hs, Ws = self.inst.shape
        self.F, self.H, self.W = F, Hs - 2 * edge, Ws - 2 * edge
        ids, stats, offsets = [], [], [0]
        for f in range(F):
            lab = self._labels(f)
            k = self._crop(self.cls[f]).astype(np.int64) if self.cls is not None else np.zeros_like(lab)
            for v in np.unique(lab[(lab >= 0) & (lab < ID_BOUND)]):
                m = lab == v
                r, c = np.nonzero(m)
                ids.append(v)
                stats.append([m.sum(), r.min(), r.max(), c.min(), c.max(), k[m].min(), k[m].max()])
            offsets.append(len(ids))
        self.ids = np.array(ids, np.int32)
        self.stats = np.array(stats, np.int32).reshape(-1, 7)
        self.offsets = np.array(offsets, np.int64)

    def _crop(self, a, e=None):
        e = self.edge if e is None else e
        return a[e:a.shape[0] - e, e:a.shape[1] - e]

    def _labels(self, f):
        return self._crop(self.inst[f]).astype(np.int64) + self.id_shift

    def frame(self, f):
        a, b = self.offsets[f], self.offsets[f + 1]
        return self.ids[a:b], self.stats[a:b]

    def finish(self, keep, depth, rgb, edge, depth_scale, max_depth):
        depth, rgb = _np(depth), _np(rgb)
        obj, dep, img = [], [], []
        for f in range(self.F):
            lab = self._labels(f)
            ids = self.ids[self.offsets[f]:self.offsets[f + 1]]
            kept = ids[np.asarray(keep[self.offsets[f]:self.offsets[f + 1]], bool)]
            obj.append(np.where(np.isin(lab, kept), lab, 0).astype(np.int32).T)
            d = self._crop(depth[f], edge).astype(np.float32) * np.float32(depth_scale)
            d[np.isnan(d) | (d > np.float32(max_depth))] = 0.0
            dep.append(d.T)
            img.append(self._crop(rgb[f], edge).transpose(1, 0, 2))
        return [torch.from_numpy(np.ascontiguousarray(np.stack(a))) for a in (obj, dep, img)]


def _linear_coef(d, ssize, scale, clamp):
    fx = np.float32((d + 0.5) * scale - 0.5)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    if clamp:
        lo = sx < 0
        fx[lo], sx[lo] = 0, 0
        hi = sx >= ssize - 1
        fx[hi], sx[hi] = 0, ssize - 1
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    return np.clip(sx, 0, ssize - 1), np.clip(sx + 1, 0, ssize - 1), a0, a1


def resize_linear(src, dh, dw):
    """cv2.resize(INTER_LINEAR) on (F, sh, sw, 3) uint8: OpenCV's 11-bit coefficients, exact horizontal pass, the vertical pass
    of its vectorised 32s -> 8u kernel"""
    a = _np(src).astype(np.int64)
    F, sh, sw, _ = a.shape
    x0, x1, a0, a1 = _linear_coef(np.arange(dw, dtype=np.float64), sw, 1.0 / (dw / sw), True)
    y0, y1, b0, b1 = _linear_coef(np.arange(dh, dtype=np.float64), sh, 1.0 / (dh / sh), False)
    h = a[:, :, x0] * a0[None, None, :, None] + a[:, :, x1] * a1[None, None, :, None]          # (F, sh, dw, 3)
    v = ((h[:, y0] >> 4) * b0[None, :, None, None] >> 16) + ((h[:, y1] >> 4) * b1[None, :, None, None] >> 16)
    return torch.from_numpy(np.clip((v + 2) >> 2, 0, 255).astype(np.uint8))


def resize_nearest(src, dh, dw):
    a = _np(src)
    F, sh, sw = a.shape
    sy = np.minimum(np.floor(np.arange(dh) * (1.0 / (dh / sh))).astype(np.int64), sh - 1)
    sx = np.minimum(np.floor(np.arange(dw) * (1.0 / (dw / sw))).astype(np.int64), sw - 1)
    return torch.from_numpy(np.ascontiguousarray(a[:, sy][:, :, sx]))


@contextlib.contextmanager
def cpu_loader():
    """cnr_amd.dataset with this restatement in place of the device kernels (and no pinned uploads)"""
    from cnr_amd import dataset as D
    saved = (D.FrameTable, D.resize_linear, D.resize_nearest, D._pinned, D._Base._parse_device)
    D.FrameTable, D.resize_linear, D.resize_nearest = CpuFrameTable, resize_linear, resize_nearest
    D._pinned = lambda arrays: torch.from_numpy(np.stack(arrays))
    D._Base._parse_device = lambda self: torch.device("cpu")
    try:
        yield D
    finally:
        D.FrameTable, D.resize_linear, D.resize_nearest, D._pinned, D._Base._parse_device = saved
