"""The device-resident ray pool of a captured train step: C pools stacked over classes, read in slices of ``Rg`` rows through
an index permutation that is redrawn at every epoch end (the pool itself never moves), with the epoch's per-slice tables beside it
and the host's mirror of the device cursor.  One type for the category step (fused.FusedCategoryTrainer: C classes, ragged
lengths, ray shards) and the background step (background.BackgroundStep: one class)."""
import torch

from . import _C


class RayPool:
    def __init__(self, pools, device, Rg, ray_world=1, ray_rank=0, R=None, seed=0, class_ids=None, min_depth=0.0,
                 indices=True, tables=True):
        """``pools``: per class a dict of rgbs (N,4), depth (N,), dirs (N,3), T (N,4,4) -- the pose the sampler is to read,
        chosen by the caller -- and, with ``indices``, indices (N,).  ``Rg`` rows per global slice, of which this rank takes rows
        ``[ray_rank R, ray_rank R + R)``.  ``seed``, the epoch and the GLOBAL class id (``class_ids``: int32 device tensor, None =
        0 .. C-1) key the permutations.  ``tables``: keep ``slice_max`` / ``counts_tab`` (``min_depth``: a valid depth is above it)."""
        self.device, self.C, self.Rg, self.ray_world = torch.device(device), len(pools), int(Rg), int(ray_world)
        # Pools of different lengths (every real scene: src/scene_cateogries.py:164-260) are padded to the longest; a padding row is
        # never referenced: the step reaches the pool only through `perm`, which reshuffle() fills per class from the class's OWN rows
        self.rows_cls = [int(p["depth"].shape[0]) for p in pools]
        self.rows = max(self.rows_cls)
        self.ragged = min(self.rows_cls) != self.rows
        assert min(self.rows_cls) >= 2 * self.Rg, "every class's pool must hold two slices of rays"
        assert not self.ragged or class_ids is not None

        def padded(t):
            t = t.to(self.device)
            return t if t.shape[0] == self.rows else torch.cat([t, t[:1].expand(self.rows - t.shape[0], *t.shape[1:])])
        st = lambda k: torch.stack([padded(p[k]) for p in pools]).contiguous()
        self.rgbs, self.depth, self.dirs, self.T = st("rgbs"), st("depth"), st("dirs"), st("T")
        self.indices = st("indices") if indices else None
        # epoch shuffle as an index permutation (C, rows), a function of seed, epoch and global class id: the same on every rank
        self.perm = torch.empty(self.C, self.rows, device=self.device, dtype=torch.int32)
        self.seed, self.class_ids, self.min_depth, self._epoch = int(seed), class_ids, float(min_depth), 0
        self.cursor0 = int(ray_rank) * int(self.Rg if R is None else R)     # this rank's first row of a global slice
        # ragged pools, per class: the epoch it is in and the slice of that epoch its next permutation row starts with (_ragged_perm)
        self._cls_epoch, self._cls_slice = [0] * self.C, [0] * self.C
        if self.ragged:
            self._perm_scratch = torch.empty(self.rows, device=self.device, dtype=torch.int32)
            self._cursor0 = torch.tensor([self.cursor0], device=self.device, dtype=torch.int64)
        # per-epoch tables, one entry per LOCAL slice (index = device cursor / R): the (global) slice's max depth (scene_cateogries.py:486)
        # and its mask counts + any-class-empty flags (render_rays.py:66-95) -- no step computes a maximum or counts a mask
        self.n_gslices = self.rows // self.Rg
        self.n_slices = self.n_gslices * self.ray_world
        self.slice_max = torch.zeros(self.C, self.n_slices, device=self.device) if tables else None
        self.counts_tab = torch.zeros(self.n_slices, self.C + 1, 4, device=self.device) if tables else None
        self.cursor = 0           # host mirror of the device cursor, in rows of the global slices

    def due(self):
        """the epoch is over: the next step needs a reshuffle first (i_batch >= N - n, scene_cateogries.py:439-449)"""
        return self.cursor >= self.rows - self.Rg

    def steps_left(self):
        """steps before the next reshuffle"""
        return -(-(self.rows - self.Rg - self.cursor) // self.Rg)

    def advance(self, U=1):
        self.cursor += U * self.Rg

    def reshuffle(self, d_state_row):
        """New permutation, the cursor of the state copy ``d_state_row`` (int64[3], the one the next step reads) back to this
        rank's first row (scene_cateogries.py:439-449), and the epoch's tables per GLOBAL slice (cnr_slice_maxdepth,
        cnr_slice_maskcounts), each entry repeated for the ray ranks that share the slice (they index by their own cursor / R)."""
        C, ng, w = self.C, self.n_gslices, self.ray_world
        if self.ragged:
            self._ragged_perm(d_state_row)
        else:
            # one launch: a keyed bijection per (seed, epoch, GLOBAL class id) and the cursor of the state copy
            _C.call("cnr_epoch_perm", self.perm, self.rows, C, self.seed, self._epoch, self.class_ids, d_state_row, self.cursor0)
            self._epoch += 1
        self.cursor = 0
        if self.slice_max is None:
            return
        direct = w == 1        # no ray shards: the tables go straight into the buffers the kernels read
        smax = self.slice_max if direct else torch.empty(C, ng, device=self.device)
        _C.call("cnr_slice_maxdepth", self.depth, self.perm, self.rows, C, self.Rg, ng, smax)
        tab = self.counts_tab if direct else torch.empty(ng, C + 1, 4, device=self.device)
        _C.call("cnr_slice_maskcounts", self.rgbs, self.depth, self.perm, self.rows, C, self.Rg, ng, self.min_depth, tab)
        if not direct:
            self.slice_max.copy_(smax.repeat_interleave(w, dim=1))
            self.counts_tab.copy_(tab.repeat_interleave(w, dim=0))

    def _ragged_perm(self, d_state_row):
        """Pools of different lengths.  The reference gives every category its own cursor: class c takes slices of n rows and
        reshuffles ITS pool when i_batch >= N_c - n (src/scene_cateogries.py:436-449), i.e. after k_c = ceil(N_c / n) - 1 slices.
        The step's kernels share one device cursor, so the permutation row of class c is laid out as what that class will read
        over the next K = max_c k_c steps: the rest of its current epoch's order, then as many further epochs of ITS OWN pool
        (each a keyed bijection of (seed, class epoch, global class id) on [0, N_c): cnr_epoch_perm) as fit.  Where a class is
        in its epoch carries over to the next call.  Host work per (longest-class) epoch, nothing per step."""
        Rg = self.Rg
        K = -(-self.rows // Rg) - 1                    # steps until the host reshuffles again (= the longest class's epoch)
        for c, N in enumerate(self.rows_cls):
            k_c = -(-N // Rg) - 1                      # slices per epoch of this class
            row, filled = self.perm[c], 0
            while filled < K:
                _C.call("cnr_epoch_perm", self._perm_scratch, N, 1, self.seed, self._cls_epoch[c], self.class_ids[c:c + 1], None, 0)
                take = min(k_c - self._cls_slice[c], K - filled)
                a = self._cls_slice[c] * Rg
                row[filled * Rg:(filled + take) * Rg].copy_(self._perm_scratch[a:a + take * Rg])
                filled += take
                self._cls_slice[c] += take
                if self._cls_slice[c] == k_c:
                    self._cls_slice[c], self._cls_epoch[c] = 0, self._cls_epoch[c] + 1
            row[K * Rg:].zero_()                       # never read (the host reshuffles after K slices); kept in range
        d_state_row[0:1].copy_(self._cursor0)
