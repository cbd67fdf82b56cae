"""GPU: the sampler of the step's first launch with its draws and its sort under its loads (csrc/sample_common.h,
sample_ray_pool) leaves, bit for bit, what cnr_sample_rays (sample_ray) leaves -- on every shape at which it takes another path,
with all four z branches in the batch -- and a pool it may not take (a pose table off its 16-byte alignment) goes through
sample_ray inside the same launch, with the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("z", "pts", "gt_rgb", "gt_depth", "depth_mask", "labels", "ray_row")


@pytest.fixture(scope="module")
def cnr(dev):
    import cnr_amd
    return cnr_amd


# (C, n_obj, R, n1, n2): 50 x (1 + 9): a block with two idle waves, ten columns; 64 x 64; 32 x (16 + 112): the 128-element sort and
# the second pass of the z loop; two classes of three objects, 65 columns: one column in the second pass
CASES = [(1, 4, 50, 1, 9), (1, 4, 64, 8, 56), (1, 4, 32, 16, 112), (2, 3, 50, 9, 56)]


@pytest.mark.parametrize("C,n_obj,R,n1,n2", CASES)
def test_prologue_sampler_equals_cnr_sample_rays(cnr, dev, C, n_obj, R, n1, n2):
    _C, ops = cnr._C, cnr.ops
    L = 32
    gen = torch.Generator().manual_seed(100 * R + n1 + n2 + C)
    pool_rows = 6 * R + 7
    pools = [cnr.scene_cateogries.synthetic_pool(pool_rows, n_obj, gen, "cpu") for _ in range(C)]
    perm_h = torch.stack([torch.randperm(pool_rows, generator=gen) for _ in range(C)])
    cursor, step = 2 * R, 7
    # rows of the slice: a handful with depth <= min_depth, a handful of each non-object state, a handful of this-object rows
    # with a depth -- all four z branches (invalid | s < n1 | this object | other object) occur
    for c in range(C):
        rows = perm_h[c, cursor:cursor + R]
        pools[c]["depth"][rows[0:3]] = 0.0
        pools[c]["rgbs"][rows[3:6], 3] = 0
        pools[c]["rgbs"][rows[6:8], 3] = 2
        pools[c]["rgbs"][rows[8:12], 3] = 1
        pools[c]["depth"][rows[3:12]] = torch.linspace(0.7, 2.9, 9)
    st = lambda k: torch.stack([p[k] for p in pools]).to(dev).contiguous()
    rgbs, depth, dirs, T, idx = st("rgbs"), st("depth"), st("dirs"), st("T_co"), st("indices")
    perm = perm_h.to(torch.int32).to(dev)
    nsl = pool_rows // R
    table = torch.empty(C, nsl, device=dev)
    _C.call("cnr_slice_maxdepth", depth, perm, pool_rows, C, R, nsl, table)
    state = torch.tensor([cursor, step, 11], dtype=torch.int64, device=dev)
    want = ops.sample_rays(rgbs, depth, dirs, T, n1, n2, 0.1, 0.05, seed=9, d_state=state, rays=R, out={}, max_bound=table,
                           pool_indices=idx, n_obj=n_obj, perm=perm, max_bound_slices=nsl)
    lab, msk = want["labels"], want["depth_mask"]
    assert bool((msk == 0).any()) and bool(((lab == 1) & (msk == 1)).any()) and bool(((lab != 1) & (msk == 1)).any())
    theta, lay = cnr.fused.init_params(C, L, n_obj, gen, dev)
    # the pose table once as it is (16-byte aligned: sample_ray_pool) and once four bytes further on (sample_ray)
    shifted = torch.empty(T.numel() + 1, device=dev)[1:].view_as(T).copy_(T)
    assert T.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for poses in (T, shifted):
        got = ops.step_prologue(theta, lay, L, n_obj, torch.empty(C, _C.pack_bytes(), device=dev, dtype=torch.uint8),
                                torch.empty(C * n_obj, 4, 32, device=dev), torch.empty(C * n_obj, 4, 32, device=dev),
                                torch.zeros(1000, device=dev), rgbs, depth, dirs, poses, n1, n2, 0.1, 0.05, 0.0, 9, state, R, {},
                                table, idx, perm, max_bound_slices=nsl)
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (k, poses is T, int((got[k] != want[k]).sum()))
    # ... and without a permutation (identity), per-class maxima instead of the table
    mb = torch.empty(C, device=dev)
    _C.call("cnr_sample_maxdepth", depth, mb, state, pool_rows, None, C, R)
    want = ops.sample_rays(rgbs, depth, dirs, T, n1, n2, 0.1, 0.05, seed=9, d_state=state, rays=R, out={}, max_bound=mb,
                           pool_indices=idx, n_obj=n_obj)
    got = ops.step_prologue(theta, lay, L, n_obj, torch.empty(C, _C.pack_bytes(), device=dev, dtype=torch.uint8),
                            torch.empty(C * n_obj, 4, 32, device=dev), torch.empty(C * n_obj, 4, 32, device=dev),
                            torch.zeros(1000, device=dev), rgbs, depth, dirs, T, n1, n2, 0.1, 0.05, 0.0, 9, state, R, {}, mb, idx, None)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), (k, "identity")
