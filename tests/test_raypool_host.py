"""CPU: the host logic of the ray pool (raypool.RayPool: padding, ragged permutation rows, epoch arithmetic, per-epoch tables,
their repetition for ray shards) and the shard plan (parallel.shard_plan), with the three pool launches replaced by a test
double: cnr_epoch_perm as a deterministic bijection keyed by (seed, epoch, global class id), the two tables as plain torch."""
import pytest
import torch


def order(seed, epoch, cid, n):
    """the double's epoch order of a pool of n rows"""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(epoch) * 1009 + int(cid))
    return torch.randperm(n, generator=g).to(torch.int32)


class PoolDouble:
    def cnr_epoch_perm(self, perm, rows, C, seed, epoch, class_ids, d_state, cursor0):
        for c in range(C):
            cid = c if class_ids is None else int(class_ids[c])
            perm.view(-1)[c * rows:(c + 1) * rows] = order(seed, epoch, cid, rows)
        if d_state is not None:
            d_state[0] = cursor0

    def cnr_slice_maxdepth(self, depth, perm, rows, C, Rg, ng, out):
        for c in range(C):
            out[c] = depth[c][perm[c, :ng * Rg].long()].reshape(ng, Rg).max(dim=1).values

    def cnr_slice_maskcounts(self, rgbs, depth, perm, rows, C, Rg, ng, min_depth, tab):
        from cnr_amd import parallel
        for s in range(ng):
            idx = perm[:, s * Rg:(s + 1) * Rg].long()
            labels = torch.stack([rgbs[c, idx[c], 3] for c in range(C)]).to(torch.uint8)
            valid = torch.stack([depth[c, idx[c]] > min_depth for c in range(C)])
            tab[s] = parallel.mask_count_table(labels, valid)


@pytest.fixture()
def cnr():
    import cnr_amd
    cnr_amd._C.install_test_double(PoolDouble())
    yield cnr_amd
    cnr_amd._C.install_test_double(None)


def make_pools(lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    pools = []
    for n in lengths:
        rgbs = torch.rand(n, 4, generator=g)
        rgbs[:, 3] = torch.randint(0, 3, (n,), generator=g).float()
        depth = torch.rand(n, generator=g) * 3
        depth[::5] = 0.0
        pools.append(dict(rgbs=rgbs, depth=depth, dirs=torch.randn(n, 3, generator=g), T=torch.eye(4).expand(n, 4, 4).clone(),
                          indices=torch.randint(0, 4, (n,), generator=g).to(torch.int32)))
    return pools


def test_ragged_rows_are_each_class_own_epochs_and_the_position_carries(cnr):
    """Rg = 4, lengths 9 / 13 / 22: 2 / 3 / 5 slices per epoch, K = 5 steps per host epoch.  Over three reshuffles the rows class c
    reads are the concatenation of ITS epoch orders, each cut to its slices per epoch; the unread tail is zero; a padding row is
    never named."""
    Rg, lengths, ids, seed = 4, (9, 13, 22), (3, 0, 5), 77
    pool = cnr.raypool.RayPool(make_pools(lengths), "cpu", Rg, seed=seed, class_ids=torch.tensor(ids, dtype=torch.int32))
    assert pool.ragged and pool.rows == 22 and pool.rows_cls == list(lengths) and pool.n_gslices == 5
    assert pool.rgbs.shape == (3, 22, 4) and pool.T.shape == (3, 22, 4, 4) and pool.indices.shape == (3, 22)
    K = 5
    state = torch.zeros(3, dtype=torch.int64)
    read = [[] for _ in lengths]
    for host_epoch in range(3):
        state[0] = 123
        pool.reshuffle(state)
        assert pool.cursor == 0 and int(state[0]) == 0
        assert pool.steps_left() == K
        for c, n in enumerate(lengths):
            read[c].append(pool.perm[c, :K * Rg].clone())
            assert int(pool.perm[c, :K * Rg].max()) < n and int(pool.perm[c].min()) >= 0        # never a padding row
            assert not bool(pool.perm[c, K * Rg:].any())                                        # the unread tail
        pool.advance(K)
        assert pool.due()
    for c, (n, cid) in enumerate(zip(lengths, ids)):
        k_c = -(-n // Rg) - 1
        want = torch.cat([order(seed, e, cid, n)[:k_c * Rg] for e in range(3 * K // k_c + 1)])[:3 * K * Rg]
        assert torch.equal(torch.cat(read[c]), want), c
    assert pool._cls_epoch == [7, 5, 3] and pool._cls_slice == [1, 0, 0]        # 15 slices = 7 x 2 + 1 = 5 x 3 = 3 x 5


def test_steps_left_due_advance_and_reshuffle(cnr):
    Rg, rows = 8, 5 * 8 + 3
    pool = cnr.raypool.RayPool(make_pools((rows, rows)), "cpu", Rg, seed=5, class_ids=torch.tensor([0, 1], dtype=torch.int32))
    state = torch.tensor([99, 4, 6], dtype=torch.int64)
    pool.reshuffle(state)
    assert not pool.ragged and pool._epoch == 1 and state.tolist() == [0, 4, 6]
    assert torch.equal(pool.perm[1], order(5, 0, 1, rows))
    steps = 0
    while not pool.due():
        assert pool.steps_left() == -(-(rows - Rg - pool.cursor) // Rg) > 0
        assert pool.cursor == steps * Rg
        pool.advance(1)
        steps += 1
    assert steps == 5 and pool.steps_left() <= 0 and pool.cursor >= rows - Rg
    pool.reshuffle(state)
    assert pool.cursor == 0 and pool._epoch == 2 and pool.steps_left() == 5
    assert torch.equal(pool.perm[0], order(5, 1, 0, rows))
    pool.advance(4)
    assert pool.cursor == 4 * Rg and pool.steps_left() == 1 and not pool.due()


def test_ray_shards_repeat_every_global_slice_entry(cnr):
    """ray_world = 2: both ranks of a global slice index the tables by their own cursor / R, so every entry stands twice"""
    R, w, rows = 4, 2, 6 * 8 + 5
    pools = make_pools((rows, rows), seed=3)
    one = cnr.raypool.RayPool(pools, "cpu", R * w, seed=9, class_ids=torch.tensor([0, 1], dtype=torch.int32), min_depth=0.1)
    one.reshuffle(torch.zeros(3, dtype=torch.int64))
    for rank in range(w):
        pool = cnr.raypool.RayPool(pools, "cpu", R * w, w, rank, R, seed=9, class_ids=torch.tensor([0, 1], dtype=torch.int32),
                                   min_depth=0.1)
        state = torch.zeros(3, dtype=torch.int64)
        pool.reshuffle(state)
        assert int(state[0]) == rank * R and pool.cursor == 0
        assert pool.n_gslices == 6 and pool.n_slices == 2 * pool.n_gslices
        assert torch.equal(pool.perm, one.perm)
        assert torch.equal(pool.slice_max, one.slice_max.repeat_interleave(2, dim=1))
        assert torch.equal(pool.counts_tab, one.counts_tab.repeat_interleave(2, dim=0))
        assert torch.equal(pool.slice_max[:, 0::2], pool.slice_max[:, 1::2])
    # the table itself, against the pool rows the slices name
    for s in range(6):
        rows_s = one.perm[:, s * 8:(s + 1) * 8].long()
        assert torch.equal(one.slice_max[:, s], torch.stack([pools[c]["depth"][rows_s[c]].max() for c in range(2)]))
        assert float(one.counts_tab[s, 0, 1]) == float((pools[0]["rgbs"][rows_s[0], 3] != 0).sum())


def test_no_tables_and_no_indices(cnr):
    """the exact-fp32 background: one class, global ids 0 .. C-1, nothing but the permutation at an epoch end"""
    pool = cnr.raypool.RayPool(make_pools((40,)), "cpu", 8, seed=2, indices=False, tables=False)
    state = torch.zeros(3, dtype=torch.int64)
    pool.reshuffle(state)
    assert pool.indices is None and pool.slice_max is None and pool.counts_tab is None
    assert torch.equal(pool.perm[0], order(2, 0, 0, 40)) and pool.steps_left() == 4
    with pytest.raises(AssertionError, match="two slices"):
        cnr.raypool.RayPool(make_pools((40, 15)), "cpu", 8, class_ids=torch.tensor([0, 1], dtype=torch.int32))


def test_shard_plan():
    from cnr_amd import parallel
    p = parallel.shard_plan(None, None, 3, 64)
    assert (p.world, p.rank, p.shard, p.ray_world, p.ray_rank, p.Rg) == (1, 0, None, 1, 0, 64)
    assert p.n_cls_global == 3 and p.class_ids == [0, 1, 2] and p.rng_map == (0, 0, 0, 0)
    p = parallel.shard_plan(None, "class", 2, 64, dp_rank=1, dp_world=4)          # class shards default to rank::world
    assert p.n_cls_global == 8 and p.class_ids == [1, 5] and p.rng_map == (1, 4, 64, 0) and (p.ray_world, p.Rg) == (1, 64)
    p = parallel.shard_plan(None, "class", 3, 64, dp_rank=0, dp_world=2, n_cls_global=8, class_ids=[0, 1, 5])
    assert p.class_ids == [0, 1, 5] and p.rng_map == (0, 0, 0, 0)                 # irregular ownership: local indices
    p = parallel.shard_plan(None, None, 2, 64, dp_rank=3, dp_world=4)             # a world without a word on how: ray shards
    assert p.shard == "ray" and (p.ray_world, p.ray_rank, p.Rg) == (4, 3, 256) and p.rng_map == (0, 1, 256, 3 * 64)
    assert p.class_ids == [0, 1] and p.n_cls_global == 2
