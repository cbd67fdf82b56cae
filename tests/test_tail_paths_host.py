"""CPU: the float64 restatements of tests/tail_cpu.py, which tests/test_tail_paths_gpu.py holds the step tail's kernels to,
checked on their own: AdamW against torch.optim.AdamW from a warm state, the latent objective with ragged classes against the
same objective written class by class on sliced tensors, and the path label of every shape the GPU cases use."""
import pytest
import torch

import tail_cpu as T


@pytest.fixture(scope="module")
def fused():
    import cnr_amd
    return cnr_amd.fused


def test_adamw_reference_equals_torch_adamw_from_a_warm_state():
    """Two parameter groups (codes with their own rate and decay), float64, five steps from non-zero moments and a step counter
    of 11: parameters and both moments to 1e-12 after every step."""
    gen = torch.Generator().manual_seed(11)
    n, n_code, t0 = 700, 200, 11
    lr, wd, code_lr, code_wd = 1e-3, 0.013, 4e-3, 0.05
    p = torch.randn(n, generator=gen, dtype=torch.float64) * 0.2
    m = torch.randn(n, generator=gen, dtype=torch.float64) * 1e-2
    v = torch.rand(n, generator=gen, dtype=torch.float64) * 1e-3
    code_mask = torch.zeros(n, dtype=torch.bool)
    code_mask[n - n_code:] = True
    a, b = p[:n - n_code].clone().requires_grad_(), p[n - n_code:].clone().requires_grad_()
    opt = torch.optim.AdamW([dict(params=[a], lr=lr, weight_decay=wd), dict(params=[b], lr=code_lr, weight_decay=code_wd)],
                            betas=(0.9, 0.999), eps=1e-8)
    for q, sl in ((a, slice(0, n - n_code)), (b, slice(n - n_code, n))):
        opt.state[q] = dict(step=torch.tensor(float(t0)), exp_avg=m[sl].clone(), exp_avg_sq=v[sl].clone())
    for s in range(5):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * torch.exp2(6 * torch.rand(n, generator=gen, dtype=torch.float64)) * 1e-3
        a.grad, b.grad = g[:n - n_code].clone(), g[n - n_code:].clone()
        opt.step()
        p, m, v = T.adamw_reference(p, m, v, g, t0 + s + 1, lr, wd, code_lr, code_wd, code_mask)
        for got, name in ((p, None), (m, "exp_avg"), (v, "exp_avg_sq")):
            want = torch.cat([a.detach() if name is None else opt.state[a][name], b.detach() if name is None else opt.state[b][name]])
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (s, name)
        assert int(opt.state[a]["step"]) == t0 + s + 1
    # the two groups and the step number are really seen: one group for all, or a step off by one, is far outside 1e-12
    one_group = T.adamw_reference(p, m, v, g, t0 + 6, lr, wd, lr, wd, code_mask)[0]
    off_by_one = T.adamw_reference(p, m, v, g, t0 + 5, lr, wd, code_lr, code_wd, code_mask)[0]
    want = T.adamw_reference(p, m, v, g, t0 + 6, lr, wd, code_lr, code_wd, code_mask)[0]
    assert float((one_group - want)[code_mask].abs().min()) > 1e-6 and torch.equal(one_group[~code_mask], want[~code_mask])
    assert float((off_by_one - want).abs().median()) > 1e-8


def test_adamw_reference_in_fp32_is_the_same_expression():
    """dtype = float32 (what the GPU test uses to size its element bound) stays within a few fp32 roundings of float64"""
    gen = torch.Generator().manual_seed(12)
    n = 4000
    p = torch.randn(n, generator=gen) * 0.2
    m, v = torch.randn(n, generator=gen) * 1e-2, torch.rand(n, generator=gen) * 1e-3
    g = torch.randn(n, generator=gen) * 1e-2
    code_mask = torch.arange(n) % 3 == 0
    hp = [float(torch.tensor(x, dtype=torch.float32)) for x in (1e-3, 0.013, 4e-3, 0.05, 0.9, 0.999, 1e-8)]
    w64 = T.adamw_reference(p, m, v, g, 12, *hp[:4], code_mask, *hp[4:])
    w32 = T.adamw_reference(p, m, v, g, 12, *hp[:4], code_mask, *hp[4:], dtype=torch.float32)
    for a, b in zip(w32, w64):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert float((a.double() - b).norm() / b.norm()) < 2e-7


@pytest.mark.parametrize("C,n_obj,L,n_real", T.RAGGED)
def test_latent_reference_with_ragged_classes_equals_per_class_slicing(fused, C, n_obj, L, n_real):
    """n_real: the objective of class c restated on tensors SLICED to its real objects (matrix products written out, no shared
    helper), one autograd call per class; padding rows get exactly 0, a one-object class no regulariser."""
    gen = torch.Generator().manual_seed(7 * n_obj + L)
    theta, lay = fused.init_params(C, L, n_obj, gen)
    rows = torch.randn(C, n_obj, 4, 32, generator=gen, dtype=torch.float64) * 0.3
    for c in range(C):
        rows[c, n_real[c]:] = 0.0
    reg = 0.02
    got = T.latent_reference(theta, lay, L, n_obj, C, rows, reg, n_real)
    assert got.dtype == torch.float64 and got.shape == (C, lay.total)
    for c in range(C):
        n = n_real[c]
        th = theta[c].double().clone().requires_grad_()
        trunk, latW = th[lay.trunk[0]:lay.trunk[1]], th[lay.latW[0]:lay.latW[1]].view(4, 32, L)
        latb = th[lay.latb[0]:lay.latb[1]].view(4, 32)
        shape, tex = th[lay.shape[0]:lay.shape[1]].view(n_obj, L)[:n], th[lay.tex[0]:lay.tex[1]].view(n_obj, L)[:n]
        obj = 0.0
        for k, (wo, bo, ld) in enumerate(T.LATENT_TARGETS):
            z = torch.clamp((tex if k == 3 else shape) @ latW[k].T + latb[k], min=0.0)          # (n, 32)
            Wt = trunk[wo:wo + 32 * ld].view(32, ld)[:, :32]
            obj = obj + ((z @ Wt.T + trunk[bo:bo + 32]) * rows[c, :n, k]).sum()
        if n > 1:
            obj = obj + reg * (shape.pow(2).sum(-1).sqrt().sum() + tex.pow(2).sum(-1).sqrt().sum())
        obj.backward()
        want = th.grad
        assert float((got[c] - want).abs().max()) <= 1e-12 * float(want.abs().max()), c
        gv = lay.views(got)
        assert not bool(gv["shape"][c, n:].any()) and not bool(gv["tex"][c, n:].any())
    # the latent path reaches the eight blocks of latent_trunk_blocks() and nothing else in the trunk, nothing in B
    other = torch.ones(T.TRUNK, dtype=torch.bool)
    blocks = T.latent_trunk_blocks()
    assert len(blocks) == 8 and sum(ix.numel() for ix in blocks.values()) == 4 * 33 * 32
    for name, ix in blocks.items():
        assert bool(other[ix].all()), name                     # disjoint
        other[ix] = False
        assert float(lay.views(got)["trunk"][:, ix].abs().max()) > 0, name
    assert not bool(lay.views(got)["trunk"][:, other].any()) and not bool(lay.views(got)["B"].any())
    # a regulariser on every row (n_real = None) is visibly another gradient
    full = T.latent_reference(theta, lay, L, n_obj, C, rows, reg, None)
    c1 = [c for c in range(C) if n_real[c] == 1][0] if 1 in n_real else None
    if c1 is not None:
        a, b = lay.views(full)["shape"][c1, 0], lay.views(got)["shape"][c1, 0]
        assert float((a - b).norm() / b.norm()) > 1e-3


def test_latent_targets_are_the_packages(fused):
    from cnr_amd import ops
    assert [tuple(t) for t in ops._LATENT_TARGETS] == list(T.LATENT_TARGETS) and ops.TRUNK_PARAMS == T.TRUNK
    th = torch.randn(2, T.TRUNK, dtype=torch.float64)
    z = torch.rand(2, 5, 4, 32, dtype=torch.float64)
    assert float((T.bias_rows(th, z) - ops.bias_rows(th, z)).abs().max()) < 1e-13


def test_tail_path_labels():
    for L, n_obj, C, path in T.SWEEP + T.REFUSED:
        assert T.tail_path(L, n_obj) == path, (L, n_obj)
    for (C, n_obj, L, n_real), path in zip(T.RAGGED, T.RAGGED_PATHS):
        assert T.tail_path(L, n_obj) == path and len(n_real) == C and max(n_real) == n_obj
    # every path has a case, and the joints of the object loops are each straddled
    assert {p for _, _, _, p in T.SWEEP + T.REFUSED} == {"1trip", "local", "general", "refused"}
    n32 = [n for L, n, _, _ in T.SWEEP if L == 32]
    for lo, hi in ((4, 5), (8, 9), (16, 17), (32, 33), (64, 65)):
        assert any(n <= lo for n in n32) and hi in n32
    # the table in the kernel's words
    assert T.tail_path(32, 4) == "1trip" and T.tail_path(256, 4) == "1trip" and T.tail_path(512, 4) == "general"
    assert T.tail_path(32, 129) == "refused" and T.tail_path(16, 5) == "general" and T.tail_path(16, 33) == "refused"
    assert T.tail_path(48, 32) == "general" and T.tail_path(1024, 128) == "local"
