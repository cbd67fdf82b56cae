"""CPU: tests/bg_emulation.py -- the float64 restatement of the fused background step that tests/test_bg_kernels_gpu.py
holds the kernels to -- pinned on its own, with the f16 roundings switched off (exact=True):

  * forward == oracle.ref_cpu.unidirs_embed + occupancy_map_forward on the weights of bg_r240_s14_h128.npz;
  * backward_chain + records + a plain dPre^T X == torch float64 autograd of that network (objective: sum of x g over the
    outputs), 1e-10 relative per tensor;
  * ordered_sums == a float64 sum to fp32 accuracy, and NOT the bits of a left-to-right fp32 sum on spread magnitudes.
"""
import pytest
import torch

import bg_emulation as E
from conftest import Golden, rel_l2
from oracle import ref_cpu as O

NAMES = ["in_layer.0", "mid1.0.0", "cat_layer.0", "mid2.0.0", "out_alpha", "color_linear.0", "out_color"]


def flat(g, prefix="mlp."):
    return torch.cat([g.t(prefix + n + s).reshape(-1) for n in NAMES for s in (".weight", ".bias")] + [g.t("B").reshape(-1)])


@pytest.fixture(scope="module")
def net():
    g = Golden("bg_r240_s14_h128")
    theta = flat(g)
    assert theta.numel() == E.NPARAM
    M = 75                                                         # two full tiles and a partial one
    return g, theta.double(), g.t("pts").reshape(-1, 3)[:M].double()


def _oracle(theta, pts, scale):
    p = E.split(theta)
    sd = {n + s: p[n.split(".")[0]][k] for n in NAMES for k, s in enumerate((".weight", ".bias"))}
    e = O.unidirs_embed(pts.view(1, -1, 1, 3), p["B"][None], scale)
    alpha, color = O.occupancy_map_forward(sd, e)
    return e.reshape(-1, 129), alpha.reshape(-1), color.reshape(-1, 3)


def test_layout_constants():
    """the offsets are the modules' registration order; the small parameters and the record entries map one to one"""
    g = Golden("bg_r240_s14_h128")
    p = E.split(flat(g))
    for n in NAMES:
        assert torch.equal(p[n.split(".")[0]][0], g.t("mlp." + n + ".weight")) and torch.equal(p[n.split(".")[0]][1], g.t("mlp." + n + ".bias"))
    assert torch.equal(p["B"], g.t("B")[0])
    assert len(E.SMALL_PARAM) == len(E.SMALL_SLOT) == 579 and len(set(E.SMALL_SLOT.tolist())) == 579
    assert E.REC_PAD == [387, 517, 518, 519] + list(range(583, 640))


def test_forward_is_the_oracle_network(net):
    g, theta, pts = net
    f = E.forward(theta, pts, g.scale, exact=True)
    e, alpha, color = _oracle(theta, pts, g.scale)
    assert rel_l2(f["e"], e) < 1e-13 and rel_l2(f["sigma"], alpha) < 1e-12 and rel_l2(f["rgb"], color) < 1e-12
    # the rounded form differs from it by the colour branch's f16 operands only
    r = E.forward(theta, pts, g.scale)
    assert torch.equal(r["sigma"], f["sigma"]) and 0 < rel_l2(r["rgb"], f["rgb"]) < 1e-3


def test_chain_and_records_are_the_autograd_gradient(net):
    g, theta, pts = net
    M = len(pts)
    gen = torch.Generator().manual_seed(5)
    gs, gc = torch.randn(M, generator=gen, dtype=E.F64), torch.randn(M, 3, generator=gen, dtype=E.F64)
    th = theta.clone().requires_grad_()
    _, alpha, color = _oracle(th, pts, g.scale)
    ((alpha * gs).sum() + (color * gc).sum()).backward()
    f = E.forward(theta, pts, g.scale, exact=True)
    act = [f["a%d" % k] for k in range(1, 6)]
    ch = E.backward_chain(theta, act, f["rgb"], gs, gc, exact=True)
    eimg = torch.zeros(M, E.EP, dtype=E.F64)
    eimg[:, :E.E1], eimg[:, E.E1P:E.E1P + E.E2] = f["e"][:, :E.E1], f["e"][:, E.E1:]
    grad = E.dw_partial(act, ch["v"], eimg, 0, M)[0]
    rec, T, S = E.records(theta, pts, g.scale, act[3], act[4], ch)
    assert rec.shape == (3, E.REC) and float(rec[:, E.REC_PAD].abs().max()) == 0
    assert bool((T >= rec.abs() * (1 - 1e-12)).all()) and bool((S[:, E.R_PEB:E.R_PEB + 63] > 0).all())
    grad[E.SMALL_PARAM] = rec.sum(0)[E.SMALL_SLOT]
    p_got, p_want = E.split(grad), E.split(th.grad)
    for name in p_want:
        pairs = [(p_got[name], p_want[name])] if name == "B" else list(zip(p_got[name], p_want[name]))
        for k, (a, b) in enumerate(pairs):                         # k: 0 weight, 1 bias
            assert float(b.abs().max()) > 0, (name, k)
            assert rel_l2(a, b) < 1e-10, (name, k, rel_l2(a, b))


def test_chain_clips_and_masks(net):
    """10 clamp(d sigma, +-8192) in fp32, oc through fp32 then f16; the mask is act > 0: +0 blocks, the smallest subnormal passes"""
    g, theta, pts = net
    rgb = torch.tensor([[0.25, 0.5, 0.75]])
    oc, dsg = E.upstream(rgb, torch.tensor([1e5]), torch.tensor([[1.0, 3.0, 1e-9]]))
    assert dsg.tolist() == [81920.0] and oc[0].tolist() == [0.1875, 0.75, float(torch.tensor(1e-9 * 0.1875).half())]
    assert E.upstream(rgb, torch.tensor([-9000.0]), torch.zeros(1, 3))[1].tolist() == [-81920.0]
    act = [torch.zeros(1, E.H, dtype=torch.float16) for _ in range(5)]
    act[3][0, 7], act[3][0, 9] = 2.0 ** -24, 1.0
    ch = E.backward_chain(theta, act, rgb, torch.tensor([3.0]), torch.ones(1, 3))
    wa = E.split(theta)["out_alpha"][0][0]
    assert float(ch["v"][4].abs().max()) == 0                      # a5 = 0: dPre5 = 0 ...
    assert ch["v"][3][0, 7] == wa[7] * 30.0 and ch["v"][3][0, 9] == wa[9] * 30.0     # ... and dPre4 = w_alpha 10 d sigma where a4 > 0
    assert int((ch["v"][3] != 0).sum()) == 2 and torch.equal(ch["T"][3], ch["v"][3].abs())


def test_ordered_sums_order_and_accuracy():
    gen = torch.Generator().manual_seed(11)
    for chunks, nrec in ((1, 1), (7, 15), (9, 17), (44, 525)):
        spread = lambda *s: torch.randn(*s, generator=gen) * torch.exp2(8 * torch.rand(*s, generator=gen))
        partials, recs = spread(chunks, E.NPARAM), spread(nrec, E.REC)
        got = E.ordered_sums(partials, recs, 256.0)
        want = partials.double().sum(0)
        want[E.SMALL_PARAM] = recs.double().sum(0)[E.SMALL_SLOT]
        T = partials.abs().double().sum(0)
        T[E.SMALL_PARAM] = recs.abs().double().sum(0)[E.SMALL_SLOT]
        n = max(chunks, nrec)
        assert bool(((got.double() * 256.0 - want).abs() <= n * 2.0 ** -24 * T).all())
        naive = torch.zeros(E.NPARAM)
        for c in range(chunks):
            naive = naive + partials[c]
        nr = torch.zeros(E.REC)
        for r in range(nrec):
            nr = nr + recs[r]
        naive[E.SMALL_PARAM] = nr[E.SMALL_SLOT]
        differs = int((naive / 256.0 != got).sum())
        if chunks > 8:
            assert differs > 1000, differs                         # the order shows in the last bits
        else:
            assert differs == 0    # fewer than 8 chunks all go through accumulator 0, up to 16 records one per group: left to right
    # NaN where the tail must not look (record padding, the small parameters' slots of the partials) changes nothing
    dirty_p, dirty_r = partials.clone(), recs.clone()
    dirty_p[:, E.SMALL_PARAM] = float("nan")
    dirty_r[:, E.REC_PAD] = float("nan")
    assert torch.equal(E.ordered_sums(dirty_p, dirty_r, 256.0), got)


def test_adamw_reference_is_torch_adamw_from_step_one():
    gen = torch.Generator().manual_seed(2)
    p0, grads = torch.randn(50, generator=gen, dtype=E.F64), torch.randn(3, 50, generator=gen, dtype=E.F64)
    p = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=0.013)
    th, m, v = p0, torch.zeros(50), torch.zeros(50)
    for t in (1, 2, 3):
        p.grad = grads[t - 1].clone()
        opt.step()
        th, m, v = E.adamw_reference(th, grads[t - 1], m, v, t, 1e-3, 0.9, 0.999, 1e-8, 0.013)
        assert rel_l2(th, p) < 1e-14 and rel_l2(m, opt.state[p]["exp_avg"]) < 1e-14 and rel_l2(v, opt.state[p]["exp_avg_sq"]) < 1e-14
