"""GPU: the positional-encoding gradient of the one-launch step body (cnr_field_train) where a ray spans tiles (KR > 1).

There the products d e2 = W_vd[e2]^T dPre(viewdir) and d e1 = W_cat[e1]^T dPre(cat) + W_xyz^T dPre(xyz) and the PE backward they
feed -- the whole gradient of the direction matrix B -- are formed by a chain wave's dW partner from the dPre pairs it takes out
of the chain wave's images during the layer steps; only a workgroup's LAST tile is done by the chain wave itself, behind the
loop, from fragments it holds in registers (the record image overwrites them in LDS meanwhile).  The cases choose how the tiles
split between the two paths: tiles = R SP / 32 with SP = 32 KR padded slots per ray, four tiles (one per chain wave) per
workgroup and iteration, iterations = ceil(tiles / (4 workgroups)); every workgroup's last iteration takes the chain-wave path.

Every case is ONE step of FusedCategoryTrainer (use_graph=False, one_launch=True, L = 32) and asserts
  1. it has the iteration count it is meant to have (from tr._nwg, the tile count and the four chain waves);
  2. the gradient norm is >= 1e-3, every tensor is within 3e-2 of the torch emulation of the kernels' own f16 arithmetic
     (tests/f16_emulation.py), B included, and the whole trunk within 5e-3 (the bars of tests/test_record_flush_gpu.py);
  3. two further launches of cnr_field_train on the same inputs leave byte-identical written record entries.
What the cases are sensitive to, by construction: B's gradient has no other source than this PE backward, so without the
behind-the-loop path it is zero in all_last_tiles (every tile is a last tile), and without the cat or the xyz half of d e1 it is
off by O(1) in every case.

Measured with the products still on the chain wave (the parent of the change that moved them), trunk / worst tensor / B:
  all_last_tiles  1.02e-03 / B 1.77e-03 / 1.77e-03
  one_workgroup   1.50e-03 / rgb.0.bias 2.06e-03 / 1.68e-03
  ragged_end      9.59e-04 / encoding_viewdir.0.weight 1.67e-03 / 1.23e-03
  kr4_s128        1.28e-03 / B 2.12e-03 / 2.12e-03
  pad_s40         1.35e-03 / encoding_viewdir.0.bias 4.40e-03 / 1.70e-03
  rowtile_40obj   1.27e-03 / encoding_viewdir.0.bias 1.49e-03 / 1.27e-03
  plain_f16       1.29e-03 / B 1.90e-03 / 1.90e-03
  two_classes     1.11e-03 / rgb.2.weight 2.23e-03 / 1.26e-03
and the records of every case are byte-equal between that build and this one.
"""
import pytest
import torch

from conftest import rel_l2
from f16_emulation import emulated_grads
from test_fullsize_gpu import _Batch, _grad_tensors
from test_record_flush_gpu import E, SENTINEL, _written

pytestmark = pytest.mark.gpu

# id: (C, n_obj, R, n1, n2, workgroups per class, precise_geometry), iterations of a workgroup's loop
CASES = {
    "all_last_tiles": ((1, 4, 16, 8, 56, 8, True), 1),     # 32 tiles, 8 workgroups: every tile takes the behind-the-loop path
    "one_workgroup": ((1, 4, 64, 8, 56, 1, True), 32),     # the partner path does all tiles but 4 of 128
    "ragged_end": ((1, 3, 50, 8, 56, 3, True), 9),         # 100 tiles, step 12: the last iteration has live tiles in one workgroup only
    "kr4_s128": ((1, 4, 16, 16, 112, 2, True), 8),         # a ray spans four tiles
    "pad_s40": ((1, 4, 32, 5, 35, 2, True), 8),            # KR = 2, padded slots
    "rowtile_40obj": ((1, 40, 64, 8, 56, 2, True), 16),    # per-tile row sums (WIDE 3)
    "plain_f16": ((1, 4, 64, 8, 56, 2, False), 16),        # without the precise geometry branch
    "two_classes": ((2, 3, 32, 8, 56, 2, True), 8),
}


@pytest.fixture(scope="module")
def cnr(dev):
    import cnr_amd
    return cnr_amd


def step_records(cnr, dev, case):
    """One step of `case` on a sentinel-filled record workspace -> (trainer, theta before the step, the step's buffers, its
    gradient, the workspace as int16 [C nwg E])."""
    (C, n_obj, R, n1, n2, blocks, precise), iters = CASES[case]
    torch.manual_seed(1234)
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=32, n_bins_cam2surface=n1, n_bins=n2)
    gen = torch.Generator().manual_seed(5)
    pools = [cnr.scene_cateogries.synthetic_pool(4 * R, n_obj, gen, "cpu") for _ in range(C)]
    tr = cnr.fused.FusedCategoryTrainer(cfg, C, n_obj, pools, R, dev, seed=2, generator=gen, use_graph=False, bwd_blocks=blocks,
                                        precise_geometry=precise, one_launch=True)
    assert tr._ft_blocks and tr.precise == precise
    S = n1 + n2
    assert 32 < S <= 128, "a ray that spans tiles"
    sp = 64 if S <= 64 else 128
    tiles, nwg = R * sp // 32, tr._nwg
    assert nwg == blocks and -(-tiles // (4 * nwg)) == iters, (tiles, nwg)
    tr.step()                                     # allocates the step's buffers
    torch.cuda.synchronize()
    ws = torch.full((C * nwg * E,), SENTINEL, dtype=torch.int16, device=dev)
    tr.bufs["bwd_ws"] = ws.view(torch.uint8)
    theta0 = tr.theta.clone()
    tr.step()
    torch.cuda.synchronize()
    bd = {k: v for k, v in tr.bufs.items() if torch.is_tensor(v)}
    return tr, theta0, bd, tr.grad.clone(), ws


@pytest.mark.parametrize("case", list(CASES))
def test_pe_partner(cnr, dev, case):
    (C, n_obj, R, n1, n2, blocks, precise), _ = CASES[case]
    tr, theta0, bd, grad, ws = step_records(cnr, dev, case)
    nwg, lay = tr._nwg, tr.lay
    written = _written(n_obj, n_obj <= 4)        # more than four objects: the per-tile form, no row sums in the record
    assert not bool((ws.cpu().view(C, nwg, E)[:, :, written] == SENTINEL).any())

    # the step's gradient against the emulation of its own arithmetic
    assert float(grad.double().norm()) >= 1e-3             # not a noise batch
    idx = bd["ray_row"].long().cpu() - torch.arange(C)[:, None] * n_obj
    got = _grad_tensors(cnr, tr, grad)
    _, emu = emulated_grads(cnr, _Batch(cnr, tr, theta0, bd, idx, dev), dev, precise=precise, regulariser=n_obj > 1)
    assert "B" in got and float(emu["B"].double().norm()) > 0
    trunk_names = {n + sfx for n, _, _ in cnr.ops.TRUNK_LAYERS for sfx in (".weight", ".bias")}
    errs = {k: rel_l2(got[k], emu[k]) for k in got}
    num = sum(float((got[k] - emu[k]).double().pow(2).sum()) for k in trunk_names)
    den = sum(float(emu[k].double().pow(2).sum()) for k in trunk_names)
    worst = max(errs, key=errs.get)
    print(f"[pe-partner] {case} trunk={(num / den) ** 0.5:.2e} worst={worst} {errs[worst]:.2e} B={errs['B']:.2e}")
    for k, e in errs.items():
        assert e < 3e-2, (k, e)
    assert (num / den) ** 0.5 < 5e-3

    # two launches on the same inputs: identical bytes in every written entry
    o = tr.bufs
    Bc = tr.theta[0, lay.B[0]:lay.B[1]]
    args = tr._field_train_args(o, o, Bc, tr.d_state2[tr.parity], 1.0, torch.zeros_like(tr.rows_fix), torch.zeros_like(tr.clamp))
    again = []
    for _ in range(2):
        ws.fill_(SENTINEL)
        cnr._C.call_struct("cnr_field_train", **args)
        torch.cuda.synchronize()
        again.append(ws.cpu().view(C, nwg, E)[:, :, written].clone())
    assert not bool((again[0] == SENTINEL).any())
    assert torch.equal(again[0], again[1])
