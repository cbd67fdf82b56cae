"""GPU: the fixed-order record reduction of the step's last launch (cnr_step_tail, cnr_step_grad), bit for bit.

The order is part of the contract (steps are bitwise reproducible, cnr_step_grad == cnr_step_tail).  For record entry i
over the nwg records of a class, with per = ceil(nwg / 4):
  * quarter q covers the records [q per, min(nwg, q per + per)); inside it 32 fp32 accumulators a[u] start at +0 and take
    a[u] += record (q per + u + 32 k) for k = 0, 1, ..; then a[u] += a[u + st] for st = 16, 8, 4, 2, 1;
  * the quarters combine as t0 += t2, t1 += t3, t0 += t1;
  * a dB entry is that sum of entry TRUNK + j plus that sum of entry TRUNK + 63 + j; a trunk entry adds the latent path's term.
`_ordered_sum` restates this on the CPU from explicit elementwise fp32 adds (exact IEEE, so independent of the kernel); with
an all-zero fixed-point table the latent-path term is exactly 0 and the gradient's trunk and B entries must EQUAL it.
Entries no launch writes lie in uncleared workspace: NaN patterns there must not change a bit of the result.
With a non-zero table: tail == grad bit for bit, both within 1e-5 of a float64 evaluation, AdamW within 1e-6 of torch's.
"""
import pytest
import torch

from conftest import rel_l2
from record_noise import LATENT_BIASES, ROWS_MAX, TR, written_mask  # noqa: F401  (the record's constants live there)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cnr(dev):
    import cnr_amd
    return cnr_amd


def _ordered_sum(x):
    """x (C, nwg, E) fp32 on the CPU -> (C, E): the kernel's order, one elementwise add at a time."""
    C, nwg, E = x.shape
    per = -(-nwg // 4)
    ts = []
    for q in range(4):
        w0, w1 = q * per, min(nwg, q * per + per)
        a = torch.zeros(32, C, E)
        k = 0
        while w0 + 32 * k < w1:
            n = min(32, w1 - (w0 + 32 * k))
            a[:n] = a[:n] + x[:, w0 + 32 * k: w0 + 32 * k + n].transpose(0, 1)
            k += 1
        for st in (16, 8, 4, 2, 1):
            a[:st] = a[:st] + a[st:2 * st]
        ts.append(a[0].clone())
    t0, t1 = ts[0] + ts[2], ts[1] + ts[3]
    return t0 + t1


def _unwritten(E, n_obj):
    return ~written_mask(E, n_obj)


def _step_grad(_C, theta, lay, L, n_obj, C, zl, ws, nwg, fix, reg, fill):
    grad = torch.full((C, lay.total), fill, device=theta.device)     # every entry must be overwritten
    dbr = torch.empty(C * n_obj, 4, 32, device=theta.device)
    _C.call("cnr_step_grad", theta, grad, lay.total, lay.B[0], lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], L,
            n_obj, C, zl, dbr, reg, ws, nwg, fix, None)
    return grad, dbr


def _step_tail(_C, theta, lay, L, n_obj, C, zl, ws, nwg, fix, reg, fill):
    dev = theta.device
    th2 = torch.stack([theta, theta.clone()])
    grad = torch.full((C, lay.total), fill, device=dev)
    m, vv = torch.zeros_like(theta), torch.zeros_like(theta)
    state = torch.zeros(2, 3, device=dev, dtype=torch.int64)
    R = 64
    rl_ws = torch.zeros(_C.render_loss_workspace_bytes(C, R), device=dev, dtype=torch.uint8)
    losses, flags = torch.zeros(3, C, device=dev), torch.zeros(C, device=dev, dtype=torch.int32)
    _C.call_struct("cnr_step_tail", theta_in=th2[0], theta_out=th2[1], grad=grad, exp_avg=m, exp_avg_sq=vv,
                   class_stride=lay.total, off_B=lay.B[0], off_latW=lay.latW[0], off_latb=lay.latb[0], off_shape=lay.shape[0],
                   off_tex=lay.tex[0], L=L, n_obj=n_obj, C=C, zl=zl, dbiasrows=torch.empty(C * n_obj, 4, 32, device=dev),
                   reg_scale=reg, do_latent=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.013,
                   state_cur=state[0], state_next=state[1], add_rows=R, rl_workspace=rl_ws, losses=losses, flags=flags,
                   depth=None, pool_rows=8 * R, perm=None, next_max_bound=None, R=R, records=ws, nwg=nwg, rows_fix=fix,
                   rl_blocks=0, clamp_flags=None, n_obj_cls=None, code_lr=0.0, code_weight_decay=0.0)
    return grad, th2[1]


# (1, 4, 32, 1) one record; (.., 3) an empty quarter; (2, 3, 32, 37) and (2, 15, 32, 50) two classes, ragged quarters;
# (.., 129) per = 33: one full chunk and a rest of one; (1, 4, 256, 256) the benchmarked count; (1, 7, 64, 260) per = 65: the
# loop beyond one round of loads; (1, 20, 32, 37) and (2, 100, 32, 130) more than 15 objects: the record carries no row sums (the
# one-object-per-tile form), so that whole region is unwritten
SHAPES = [(1, 4, 32, 1), (1, 4, 32, 3), (2, 3, 32, 37), (1, 4, 32, 129), (1, 4, 256, 256), (1, 7, 64, 260), (2, 15, 32, 50),
          (1, 20, 32, 37), (2, 100, 32, 130)]


@pytest.mark.parametrize("C,n_obj,L,nwg", SHAPES)
def test_record_reduction_bits(cnr, dev, C, n_obj, L, nwg):
    _C = cnr._C
    gen = torch.Generator().manual_seed(1000 + nwg)
    theta, lay = cnr.fused.init_params(C, L, n_obj, gen, dev)
    zl, br = torch.empty(C * n_obj, 4, 32, device=dev), torch.empty(C * n_obj, 4, 32, device=dev)
    _C.call("cnr_latent_fwd", theta, lay.total, lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], L, n_obj, C, zl, br)
    E = _C.field_bwd_workspace_bytes(1, 1) // 2                      # entries of one record (bf16 each)
    assert _C.field_bwd_workspace_bytes(C, nwg) // 2 == C * nwg * E
    # magnitudes spread over a few binades, so that the order of the adds shows in the last bits
    recs = (torch.randn(C, nwg, E, generator=gen) * torch.exp2(4 * torch.rand(C, nwg, E, generator=gen)) * 1e-2).to(torch.bfloat16)
    unwritten = _unwritten(E, n_obj)
    clean = recs.clone()
    clean[:, :, unwritten] = 0
    dirty = recs.view(torch.int16).clone()                           # bf16 NaN patterns, both signs, quiet and signalling
    nan = torch.tensor([0x7fc0, -1, 0x7f81, -0x7f], dtype=torch.int16)[torch.arange(int(unwritten.sum())) % 4]
    dirty[:, :, unwritten] = nan
    dirty = dirty.view(torch.bfloat16)
    assert bool(torch.isnan(dirty[:, :, unwritten].float()).all()) and not bool(torch.isnan(dirty[:, :, ~unwritten].float()).any())
    ws_clean, ws_dirty = clean.reshape(-1).to(dev), dirty.reshape(-1).to(dev)
    reg = 0.0005

    # ---- all-zero table: the latent-path term is exactly 0, trunk and B are the ordered sums alone
    s = _ordered_sum(clean.float())                                  # (C, E)
    want_trunk = s[:, :TR].clone()
    for off in LATENT_BIASES:
        want_trunk[:, off:off + 32] = 0.0                            # what the latent path alone leaves there: 0
    want_B = (s[:, TR:TR + 63] + s[:, TR + 63:TR + 126]).reshape(C, 21, 3)
    zero = torch.zeros(8, C * n_obj, 4, 32, dtype=torch.int64, device=dev)
    for ws in (ws_dirty, ws_clean):
        for fn in (_step_grad, _step_tail):
            g = lay.views(fn(_C, theta, lay, L, n_obj, C, zl, ws, nwg, zero, reg, 7.0)[0])
            assert torch.equal(g["trunk"].cpu(), want_trunk), (fn.__name__, int((g["trunk"].cpu() != want_trunk).sum()))
            assert torch.equal(g["B"].cpu(), want_B), (fn.__name__, int((g["B"].cpu() != want_B).sum()))

    # ---- non-zero table (eight addends per entry, 2^-40 fixed point)
    rows = torch.randn(C * n_obj, 4, 32, generator=gen, dtype=torch.float64) * 0.3
    parts = torch.rand(8, *rows.shape, generator=gen, dtype=torch.float64)
    parts = parts / parts.sum(0, keepdim=True) * rows
    fix = torch.round(parts * 2.0 ** 40).to(torch.int64).to(dev).contiguous()
    rows_q = fix.sum(0).double() * 2.0 ** -40                        # what the table holds exactly
    grad, dbr_out = _step_grad(_C, theta, lay, L, n_obj, C, zl, ws_dirty, nwg, fix, reg, 7.0)
    grad_clean, _ = _step_grad(_C, theta, lay, L, n_obj, C, zl, ws_clean, nwg, fix, reg, 5.0)
    assert torch.equal(grad, grad_clean)                             # garbage in unwritten entries changes nothing
    assert rel_l2(dbr_out, rows_q) < 1e-6
    th = theta.clone().double().requires_grad_()
    v = lay.views(th)
    zs = []
    for k in range(4):
        code = v["tex"] if k == 3 else v["shape"]
        zs.append(torch.relu(torch.einsum("col,cnl->cno", v["latW"][:, k], code) + v["latb"][:, k][:, None, :]))
    rws = cnr.ops.bias_rows(v["trunk"], torch.stack(zs, dim=2)).reshape(C * n_obj, 4, 32)
    obj = (rws * rows_q).sum()
    if n_obj > 1:
        obj = obj + reg * (torch.norm(v["shape"], dim=-1).sum() + torch.norm(v["tex"], dim=-1).sum())
    obj.backward()
    want = th.grad.clone()
    rs = clean.double().sum(1).to(want.device)
    wv = lay.views(want)
    wv["trunk"] += rs[:, :TR]
    wv["B"] += (rs[:, TR:TR + 63] + rs[:, TR + 63:TR + 126]).reshape(C, 21, 3)
    gv = lay.views(grad)
    for k in ("trunk", "B", "latW", "latb", "shape", "tex"):
        assert rel_l2(gv[k], wv[k]) < 1e-5, (k, rel_l2(gv[k], wv[k]))
    grad2, theta_out = _step_tail(_C, theta, lay, L, n_obj, C, zl, ws_dirty, nwg, fix, reg, 3.0)
    assert torch.equal(grad2, grad)
    p = theta.clone().requires_grad_()
    p.grad = grad.clone()
    torch.optim.AdamW([p], lr=1e-3, weight_decay=0.013).step()
    assert rel_l2(theta_out, p.detach()) < 1e-6


def test_records_must_be_16_byte_aligned(cnr, dev):
    """The reduction loads 16 bytes at a time: a records pointer off by one element is CNR_E_ARG (-1) at both entries,
    before anything is launched."""
    _C = cnr._C
    C, n_obj, L, nwg = 1, 4, 32, 3
    gen = torch.Generator().manual_seed(3)
    theta, lay = cnr.fused.init_params(C, L, n_obj, gen, dev)
    zl = torch.zeros(C * n_obj, 4, 32, device=dev)
    fix = torch.zeros(8, C * n_obj, 4, 32, dtype=torch.int64, device=dev)
    big = torch.zeros(_C.field_bwd_workspace_bytes(C, nwg) // 2 + 8, device=dev, dtype=torch.bfloat16)
    assert big.data_ptr() % 16 == 0
    for fn in (_step_grad, _step_tail):
        with pytest.raises(_C.CnrError, match="code -1"):
            fn(_C, theta, lay, L, n_obj, C, zl, big[1:], nwg, fix, 0.0005, 0.0)
        fn(_C, theta, lay, L, n_obj, C, zl, big[8:], nwg, fix, 0.0005, 0.0)      # 16 bytes on: accepted
    torch.cuda.synchronize()
