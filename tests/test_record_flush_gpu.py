"""GPU: how the 8-wave field kernel (cnr_field_train, cnr_field_bwd_pipe) writes its per-workgroup gradient records.

The record format is pinned by tests/test_tail_reduce_gpu.py; this file pins the WRITER of it: entry i of a workgroup's record is
trunk parameter i, the dB halves sit at TR and TR + 63, the per-object row sums at TR + 126 (only when the launch carries them
in the record), bf16 each; a record is E = 16 128 entries and nothing is written outside the records of the launch.

Every case is ONE step of FusedCategoryTrainer with `bwd_blocks` workgroups per class, its record workspace replaced by a slice of
a larger buffer: a guard of 64 KB in front of the first record and behind the last one, guards and workspace pre-filled with a
bf16 NaN pattern no gradient value can equal (SENTINEL).  one_launch=False takes the stand-alone backward (KR = 0) through
ops.field_bwd, the default the one-launch step body.  Asserted per case:
  1. the guards still hold the sentinel, every entry the format calls written does not, and every entry behind the last 16-byte
     chunk that can hold a written entry still does (unwritten entries inside that span may hold anything: consumers skip them);
  2. the fixed-order fp32 sum of the records read back (`_ordered_sum`, the order test_tail_reduce_gpu documents, restated
     here) EQUALS what the reduction entry point cnr_step_grad returns for that workspace with an all-zero row table (the
     latent-path term is then exactly 0): trunk entries and B, bit for bit.  With one workgroup that is "unpacked record ==
     gradient" entry by entry, so a misplaced or stale 16-byte chunk shows;
     where the record carries the row sums, their sum over the records agrees with the exact fixed-point row sums of the step
     within the bf16 rounding of the addends (2^-9 relative each, bound below);
  3. the step's gradient meets the bars of tests/test_fused_gpu.py::test_fused_backward_vs_emulated_f16 against the torch
     emulation of its own arithmetic (tests/f16_emulation.py): 5e-3 on the whole trunk, 3e-2 on the worst tensor -- a chunk of
     eight wrong entries fails them;
  4. two further launches of the kernel on the same inputs leave identical bytes in every written entry.
"""
import pytest
import torch

from conftest import rel_l2
from f16_emulation import emulated_grads
from test_fullsize_gpu import _Batch, _grad_tensors

pytestmark = pytest.mark.gpu

TR = 13892                                   # trunk parameters = first dB record entry
E = 16128                                    # entries of one record
LATENT_BIASES = (3840, 8736, 4896, 13281)    # biases of the latent-conditioned layers: no record entry is written for them
ROWS_MAX = 15
SENTINEL = 0x7fa5                            # a bf16 NaN: never the rounding of a finite gradient value
GUARD = 64 * 1024 // 2                       # guard entries on either side of the records


@pytest.fixture(scope="module")
def cnr(dev):
    import cnr_amd
    return cnr_amd


def _ordered_sum(x):
    """x (C, nwg, n) fp32 on the CPU -> (C, n), one elementwise fp32 add at a time in the reduction's order: with per =
    ceil(nwg / 4), quarter q covers the records [q per, min(nwg, q per + per)); inside it 32 accumulators a[u] start at +0 and
    take a[u] += record (q per + u + 32 k) for k = 0, 1, ..; then a[u] += a[u + st] for st = 16, 8, 4, 2, 1; the quarters
    combine as t0 += t2, t1 += t3, t0 += t1."""
    C, nwg, n = x.shape
    per = -(-nwg // 4)
    ts = []
    for q in range(4):
        w0, w1 = q * per, min(nwg, q * per + per)
        a = torch.zeros(32, C, n)
        k = 0
        while w0 + 32 * k < w1:
            m = min(32, w1 - (w0 + 32 * k))
            a[:m] = a[:m] + x[:, w0 + 32 * k: w0 + 32 * k + m].transpose(0, 1)
            k += 1
        for st in (16, 8, 4, 2, 1):
            a[:st] = a[:st] + a[st:2 * st]
        ts.append(a[0].clone())
    return (ts[0] + ts[2]) + (ts[1] + ts[3])


def _written(n_obj, rows_in_record):
    m = torch.ones(E, dtype=torch.bool)
    for off in LATENT_BIASES:
        m[off:off + 32] = False
    m[TR + 126 + (n_obj * 128 if rows_in_record else 0):] = False
    return m


# id: (C, n_obj, R, n1, n2, workgroups per class, precise_geometry, one_launch, rows_in_record)
# S = 64: a ray spans two tiles (KR = 2); S = 32: one tile per ray (KR = 1); S = 10: two padded rays per tile (TWO / PAD).
# Row-sum form of the kernel: <= 4 objects WIDE 0, <= 7 WIDE 1, <= 15 WIDE 2; the one-launch step with a whole ray per tile
# group takes more than four objects per class in its per-tile form (WIDE 3: the row sums go to the fixed-point table only, the
# record carries none) -- so WIDE 1 and 2 at S = 64 are reached through the stand-alone backward, and at S = 10 in one launch.
CASES = {
    "w0_1obj_1wg": (1, 1, 64, 8, 56, 1, True, True, True),
    "w0_3obj_3wg": (1, 3, 64, 8, 56, 3, True, True, True),
    "w0_4obj_1wg": (1, 4, 64, 8, 56, 1, True, True, True),
    "w0_4obj_3wg": (1, 4, 64, 8, 56, 3, True, True, True),
    "two_classes_kr1": (2, 3, 64, 4, 28, 2, True, True, True),
    "w1_7obj_s64_standalone": (1, 7, 64, 8, 56, 2, True, False, True),
    "w2_15obj_s64_standalone": (1, 15, 64, 8, 56, 2, True, False, True),
    "7obj_s64_one_launch": (1, 7, 64, 8, 56, 2, True, True, False),
    "15obj_s64_one_launch": (1, 15, 64, 8, 56, 2, True, True, False),
    "w2_15obj_s10_one_launch": (1, 15, 64, 1, 9, 2, True, True, True),
    "w3_40obj_s32": (1, 40, 64, 4, 28, 2, True, True, False),
    "two_pad_s10": (1, 4, 64, 1, 9, 2, True, True, True),
    "plain_f16": (1, 4, 64, 8, 56, 2, False, True, True),
    "kr0_standalone": (1, 4, 64, 8, 56, 2, True, False, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_record_flush(cnr, dev, case):
    C, n_obj, R, n1, n2, blocks, precise, one_launch, rows_in_record = CASES[case]
    _C, L = cnr._C, 32
    torch.manual_seed(1234)
    cfg = cnr.cfg.synthetic_config(device=str(dev), latent_dim=L, n_bins_cam2surface=n1, n_bins=n2)
    gen = torch.Generator().manual_seed(5)
    pools = [cnr.scene_cateogries.synthetic_pool(4 * R, n_obj, gen, "cpu") for _ in range(C)]
    tr = cnr.fused.FusedCategoryTrainer(cfg, C, n_obj, pools, R, dev, seed=2, generator=gen, use_graph=False, bwd_blocks=blocks,
                                        precise_geometry=precise, one_launch=one_launch)
    assert bool(tr._ft_blocks) == one_launch and tr.precise == precise
    tr.step()                                     # allocates the step's buffers
    torch.cuda.synchronize()
    nwg = tr._nwg
    assert nwg == blocks and _C.field_bwd_workspace_bytes(C, blocks) == C * nwg * E * 2

    # ---- the step under test, on a guarded, sentinel-filled workspace
    big = torch.full((GUARD + C * nwg * E + GUARD,), SENTINEL, dtype=torch.int16, device=dev)
    ws = big[GUARD:GUARD + C * nwg * E]
    assert ws.data_ptr() % 16 == 0
    tr.bufs["bwd_ws"] = ws.view(torch.uint8)
    theta0 = tr.theta.clone()
    tr.step()
    torch.cuda.synchronize()
    bd = {k: v for k, v in tr.bufs.items() if torch.is_tensor(v)}
    grad = tr.grad.clone()
    dbias = tr.dbias.clone()
    recs = ws.cpu().view(C, nwg, E)

    # 1. guards, written entries, nothing behind the span
    assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + C * nwg * E:] == SENTINEL).all())
    written = _written(n_obj, rows_in_record)
    assert not bool((recs[:, :, written] == SENTINEL).any()), int((recs[:, :, written] == SENTINEL).sum())
    span = -(-(TR + 126 + (n_obj * 128 if n_obj <= ROWS_MAX else 0)) // 8) * 8
    assert bool((recs[:, :, span:] == SENTINEL).all()), int((recs[:, :, span:] != SENTINEL).sum())

    # 2. ordered sum of the records == the reduction's gradient (all-zero row table), bit for bit
    vals = recs.view(torch.bfloat16).float()
    vals[:, :, ~written] = 0.0
    assert bool(torch.isfinite(vals).all())
    s = _ordered_sum(vals)
    want_trunk = s[:, :TR].clone()
    want_B = (s[:, TR:TR + 63] + s[:, TR + 63:TR + 126]).reshape(C, 21, 3)
    lay = tr.lay
    g_red = torch.full((C, lay.total), 7.0, device=dev)
    zero = torch.zeros(8, C * n_obj, 4, 32, dtype=torch.int64, device=dev)
    _C.call("cnr_step_grad", theta0, g_red, lay.total, lay.B[0], lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], L,
            n_obj, C, bd["zl"], torch.empty(C * n_obj, 4, 32, device=dev), tr._reg, ws.view(torch.uint8), nwg, zero, None)
    gv = lay.views(g_red)
    assert torch.equal(gv["trunk"].cpu(), want_trunk), int((gv["trunk"].cpu() != want_trunk).sum())
    assert torch.equal(gv["B"].cpu(), want_B), int((gv["B"].cpu() != want_B).sum())
    if rows_in_record:
        # every addend is the bf16 rounding (2^-9 relative) of a workgroup's share; the step's row sums are exact fixed point
        rows = vals[:, :, TR + 126:TR + 126 + n_obj * 128]
        got_rows = rows.double().sum(1).reshape(C * n_obj, 4, 32)
        ref_rows = dbias.double().cpu()                          # (as fp32: 2^-24 relative on top)
        bound = 2.0 ** -8 * rows.double().abs().sum(1).reshape(C * n_obj, 4, 32) + 2.0 ** -22 * ref_rows.abs() + 1e-9
        assert bool(((got_rows - ref_rows).abs() <= bound).all()), float(((got_rows - ref_rows).abs() - bound).max())

    # 3. the step's gradient against the emulation of its own arithmetic
    assert float(grad.double().norm()) >= 1e-3             # not a noise batch
    idx = bd["ray_row"].long().cpu() - torch.arange(C)[:, None] * n_obj
    got = _grad_tensors(cnr, tr, grad)
    _, emu = emulated_grads(cnr, _Batch(cnr, tr, theta0, bd, idx, dev), dev, precise=precise, regulariser=n_obj > 1)
    trunk_names = {n + sfx for n, _, _ in cnr.ops.TRUNK_LAYERS for sfx in (".weight", ".bias")}
    errs = {k: rel_l2(got[k], emu[k]) for k in got}
    num = sum(float((got[k] - emu[k]).double().pow(2).sum()) for k in trunk_names)
    den = sum(float(emu[k].double().pow(2).sum()) for k in trunk_names)
    worst = max(errs, key=errs.get)
    print(f"[flush] {case} trunk={(num / den) ** 0.5:.2e} worst={worst} {errs[worst]:.2e}")
    for k, e in errs.items():
        assert e < 3e-2, (k, e)
    assert (num / den) ** 0.5 < 5e-3

    # 4. two launches on the same inputs: identical bytes in every written entry
    o = tr.bufs
    Bc = tr.theta[0, lay.B[0]:lay.B[1]]
    if one_launch:
        args = tr._field_train_args(o, o, Bc, tr.d_state2[tr.parity], 1.0, torch.zeros_like(tr.rows_fix), torch.zeros_like(tr.clamp))
        run = lambda: _C.call_struct("cnr_field_train", **args)
    else:
        kw = dict(device=dev, dtype=torch.float32)
        scratch = (torch.zeros(C, TR, **kw), torch.zeros(C, 21, 3, **kw), torch.zeros_like(tr.dbias))
        run = lambda: cnr.ops.field_bwd(o["pts"], lay.views(tr.theta)["B"].contiguous(), o["packed"], o["brows"], o["ray_row"],
                                        tr.scale, o["dsig"], o["drgb"], tr.grad_scale, *scratch, C, R, n1 + n2, n_obj, blocks,
                                        ws.view(torch.uint8), packed_lo=o["packed_lo"])
    twice = []
    for _ in range(2):
        big.fill_(SENTINEL)
        run()
        torch.cuda.synchronize()
        assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + C * nwg * E:] == SENTINEL).all())
        twice.append(ws.cpu().view(C, nwg, E)[:, :, written].clone())
    assert not bool((twice[0] == SENTINEL).any())
    assert torch.equal(twice[0], twice[1])
