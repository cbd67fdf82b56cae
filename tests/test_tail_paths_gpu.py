"""GPU: every latent and AdamW path of the step's last launch (cnr_step_tail, cnr_step_grad; csrc/tail.hip, csrc/latent_common.h)
against the float64 restatement of tests/tail_cpu.py, path by path and tensor by tensor.

The launch switches on object count and code length (tail_cpu.tail_path: one-trip blocks up to four objects, per-block "local"
blocks from five, the general blocks where the code length does not divide 256, CNR_E_SHAPE beyond 32 objects there), and inside
the paths on further joints: code entries in chunks of 32 objects, table rows in passes beyond 1024, d pre entries in passes
beyond 256, the reducing blocks' latent-path term in rounds of 8 objects, the fixed-point table's per-copy and per-class strides.
tail_cpu.SWEEP puts a case on each side of every joint, up to the 100 objects the reference trains with and the limit of 128.

  * sweep: ONE all-zero record per class, so the trunk gradient is the latent path's term alone and B must come out exactly 0:
    latent weights, biases, both code tables and each of the eight latent-conditioned trunk blocks to 1e-5 (the bar these kernels
    have at up to 15 objects, tests/test_fullsize_gpu.py), every other entry exactly 0, the published float rows to 1e-6,
    cnr_step_tail == cnr_step_grad bit for bit, a second call the same bits;
  * ragged classes (n_obj_cls): padding rows with live, non-zero codes get exactly 0, a one-object class no regulariser; the same
    cases through cnr_latent_bwd;
  * AdamW from a warm state over three steps in the launch's three forms (reduce_block's owner code + AdamSink, adam_one after
    cnr_step_grad, adam_one + latent_trunk_term + the plain latent blocks), parameters and BOTH moments against
    tail_cpu.adamw_reference, with the codes' own group, element by element.

The regulariser scale is 0.02 here (the trainers use 5e-4): at 5e-4 it is 2e-4 of a code gradient of these tables, and a class
that wrongly gets or misses it would move by less than the 1e-3 the ragged cases ask for to tell the two apart.
"""
import numpy as np
import pytest
import torch

import tail_cpu as T
from conftest import rel_l2
from record_noise import TR, written_mask

pytestmark = pytest.mark.gpu

REG = 0.02
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.013)


@pytest.fixture(scope="module")
def cnr(dev):
    import cnr_amd
    assert [tuple(t) for t in cnr_amd.ops._LATENT_TARGETS] == list(T.LATENT_TARGETS)
    return cnr_amd


def _f32(x):
    """the value a float argument has once it has crossed the C ABI"""
    return float(torch.tensor(x, dtype=torch.float32))


def _inputs(cnr, dev, C, n_obj, L, seed, n_real=None):
    """parameters, the latent forward's activations, and a fixed-point table (eight int64 addends per entry at 2^-40) of rows
    0.3 randn, every object its own, padding objects exactly zero"""
    _C = cnr._C
    gen = torch.Generator().manual_seed(seed)
    theta, lay = cnr.fused.init_params(C, L, n_obj, gen, dev)
    zl, br = torch.empty(C * n_obj, 4, 32, device=dev), torch.empty(C * n_obj, 4, 32, device=dev)
    _C.call("cnr_latent_fwd", theta, lay.total, lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], L, n_obj, C, zl, br)
    assert bool((zl == 0).any()) and bool((zl > 0).any())               # the ReLU mask matters
    rows = torch.randn(C, n_obj, 4, 32, generator=gen, dtype=torch.float64) * 0.3
    if n_real is not None:
        for c in range(C):
            rows[c, n_real[c]:] = 0.0
    parts = torch.rand(8, *rows.shape, generator=gen, dtype=torch.float64)
    parts = parts / parts.sum(0, keepdim=True) * rows
    fix = torch.round(parts * 2.0 ** 40).to(torch.int64).reshape(8, C * n_obj, 4, 32).to(dev).contiguous()
    rows_q = fix.sum(0).double().cpu() * 2.0 ** -40                     # what the table holds exactly
    if n_real is not None:
        for c in range(C):
            assert not bool(fix.view(8, C, n_obj, 128)[:, c, n_real[c]:].any())
            if n_real[c] < n_obj:                                       # padding rows keep live codes
                assert float(lay.views(theta)["shape"][c, n_real[c]:].abs().min()) > 0
    cls = None if n_real is None else torch.tensor(n_real, device=dev, dtype=torch.int32)
    return theta, lay, zl, fix, rows_q, cls


def _step_grad(_C, theta, lay, C, zl, ws, nwg, fix, cls, grad, dbr):
    _C.call("cnr_step_grad", theta, grad, lay.total, lay.B[0], lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], lay.L,
            lay.n_obj, C, zl, dbr, REG, ws, nwg, fix, cls)


def _step_tail(_C, theta_in, theta_out, lay, C, zl, ws, nwg, fix, cls, grad, dbr, m, v, state_cur, state_next, do_latent=1,
               code_lr=0.0, code_wd=0.0, R=64):
    dev = theta_in.device
    rl_ws = torch.zeros(_C.render_loss_workspace_bytes(C, R), device=dev, dtype=torch.uint8)
    losses, flags = torch.zeros(3, C, device=dev), torch.zeros(C, device=dev, dtype=torch.int32)
    _C.call_struct("cnr_step_tail", theta_in=theta_in, theta_out=theta_out, grad=grad, exp_avg=m, exp_avg_sq=v,
                   class_stride=lay.total, off_B=lay.B[0], off_latW=lay.latW[0], off_latb=lay.latb[0], off_shape=lay.shape[0],
                   off_tex=lay.tex[0], L=lay.L, n_obj=lay.n_obj, C=C, zl=zl, dbiasrows=dbr, reg_scale=REG, do_latent=do_latent,
                   state_cur=state_cur, state_next=state_next, add_rows=R, rl_workspace=rl_ws, losses=losses, flags=flags,
                   depth=None, pool_rows=8 * R, perm=None, next_max_bound=None, R=R, records=ws, nwg=nwg, rows_fix=fix,
                   rl_blocks=0, clamp_flags=None, n_obj_cls=cls, code_lr=code_lr, code_weight_decay=code_wd, **HYPER)


def _worst(got, want):
    """where the largest difference sits, for the assertion's message"""
    d = (got.detach().double().cpu() - want.detach().double().cpu()).abs()
    at = int(d.reshape(-1).argmax())
    return tuple(int(i) for i in np.unravel_index(at, tuple(d.shape))), float(d.reshape(-1)[at])


def _assert_latent_gradient(tag, grad, want, lay):
    """a gradient that holds the latent path alone: its four tensors and the eight trunk blocks to 1e-5, all else exactly 0"""
    gv, wv = lay.views(grad.cpu()), lay.views(want)
    for k in ("latW", "latb", "shape", "tex"):
        e = rel_l2(gv[k], wv[k])
        assert e < 1e-5, (tag, k, e, _worst(gv[k], wv[k]))
    other = torch.ones(TR, dtype=torch.bool)
    for name, ix in T.latent_trunk_blocks().items():
        e = rel_l2(gv["trunk"][:, ix], wv["trunk"][:, ix])
        assert e < 1e-5, (tag, name, e, _worst(gv["trunk"][:, ix], wv["trunk"][:, ix]))
        other[ix] = False
    assert not bool(gv["trunk"][:, other].any()), (tag, "trunk entries the latent path does not reach", int((gv["trunk"][:, other] != 0).sum()))
    assert not bool(gv["B"].any()), (tag, "B")


def _both_entries(cnr, dev, C, n_obj, L, n_real, seed):
    """cnr_step_grad and cnr_step_tail on one all-zero record per class, each twice -> (gradient, oracle, layout, inputs)"""
    _C = cnr._C
    theta, lay, zl, fix, rows_q, cls = _inputs(cnr, dev, C, n_obj, L, seed, n_real)
    E = _C.field_bwd_workspace_bytes(1, 1) // 2
    ws = torch.zeros(C * E, device=dev, dtype=torch.bfloat16)
    want = T.latent_reference(theta, lay, L, n_obj, C, rows_q, REG, n_real)
    grads = []
    for fill in (7.0, -3.0):                                            # an element nobody writes shows; twice: same bits
        grad, dbr = torch.full((C, lay.total), fill, device=dev), torch.full((C * n_obj, 4, 32), fill, device=dev)
        _step_grad(_C, theta, lay, C, zl, ws, 1, fix, cls, grad, dbr)
        assert rel_l2(dbr, rows_q) < 1e-6, ("cnr_step_grad rows", rel_l2(dbr, rows_q), _worst(dbr.reshape(C, n_obj, 128), rows_q.reshape(C, n_obj, 128)))
        grads.append(grad)
    _assert_latent_gradient("cnr_step_grad", grads[0], want, lay)
    assert torch.equal(grads[0], grads[1])
    for fill in (7.0, -3.0):
        th2 = torch.stack([theta, torch.full_like(theta, fill)])
        grad, dbr = torch.full((C, lay.total), fill, device=dev), torch.full((C * n_obj, 4, 32), fill, device=dev)
        m, v = torch.zeros_like(theta), torch.zeros_like(theta)
        state = torch.zeros(2, 3, device=dev, dtype=torch.int64)
        _step_tail(_C, th2[0], th2[1], lay, C, zl, ws, 1, fix, cls, grad, dbr, m, v, state[0], state[1])
        assert rel_l2(dbr, rows_q) < 1e-6, ("cnr_step_tail rows", rel_l2(dbr, rows_q), _worst(dbr.reshape(C, n_obj, 128), rows_q.reshape(C, n_obj, 128)))
        assert torch.equal(grad, grads[0]), ("cnr_step_tail != cnr_step_grad", int((grad != grads[0]).sum()), _worst(grad, grads[0]))
        assert not bool((th2[1] == fill).any())                         # every parameter was written
        assert torch.equal(th2[0], theta)
    return grads[0], want, lay, (theta, zl, rows_q, cls)


@pytest.mark.parametrize("L,n_obj,C,path", T.SWEEP, ids=[f"L{L}-n{n}-C{C}-{p}" for L, n, C, p in T.SWEEP])
def test_latent_paths_sweep(cnr, dev, L, n_obj, C, path):
    """Every path and joint of the object-count / code-length dispatch (tail_cpu.SWEEP) against the float64 oracle."""
    assert T.tail_path(L, n_obj) == path
    _both_entries(cnr, dev, C, n_obj, L, None, 100 * L + n_obj)


@pytest.mark.parametrize("L,n_obj,C,path", T.REFUSED)
def test_unsupported_shape_is_refused_by_both_entries(cnr, dev, L, n_obj, C, path):
    """More than 32 objects with a code length the per-block form does not take: CNR_E_SHAPE (-2) from both entries, before any
    launch -- no output is touched."""
    _C = cnr._C
    assert T.tail_path(L, n_obj) == path == "refused"
    theta, lay, zl, fix, rows_q, cls = _inputs(cnr, dev, C, n_obj, L, 5)
    E = _C.field_bwd_workspace_bytes(1, 1) // 2
    ws = torch.zeros(C * E, device=dev, dtype=torch.bfloat16)
    grad, dbr = torch.full((C, lay.total), 7.0, device=dev), torch.full((C * n_obj, 4, 32), 7.0, device=dev)
    with pytest.raises(_C.CnrError, match="code -2"):
        _step_grad(_C, theta, lay, C, zl, ws, 1, fix, cls, grad, dbr)
    th2 = torch.stack([theta, torch.full_like(theta, 7.0)])
    m, v = torch.full_like(theta, 7.0), torch.full_like(theta, 7.0)
    state = torch.full((2, 3), 7, device=dev, dtype=torch.int64)
    with pytest.raises(_C.CnrError, match="code -2"):
        _step_tail(_C, th2[0], th2[1], lay, C, zl, ws, 1, fix, cls, grad, dbr, m, v, state[0], state[1])
    torch.cuda.synchronize()
    for t in (grad, dbr, th2[1], m, v, state):
        assert bool((t == 7).all())


@pytest.mark.parametrize("C,n_obj,L,n_real", T.RAGGED, ids=[f"L{L}-n{n}-real{'_'.join(map(str, r))}" for _, n, L, r in T.RAGGED])
def test_ragged_classes(cnr, dev, C, n_obj, L, n_real):
    """n_obj_cls: classes with fewer objects than the layout.  Their padding rows hold random codes, so a regulariser applied
    to them, or to a class with ONE real object, shows.  Both entries as in the sweep, then cnr_latent_bwd on the same inputs."""
    _C = cnr._C
    assert T.tail_path(L, n_obj) == T.RAGGED_PATHS[T.RAGGED.index((C, n_obj, L, n_real))]
    grad, want, lay, (theta, zl, rows_q, cls) = _both_entries(cnr, dev, C, n_obj, L, n_real, 17 * n_obj + L)
    gv, wv = lay.views(grad.cpu()), lay.views(want)
    with_reg = lay.views(T.latent_reference(theta, lay, L, n_obj, C, rows_q, REG, None))
    for c in range(C):
        for k in ("shape", "tex"):
            assert not bool(gv[k][c, n_real[c]:].any()), (c, k, "padding rows")
            if n_real[c] == 1:      # the oracle leaves the regulariser out, and the case can tell: with it the row is another one
                assert rel_l2(with_reg[k][c, 0], wv[k][c, 0]) > 1e-3
                assert rel_l2(gv[k][c, 0], wv[k][c, 0]) < 1e-5 and rel_l2(gv[k][c, 0], with_reg[k][c, 0]) > 1e-3
    # ---- cnr_latent_bwd with n_obj_cls: latent tensors stored, trunk entries ADDED to what the buffer held, B untouched
    assert n_obj <= 64
    g0 = torch.randn(C, lay.total, device=dev)
    g = g0.clone()
    _C.call("cnr_latent_bwd", theta, lay.total, lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], L, n_obj, C, zl,
            rows_q.float().reshape(C * n_obj, 4, 32).to(dev), REG, g, cls)
    g, g0 = g.cpu(), g0.cpu()
    bv, b0 = lay.views(g), lay.views(g0)
    for k in ("latW", "latb", "shape", "tex"):
        assert rel_l2(bv[k], wv[k]) < 1e-5, ("cnr_latent_bwd", k, rel_l2(bv[k], wv[k]), _worst(bv[k], wv[k]))
    added = bv["trunk"] - b0["trunk"]
    other = torch.ones(TR, dtype=torch.bool)
    for name, ix in T.latent_trunk_blocks().items():
        assert rel_l2(added[:, ix], wv["trunk"][:, ix]) < 1e-5, ("cnr_latent_bwd", name)
        other[ix] = False
    assert torch.equal(bv["trunk"][:, other], b0["trunk"][:, other]) and torch.equal(bv["B"], b0["B"])
    for c in range(C):
        assert not bool(bv["shape"][c, n_real[c]:].any()) and not bool(bv["tex"][c, n_real[c]:].any())


def test_latent_bwd_refuses_more_than_64_objects(cnr, dev):
    _C = cnr._C
    C, n_obj, L = 1, 65, 32
    theta, lay = cnr.fused.init_params(C, L, n_obj, torch.Generator().manual_seed(1), dev)
    zl, dbr = torch.zeros(C * n_obj, 4, 32, device=dev), torch.zeros(C * n_obj, 4, 32, device=dev)
    grad = torch.full((C, lay.total), 7.0, device=dev)
    with pytest.raises(_C.CnrError, match="code -2"):
        _C.call("cnr_latent_bwd", theta, lay.total, lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], L, n_obj, C, zl, dbr,
                REG, grad, None)
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all())


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------
ADAM_BOUND_SCALE = 1.0    # the bound below as counted (it would be twice what an fp32 evaluation on the CPU needs, if that
#                           needed more: it needs 0.544 of it, see test_adamw_from_a_warm_state_in_three_forms)


def _adam_bound(want_p, p0, lr_g, wd_g):
    """|theta_out - want| <= 4 * 2^-24 |want| + 8 * 2^-24 |update|, update = want - p (1 - lr wd): the fp32 roundings of the
    expression in csrc/adamw_common.h / tail.hip, counted -- the decayed parameter is one rounded product with a rounded factor
    and the final difference rounds once more (each at most 2^-24 relative to ~|want|); the update passes the roundings of m
    (2), v (3, halved by the root), the root, the scaled denominator (2), the quotient, the step size and its product"""
    update = want_p - p0 * (1.0 - lr_g * wd_g)
    return ADAM_BOUND_SCALE * 2.0 ** -24 * (4 * want_p.abs() + 8 * update.abs())


def test_adamw_from_a_warm_state_in_three_forms(cnr, dev):
    """AdamW of the tail launch from exp_avg = 1e-2 randn, exp_avg_sq = 1e-3 rand and step counter 11, three launches with fresh
    random bf16 records each, parameters and state ping-ponging between their two copies, codes in their own group
    (code_lr = 4e-3, code_weight_decay = 0.05) -- a first step from zero moments is p (1 - lr wd) - lr sign(g) and sees neither
    beta, nor the bias corrections, nor the gradient's size.  Three forms of the same step:
      (i)   cnr_step_tail with records and table: reduce_block's owner code (trunk, B) and AdamSink::latent_set (the rest);
      (ii)  cnr_step_grad, then cnr_step_tail(do_latent = 0, no records, no table) on that gradient: adam_one everywhere --
            what the trainer runs around the all-reduce of a ray-sharded step;
      (iii) cnr_step_tail(do_latent = 1, no records, no table) on a gradient that holds the records' fp32 sums in trunk and B and
            float rows in dbiasrows: adam_one + latent_trunk_term and the plain latent_bwd_block with AdamSink.
    After each launch the gradient the launch left is put through tail_cpu.adamw_reference (float64, the hyper-parameters at the
    fp32 values the kernel receives) from the state the launch started from: parameters, exp_avg and exp_avg_sq to 1e-6, and the
    parameters element by element to _adam_bound.  (i) and (ii) are the same expressions on the same gradient bits: gradient,
    the gradient and exp_avg are asserted EQUAL after the first launch.  exp_avg_sq and the parameters are NOT equal there, and
    why is known: the compiler contracts one of the two products of v b2 + ((1 - b2) g) g into the sum, and it picks the other
    one in adam_one than in reduce_block's owner code and AdamSink::latent_set.  Recomputed on the CPU with exact products,
    EVERY element of (i)'s exp_avg_sq is fl(v b2 + fl(fl((1 - b2) g) g)) and every element of (ii)'s is
    fl(fl((1 - b2) g) g + fl(v b2)) -- the effect csrc/adamw_common.h describes for adam_update.  Measured on MI355X: 8990 of
    the 37 510 elements of exp_avg_sq differ in the last bit, and 19 parameters, all among those 8990 (the root and the
    quotient usually absorb half an ulp of v).  Both are correct roundings of the same expression, so the 1e-6 bars against the
    oracle stay as they are for each form; after the first launch exp_avg_sq is held to ONE last bit between the two (2^-23
    relative), a parameter may differ only where its exp_avg_sq does and by no more than the element bound, and afterwards, when
    the states have parted by those bits, the two are held to 1e-6 of each other.  (iii) sums its latent term in
    another order: 1e-5 of the oracle like the others, no bit equality.
    The element bound is counted, not measured; the same expression evaluated in fp32 on the CPU (tail_cpu.adamw_reference with
    dtype = float32) is printed against it ("[adam]" lines) and stays inside: measured worst |cpu fp32 - want| / bound = 0.544
    over the nine launches, the kernel's 0.557, so the bound stands as counted (ADAM_BOUND_SCALE = 1)."""
    _C = cnr._C
    C, n_obj, L, nwg, n_real, R = 2, 9, 32, 5, (9, 4), 64
    assert T.tail_path(L, n_obj) == "local"
    theta0, lay, _, fix, rows_q, cls = _inputs(cnr, dev, C, n_obj, L, 2024, n_real)
    gen = torch.Generator().manual_seed(99)
    E = _C.field_bwd_workspace_bytes(1, 1) // 2
    assert _C.field_bwd_workspace_bytes(C, nwg) // 2 == C * nwg * E
    recs = [(torch.randn(C, nwg, E, generator=gen) * 1e-2).to(torch.bfloat16) for _ in range(3)]
    mask = written_mask(E, n_obj, rows_in_record=False)
    m0 = (torch.randn(C, lay.total, generator=gen) * 1e-2).to(dev)
    v0 = (torch.rand(C, lay.total, generator=gen) * 1e-3).to(dev)
    lr, wd, code_lr, code_wd = 1e-3, 0.013, 4e-3, 0.05
    hp = dict(lr=_f32(lr), wd=_f32(wd), code_lr=_f32(code_lr), code_wd=_f32(code_wd), b1=_f32(0.9), b2=_f32(0.999), eps=_f32(1e-8))
    code_mask = torch.zeros(C, lay.total, dtype=torch.bool)
    code_mask[:, lay.shape[0]:lay.tex[1]] = True
    assert lay.shape[1] == lay.tex[0] and int(code_mask.sum()) == 2 * C * n_obj * L
    lr_g = torch.where(code_mask, torch.tensor(hp["code_lr"], dtype=torch.float64), torch.tensor(hp["lr"], dtype=torch.float64))
    wd_g = torch.where(code_mask, torch.tensor(hp["code_wd"], dtype=torch.float64), torch.tensor(hp["wd"], dtype=torch.float64))

    def oracle_gradient(theta, rec):
        want = T.latent_reference(theta, lay, L, n_obj, C, rows_q, REG, n_real)
        rs = rec.double()
        rs[:, :, ~mask] = 0.0
        rs = rs.sum(1)
        wv = lay.views(want)
        wv["trunk"] += rs[:, :TR]
        wv["B"] += (rs[:, TR:TR + 63] + rs[:, TR + 63:TR + 126]).reshape(C, 21, 3)
        return want, rs

    bounds = []

    def run(form):
        th2 = torch.stack([theta0, torch.full_like(theta0, 7.0)])
        m, v = m0.clone(), v0.clone()
        state = torch.tensor([[128, 5, 11], [-1, -1, -1]], device=dev, dtype=torch.int64)
        out = []
        for s in range(3):
            par = s & 1
            p_start, m_start, v_start = th2[par].cpu().double(), m.cpu().double(), v.cpu().double()
            cursor, rng, t_prev = state[par].tolist()
            zl, br = torch.empty(C * n_obj, 4, 32, device=dev), torch.empty(C * n_obj, 4, 32, device=dev)
            _C.call("cnr_latent_fwd", th2[par], lay.total, lay.latW[0], lay.latb[0], lay.shape[0], lay.tex[0], L, n_obj, C, zl, br)
            assert bool((zl == 0).any()) and bool((zl > 0).any())
            ws = recs[s].reshape(-1).to(dev)
            want_g, rs = oracle_gradient(th2[par], recs[s])
            grad, dbr = torch.full((C, lay.total), 7.0, device=dev), torch.full((C * n_obj, 4, 32), 7.0, device=dev)
            common = dict(code_lr=code_lr, code_wd=code_wd, R=R)
            if form == "i":
                _step_tail(_C, th2[par], th2[1 - par], lay, C, zl, ws, nwg, fix, cls, grad, dbr, m, v, state[par], state[1 - par], **common)
            elif form == "ii":
                _step_grad(_C, th2[par], lay, C, zl, ws, nwg, fix, cls, grad, dbr)
                _step_tail(_C, th2[par], th2[1 - par], lay, C, zl, None, 0, None, cls, grad, dbr, m, v, state[par], state[1 - par],
                           do_latent=0, **common)
            else:
                gv = lay.views(grad)
                gv["trunk"][:] = rs[:, :TR].float().to(dev)
                gv["B"][:] = (rs[:, TR:TR + 63] + rs[:, TR + 63:TR + 126]).reshape(C, 21, 3).float().to(dev)
                dbr = rows_q.float().reshape(C * n_obj, 4, 32).to(dev)
                _step_tail(_C, th2[par], th2[1 - par], lay, C, zl, None, 0, None, cls, grad, dbr, m, v, state[par], state[1 - par],
                           do_latent=1, **common)
            t = t_prev + 1
            assert state[1 - par].tolist() == [cursor + R, rng + 1, t], (form, s)
            assert torch.equal(th2[par].cpu().double(), p_start)                       # out of place
            # ---- the gradient the launch left, against the oracle
            g = grad.cpu()
            for k in ("trunk", "B", "latW", "latb", "shape", "tex"):
                a, b = lay.views(g)[k], lay.views(want_g)[k]
                assert rel_l2(a, b) < 1e-5, (form, s, k, rel_l2(a, b), _worst(a, b))
            # ---- AdamW on exactly that gradient from the state the launch started from
            want_p, want_m, want_v = T.adamw_reference(p_start, m_start, v_start, g, t, code_mask=code_mask, **hp)
            got_p, got_m, got_v = th2[1 - par].cpu(), m.cpu(), v.cpu()
            for name, a, b in (("theta_out", got_p, want_p), ("exp_avg", got_m, want_m), ("exp_avg_sq", got_v, want_v)):
                assert rel_l2(a, b) < 1e-6, (form, s, name, rel_l2(a, b), _worst(a, b))
            bound = _adam_bound(want_p, p_start, lr_g, wd_g)
            p32 = T.adamw_reference(p_start, m_start, v_start, g, t, code_mask=code_mask, dtype=torch.float32, **hp)[0].double()
            err = (got_p.double() - want_p).abs()
            print(f"[adam] form {form} step {s} t={t}: worst |kernel - want| / bound = {float((err / bound).max()):.3f}, "
                  f"worst |cpu fp32 - want| / bound = {float(((p32 - want_p).abs() / bound).max()):.3f}, "
                  f"kernel == cpu fp32 on {float((got_p.double() == p32).double().mean()):.4f} of the elements")
            assert bool((err <= bound).all()), (form, s, int((err > bound).sum()), _worst(err / bound, torch.zeros_like(err)))
            if s == 0:      # t = 12: a bias correction off by one step is far outside the bound, so the case can see one
                assert t == 12
                for t_wrong in (11, 13):
                    wrong = T.adamw_reference(p_start, m_start, v_start, g, t_wrong, code_mask=code_mask, **hp)[0]
                    # (beyond the element bound on most elements -- measured 0.82 of them, the rest have an update near 0 --
                    #  and beyond the 1e-6 of the whole tensor)
                    assert float(((wrong - want_p).abs() > bound).double().mean()) > 0.5 and rel_l2(wrong, want_p) > 1e-6
            out.append((grad.clone(), th2[1 - par].clone(), m.clone(), v.clone()))
            if form == "i":
                bounds.append(bound)
        return out

    res = {form: run(form) for form in ("i", "ii", "iii")}
    # (i) against (ii) after the first launch, where both started from the same bits (see the docstring)
    (g1, p1, m1, v1), (g2, p2, m2, v2) = res["i"][0], res["ii"][0]
    assert torch.equal(g1, g2), ("(i) != (ii)", "grad", int((g1 != g2).sum()), _worst(g1, g2))
    assert torch.equal(m1, m2), ("(i) != (ii)", "exp_avg", int((m1 != m2).sum()), _worst(m1, m2))
    print(f"[adam] (i) != (ii): exp_avg_sq in {int((v1 != v2).sum())}, theta_out in {int((p1 != p2).sum())} of {v1.numel()} elements")
    a, b = v1.double().cpu(), v2.double().cpu()
    assert bool(((a - b).abs() <= 2.0 ** -23 * b.abs()).all()), ("(i) vs (ii): exp_avg_sq by more than a last bit", _worst(a, b))
    # a parameter differs only where its second moment does, and by no more than the element bound allows either form alone
    assert not bool(((p1 != p2) & (v1 == v2)).any())
    a, b = p1.double().cpu(), p2.double().cpu()
    assert bool(((a - b).abs() <= bounds[0]).all()), ("(i) vs (ii): theta_out", _worst(a, b))
    for s in range(3):
        for name, a, b in zip(("grad", "theta_out", "exp_avg", "exp_avg_sq"), res["i"][s], res["ii"][s]):
            assert rel_l2(a, b) < 1e-6, ("(i) vs (ii)", s, name, rel_l2(a, b))
