"""The fused background step (csrc/bg_fused.hip) restated in float64 from its documented arithmetic: the header comment of
that file and its layout constants O_* (flat parameter vector) and R_* (per-workgroup record).  No kernel is involved;
tests/test_bg_emulation_host.py pins this module itself on the CPU (against oracle.ref_cpu, torch autograd and a float64
sum), tests/test_bg_kernels_gpu.py then holds every kernel, stage by stage, to it.

Every function works on the flat 94403-parameter vector.  `exact=True` switches every f16 / fp32 rounding off (the network in
plain float64, the yardstick the roundings are measured with), as in tests/f16_emulation.py.

Beside a value v the stage functions return T, the same sum of products with absolute values, and n, its number of addends:
an fp32 accumulation of n terms in ANY order with at most one ulp of error per add stays within n 2^-23 T of the exact sum,
so a bound built from (v, T, n) needs no knowledge of the matrix core's internal order.
"""
import math

import torch

H, E1, E2, E1P, EP = 128, 87, 42, 96, 144                    # hidden width, PE widths, E2's column in the (M, 144) image, its width
O_IN_W, O_IN_B, O_M1_W, O_M1_B, O_CAT_W, O_CAT_B = 0, 11136, 11264, 27648, 27776, 55296
O_M2_W, O_M2_B, O_OA_W, O_OA_B, O_CL_W, O_CL_B = 55424, 71808, 71936, 72064, 72065, 93825
O_OC_W, O_OC_B, O_PE_B, NPARAM = 93953, 94337, 94340, 94403
REC, R_OCW, R_OCB, R_OAW, R_OAB, R_PEB = 640, 0, 384, 388, 516, 520
TS = 32                                                        # samples per workgroup tile = per record
F64 = torch.float64
# (parameter index, record entry) of the small parameters, whose gradient the tail takes from the records
SMALL_PARAM = torch.cat([torch.arange(O_OC_W, O_OC_W + 3 * H), torch.arange(O_OC_B, O_OC_B + 3), torch.arange(O_OA_W, O_OA_W + H),
                         torch.tensor([O_OA_B]), torch.arange(O_PE_B, O_PE_B + 63)])
SMALL_SLOT = torch.cat([torch.arange(R_OCW, R_OCW + 3 * H), torch.arange(R_OCB, R_OCB + 3), torch.arange(R_OAW, R_OAW + H),
                        torch.tensor([R_OAB]), torch.arange(R_PEB, R_PEB + 63)])
REC_PAD = sorted(set(range(REC)) - set(SMALL_SLOT.tolist()))   # 387, 517..519, 583..639


def split(theta):
    """flat vector -> {name: (W, b)} and "B" (21, 3), as views (dtype and autograd graph of theta are kept)"""
    lay = dict(in_layer=(O_IN_W, O_IN_B, H, E1), mid1=(O_M1_W, O_M1_B, H, H), cat_layer=(O_CAT_W, O_CAT_B, H, H + E1),
               mid2=(O_M2_W, O_M2_B, H, H), out_alpha=(O_OA_W, O_OA_B, 1, H), color_linear=(O_CL_W, O_CL_B, H, H + E2),
               out_color=(O_OC_W, O_OC_B, 3, H))
    p = {k: (theta[w:w + o * i].view(o, i), theta[b:b + o]) for k, (w, b, o, i) in lay.items()}
    p["B"] = theta[O_PE_B:O_PE_B + 63].view(21, 3)
    return p


def _h(x, exact):
    """an f16 operand: rounded to f16 (exact: left alone), as float64"""
    return x.double() if exact else x.half().double()


def _lin(x, W, b=None):
    """-> (x W^T + b, the same with absolute values)"""
    v, T = x @ W.T, x.abs() @ W.abs().T
    return (v, T) if b is None else (v + b, T + b.abs())


def embed(theta, pts, scale):
    """-> t (M, 3), p (M, 21) = B t, e (M, 129): e[0..2] = t, e[3 + 21 b + d] = sin(pi 2^b p_d); float64, unrounded"""
    t = pts.double().reshape(-1, 3) / scale
    p = t @ split(theta.double())["B"].T
    bands = 2.0 ** torch.arange(6, dtype=F64)
    e = torch.cat([t, torch.sin(math.pi * bands[None, :, None] * p[:, None, :]).reshape(len(t), -1)], 1)
    return t, p, e


def color_layer(theta, a4, e2, exact=False):
    """a5 = relu(f16(W_cl) [a4 | e2] + b) from the f16 arrays the kernel stored -> (a5, T, n)"""
    W, b = split(theta.double())["color_linear"]
    v, T = _lin(torch.cat([a4.double(), e2.double()], 1), _h(W, exact), b)
    return torch.relu(v), T, H + E2 + 1


def out_color(theta, a5, exact=False):
    """the colour logit f16(W_oc) a5 + b -> (logit, T, n)"""
    W, b = split(theta.double())["out_color"]
    v, T = _lin(a5.double(), _h(W, exact), b)
    return v, T, H + 1


def forward(theta, pts, scale, exact=False):
    """-> dict: e, pre1..pre5, a1..a5, sigma (the x10 head), logit, rgb.  The geometry branch is unrounded (the kernel's
    three-product scheme approximates the full fp32 product); the colour branch multiplies f16 operands."""
    p = split(theta.double())
    t, proj, e = embed(theta, pts, scale)
    e1, e2 = e[:, :E1], e[:, E1:]
    o = dict(e=e, t=t, p=proj)
    o["pre1"] = _lin(e1, *p["in_layer"])[0]
    o["a1"] = torch.relu(o["pre1"])
    o["pre2"] = _lin(o["a1"], *p["mid1"])[0]
    o["a2"] = torch.relu(o["pre2"])
    o["pre3"] = _lin(torch.cat([o["a2"], e1], 1), *p["cat_layer"])[0]
    o["a3"] = torch.relu(o["pre3"])
    o["pre4"] = _lin(o["a3"], *p["mid2"])[0]
    o["a4"] = torch.relu(o["pre4"])
    o["sigma"] = 10.0 * _lin(o["a4"], *p["out_alpha"])[0][:, 0]
    o["a5"] = color_layer(theta, _h(o["a4"], exact), _h(e2, exact), exact)[0]
    o["logit"] = out_color(theta, _h(o["a5"], exact), exact)[0]
    o["rgb"] = torch.sigmoid(o["logit"])
    return o


def upstream(rgb, d_sigma, d_rgb, exact=False):
    """-> oc = f16(fp32(d_rgb rgb (1 - rgb))) in the kernel's fp32 steps, dsg = 10 clamp(d_sigma, +-8192) in fp32; float64"""
    if exact:
        return d_rgb.double() * rgb.double() * (1 - rgb.double()), 10.0 * d_sigma.double().clamp(-8192, 8192)
    d, r = d_rgb.float(), rgb.float()
    return ((d * r) * (1.0 - r)).half().double(), (d_sigma.float().clamp(-8192.0, 8192.0) * 10.0).double()


def backward_chain(theta, act, rgb, d_sigma, d_rgb, dpre=None, exact=False):
    """The data-gradient chain, stage by stage.  act: the five (M, 128) activation arrays (mask = act > 0); dpre: the five arrays
    the kernel wrote -- stage l then reads the KERNEL's dpre[l + 1] as its input (None: this function's own, rounded to f16).
    -> dict: oc, dsg, v[l] / T[l] / n[l] for dPre_{l+1} (l = 4 .. 0, unrounded float64 values), de1 (M, 87), de2 (M, 42) with
    T_de1, T_de2, n_de1, n_de2."""
    p = {k: (_h(w[0], exact), w[1]) if k != "B" else w for k, w in split(theta.double()).items()}
    w_alpha = split(theta.double())["out_alpha"][0][0]           # fp32 in the kernel, from theta
    a = [x.double() for x in act]
    oc, dsg = upstream(rgb, d_sigma, d_rgb, exact)
    v, T, n = [None] * 5, [None] * 5, [H, H, H, H + 1, 3]

    def masked(l, val, Tv):
        m = a[l] > 0
        v[l], T[l] = torch.where(m, val, torch.zeros_like(val)), torch.where(m, Tv, torch.zeros_like(Tv))
        return _h(v[l], exact) if dpre is None else dpre[l].double()

    def tr(D, W):                                                # d input = D W, with absolute values
        return D @ W, D.abs() @ W.abs()
    d5 = masked(4, *tr(oc, p["out_color"][0]))
    x, Tx = tr(d5, p["color_linear"][0][:, :H])
    d4 = masked(3, x + w_alpha * dsg[:, None], Tx + (w_alpha * dsg[:, None]).abs())
    d3 = masked(2, *tr(d4, p["mid2"][0]))
    d2 = masked(1, *tr(d3, p["cat_layer"][0][:, :H]))
    d1 = masked(0, *tr(d2, p["mid1"][0]))
    de2, T2 = tr(d5, p["color_linear"][0][:, H:])
    x3, T3 = tr(d3, p["cat_layer"][0][:, H:])
    x1, T1 = tr(d1, p["in_layer"][0])
    return dict(oc=oc, dsg=dsg, v=v, T=T, n=n, de1=x3 + x1, T_de1=T3 + T1, n_de1=2 * H, de2=de2, T_de2=T2, n_de2=H)


def tiles(M):
    """the [lo, hi) sample rows of every workgroup tile / record"""
    return [(lo, min(lo + TS, M)) for lo in range(0, M, TS)]


def records(theta, pts, scale, a4, a5, ch):
    """Per 32-sample tile the record the backward writes, from the chain `ch` (backward_chain's result) and the f16 activations:
    dW / db of out_color (oc, a5), dW / db of out_alpha (dsg, a4), dB[d][k] = sum_s sum_b de[3 + 21 b + d] cos(pi 2^b p_d) pi 2^b t_k.
    -> (rec, T, S) of shape (tiles, 640), float64: T the sums with absolute values (through de's own T), S = sum |de| pi 2^b |t|
    (what an error of the cosine multiplies; dB entries only).  Padding entries are 0."""
    t, p, _ = embed(theta, pts, scale)
    M = len(t)
    a4, a5, oc, dsg = a4.double(), a5.double(), ch["oc"], ch["dsg"]
    bands = 2.0 ** torch.arange(6, dtype=F64)
    cosw = torch.cos(math.pi * bands[None, :, None] * p[:, None, :])                  # (M, 6, 21)
    amp = (math.pi * bands)[None, :, None]
    de = torch.cat([ch["de1"], ch["de2"]], 1)[:, 3:].reshape(M, 6, 21)
    Tde = torch.cat([ch["T_de1"], ch["T_de2"]], 1)[:, 3:].reshape(M, 6, 21)
    gp, Tgp, Sgp = (de * cosw * amp).sum(1), (Tde * cosw.abs() * amp).sum(1), (de.abs() * amp).sum(1)    # (M, 21)
    tl = tiles(M)
    rec, T, S = (torch.zeros(len(tl), REC, dtype=F64) for _ in range(3))
    for k, (lo, hi) in enumerate(tl):
        s = slice(lo, hi)
        rec[k, R_OCW:R_OCW + 3 * H] = (oc[s].T @ a5[s]).reshape(-1)
        T[k, R_OCW:R_OCW + 3 * H] = (oc[s].abs().T @ a5[s].abs()).reshape(-1)
        rec[k, R_OCB:R_OCB + 3], T[k, R_OCB:R_OCB + 3] = oc[s].sum(0), oc[s].abs().sum(0)
        rec[k, R_OAW:R_OAW + H], T[k, R_OAW:R_OAW + H] = dsg[s] @ a4[s], dsg[s].abs() @ a4[s].abs()
        rec[k, R_OAB], T[k, R_OAB] = dsg[s].sum(), dsg[s].abs().sum()
        rec[k, R_PEB:R_PEB + 63] = (gp[s].T @ t[s]).reshape(-1)
        T[k, R_PEB:R_PEB + 63] = (Tgp[s].T @ t[s].abs()).reshape(-1)
        S[k, R_PEB:R_PEB + 63] = (Sgp[s].T @ t[s].abs()).reshape(-1)
    return rec, T, S


def dw_inputs(act, eimg):
    """the input rows X of the five 128-wide layers (in_layer, mid1, cat_layer, mid2, color_linear), as cnr_bg_dw reads them"""
    e1, e2 = eimg[:, :E1], eimg[:, E1P:E1P + E2]
    return [e1, act[0], torch.cat([act[1], e1], 1), act[2], torch.cat([act[3], e2], 1)]


BIG = ((O_IN_W, O_IN_B), (O_M1_W, O_M1_B), (O_CAT_W, O_CAT_B), (O_M2_W, O_M2_B), (O_CL_W, O_CL_B))


def dw_partial(act, dpre, eimg, lo, hi):
    """float64 dW = dPre^T X and db = column sums over the sample rows [lo, hi) of the five big layers, in the flat layout
    -> (value, T), both (94403,) with zeros at the parameters cnr_bg_dw does not own"""
    val, T = torch.zeros(NPARAM, dtype=F64), torch.zeros(NPARAM, dtype=F64)
    for l, (x, (ow, ob)) in enumerate(zip(dw_inputs(act, eimg), BIG)):
        d, x = dpre[l][lo:hi].double(), x[lo:hi].double()
        k = x.shape[1]
        val[ow:ow + H * k], T[ow:ow + H * k] = (d.T @ x).reshape(-1), (d.abs().T @ x.abs()).reshape(-1)
        val[ob:ob + H], T[ob:ob + H] = d.sum(0), d.abs().sum(0)
    return val, T


def _acc8(x):
    """x (n, E) fp32 -> (E,): eight accumulators take rows c .. c + 7 per round, the rest goes into accumulator 0, then a
    pairwise tree -- elementwise fp32 adds, one at a time"""
    sv = torch.zeros(8, x.shape[1], dtype=torch.float32)
    c = 0
    while c + 8 <= len(x):
        sv = sv + x[c:c + 8]
        c += 8
    for r in range(c, len(x)):
        sv[0] = sv[0] + x[r]
    return ((sv[0] + sv[1]) + (sv[2] + sv[3])) + ((sv[4] + sv[5]) + (sv[6] + sv[7]))


def ordered_sums(partials, recs, gscale):
    """bg_tail_kernel's gradient: partials (chunks, 94403) for the big layers, records (nrec, 640) for the small parameters, in
    the kernel's order of fp32 adds, times 1 / gscale -> (94403,) fp32"""
    partials, recs = partials.float().cpu(), recs.float().cpu()
    grad = _acc8(partials)
    nrec = len(recs)
    per = -(-nrec // 16)
    t = torch.zeros(REC, dtype=torch.float32)
    for q in range(16):
        r0, r1 = q * per, min(nrec, q * per + per)
        t = t + _acc8(recs[r0:max(r0, r1)])
    grad[SMALL_PARAM] = t[SMALL_SLOT]
    return grad * torch.tensor(1.0 / gscale, dtype=torch.float32)


def adamw_reference(theta, grad, m, v, t, lr, b1, b2, eps, wd):
    """torch.optim.AdamW's step number t from the moments (m, v) of step t - 1 -> (theta, m, v); float64"""
    p = theta.detach().double().clone().requires_grad_()
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p.grad = torch.zeros_like(p)
    opt.step()                                                   # creates the state
    with torch.no_grad():
        p.copy_(theta.double())
    st = opt.state[p]
    st["step"] = torch.tensor(float(t - 1)) if torch.is_tensor(st["step"]) else t - 1
    st["exp_avg"].copy_(m.double())
    st["exp_avg_sq"].copy_(v.double())
    p.grad = grad.detach().double().clone()
    opt.step()
    return p.detach(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def ulp16(v):
    """spacing of f16 at |v| (float64): 2^(floor(log2 |v|) - 10), at least the subnormal spacing 2^-24"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -30)))
    return torch.exp2((e - 10).clamp_min(-24.0))
