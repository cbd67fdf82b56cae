"""Case builders and the two oracle evaluations for the modular exact-fp32 kernels (tests/test_modular_kernels_gpu.py on
the GPU, tests/test_modular_cases_host.py without one).

A case is the argument tuple of one C-ABI entry point on CPU tensors, output buffers included (pre-filled with NaN where
the kernel overwrites, with PATTERN where it adds).  `oracle(name, dtype, *args)` runs tests/cpu_double.py's
restatement of that entry point on copies cast to `dtype`: float64 is the truth, float32 the yardstick (the same oracle
in the reference's own precision).  Every floating input is DRAWN in float32 and upcast, so the kernel and both
evaluations see identical values; integer and mask inputs come from integer draws or comparisons of float32 draws."""
import math

import numpy as np
import torch

from cpu_double import Double, E, E1, TRUNK, _trunk_preacts, _unpack
from oracle import ref_cpu as O

F32 = torch.float32
FACTOR, FLOOR = 5.0, 2.0 ** -22      # within 5x of the fp32 oracle's own error; four half-ulps of the largest value
TIE_MARGIN = 1e-4                    # no ReLU pre-activation of an mlp case is closer to zero than this (in fp64)
TRUNK_SIZE = sum(o * i + o for _, o, i in TRUNK)

# index of every output buffer in the argument tuple of each entry point
OUTPUTS = {
    "cnr_pe_fwd": {"e": 2},
    "cnr_pe_bwd": {"dB": 3, "dx": 4},
    "cnr_mlp_fwd_f32": {"sig": 3, "rgb": 4},
    "cnr_mlp_bwd_f32": {"de": 5, "dzlat": 6, "dtrunk": 7},
    "cnr_composite_fwd": {"term": 3, "depth": 4, "var": 5, "rgb": 6, "opacity": 7},
    "cnr_composite_bwd": {"d_alpha": 7, "d_color": 8},
    "cnr_loss_fwd_bwd": {"losses": 11, "flags": 12, "d_depth": 13, "d_rgb": 14, "d_opacity": 15},
}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F32)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32)


def pattern(*shape):
    """the known non-zero pre-fill of the buffers a kernel ADDS to (dB, dzlat, dtrunk): 1/16 .. 13/16"""
    n = int(np.prod(shape))
    return ((torch.arange(n) % 13 + 1).to(F32) * 0.0625).reshape(shape)


# ---- the two oracle evaluations and the comparison rule ---------------------------------------------------------------
def oracle(name, dtype, *args):
    """cpu_double.Double().<name> on CPU copies of `args` (floating tensors cast to `dtype`) under that default dtype.
    -> {output name: tensor} for the outputs that were passed (OUTPUTS[name])."""
    conv = []
    for a in args:
        if torch.is_tensor(a):
            a = a.detach().cpu().clone()
            a = a.to(dtype) if a.is_floating_point() else a
        conv.append(a)
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        getattr(Double(), name)(*conv)
    finally:
        torch.set_default_dtype(old)
    return {k: conv[i] for k, i in OUTPUTS[name].items() if conv[i] is not None}


def outputs_of(name, args):
    return {k: args[i] for k, i in OUTPUTS[name].items() if args[i] is not None}


def check(got, want64, ref32, what, sum_bound=None):
    """e_k = max|got - want64| <= 5 e_r + 2^-22 max|want64| with e_r = max|ref32 - want64|; integer outputs equal.
    sum_bound (a tensor shaped like the output, or None): for a SUMMED output that a kernel read and believed right misses
    under the rule above, the order-independent bound n * 2^-24 * sum|addends| (summation_bound) REPLACES the rule, element by
    element; e_k, e_r and the ratio are printed all the same."""
    got, want64, ref32 = got.detach().cpu(), want64.detach().cpu(), ref32.detach().cpu()
    assert got.shape == want64.shape == ref32.shape, what
    if not got.is_floating_point():
        print(f"{what}: integer output {got.tolist()} want {want64.tolist()}")
        assert np.array_equal(got.numpy(), want64.numpy()) and np.array_equal(ref32.numpy(), want64.numpy()), what
        return None
    assert want64.dtype == torch.float64 and bool(torch.isfinite(want64).all()), what
    assert bool(torch.isfinite(got).all()), f"{what}: the kernel left NaN / inf in {int((~torch.isfinite(got)).sum())} elements"
    e_k = float((got.double() - want64).abs().max())
    e_r = float((ref32.double() - want64).abs().max())
    scale = float(want64.abs().max())
    bound = FACTOR * e_r + FLOOR * scale
    ratio = e_k / e_r if e_r > 0 else (0.0 if e_k == 0 else float("inf"))
    if sum_bound is not None:
        sum_bound = sum_bound.detach().cpu().double()
        assert sum_bound.shape == want64.shape, what
        over = float(((got.double() - want64).abs() / sum_bound).max())
        print(f"{what}: e_k {e_k:.3e} e_r {e_r:.3e} ratio {ratio:.2f} scale {scale:.3e} order-independent bound "
              f"{float(sum_bound.max()):.3e} (e_k / bound {over:.3f}; the plain rule's bound {bound:.3e})")
        assert over <= 1.0, f"{what}: e_k / (n 2^-24 sum|addends|) = {over:.3f}"
        return ratio
    print(f"{what}: e_k {e_k:.3e} e_r {e_r:.3e} ratio {ratio:.2f} scale {scale:.3e} bound {bound:.3e}")
    assert e_k <= bound, f"{what}: e_k {e_k:.3e} > 5 * {e_r:.3e} + 2^-22 * {scale:.3e}"
    return ratio


def summation_bound(addends64, n, dim=-1):
    """n * 2^-24 * sum|addends| along `dim`: what ANY order of n-long fp32 addition chains can lose, addends in fp64"""
    return n * 2.0 ** -24 * addends64.double().abs().sum(dim)


def check_exact(got, want, what):
    """outputs defined to be exactly zero (or exactly the pre-fill)"""
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    print(f"{what}: exact, {got.size} elements")
    assert np.array_equal(got, want), what


def split_trunk(t):
    """(C, TRUNK_SIZE) -> [(layer.weight | layer.bias, (C, n))] in the packed order"""
    out, off = [], 0
    for n, o, i in TRUNK:
        out.append((n + ".weight", t[:, off:off + o * i])); off += o * i
        out.append((n + ".bias", t[:, off:off + o])); off += o
    return out


def unidirs_B(g, C):
    return torch.tensor(O.UNIDIRS, dtype=F32).view(21, 3).repeat(C, 1, 1) + 0.01 * randn(g, C, 21, 3)


# ---- cnr_pe_fwd / cnr_pe_bwd -----------------------------------------------------------------------------------
def pe_inputs(C, N, scale, seed):
    """x in [-scale, scale]^3 (t = x / scale in the unit cube); row N // 2 of every class exactly 0 when N > 1; the LAST
    class of a C > 1 case has its B scaled so that max|p| is about 3 (top band argument 96 pi)."""
    g = gen(seed)
    x = (rand(g, C, N, 3) * 2 - 1) * scale
    if N > 1:
        x[:, N // 2] = 0.0
    B = unidirs_B(g, C)
    if C > 1:
        p = torch.matmul(x[-1] / scale, B[-1].t()).abs().max()
        B[-1] *= (3.0 / p).to(F32)
    return g, x.contiguous(), B.contiguous()


def pe_fwd_case(C, N, scale, seed=11):
    _, x, B = pe_inputs(C, N, scale, seed)
    return ("cnr_pe_fwd", (x, B, nan(C, N, E), C, N, float(scale)))


def pe_bwd_case(C, N, scale, with_dx, seed=12):
    g, x, B = pe_inputs(C, N, scale, seed)
    de = randn(g, C, N, E)
    return ("cnr_pe_bwd", (x, B, de, pattern(C, 21, 3), nan(C, N, 3) if with_dx else None, C, N, float(scale)))


# ---- cnr_mlp_fwd_f32 / cnr_mlp_bwd_f32 ----------------------------------------------------------------------------
MLP_SHAPES = [(1, 1, 1), (2, 7, 37), (1, 3, 100), (2, 300, 1), (1, 5, 64)]
MLP_BWD_SHAPES = MLP_SHAPES + [(1, 2053, 64)]
_mlp_cache = {}


def pack_trunk(p):
    return torch.cat([torch.cat([p[n + ".weight"].flatten(1), p[n + ".bias"]], 1) for n, _, _ in TRUNK], 1).contiguous()


def preacts(dtype, e, zlat, trunk):
    """all ReLU pre-activations of the trunk, evaluated in `dtype`: a list of (C, R, S, width)"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return _trunk_preacts(_unpack(trunk.to(dtype)), e.to(dtype), zlat.to(dtype))
    finally:
        torch.set_default_dtype(old)


def mlp_inputs(C, R, S):
    """-> dict(e, zlat, trunk, pts, B, redrawn).  Weights from the oracle's init, embeddings of points in [-1, 1]^3, zlat >= 0
    (post-ReLU in the product).  Samples with a pre-activation within TIE_MARGIN of zero (fp64) are redrawn, from the
    same seeded generator, until none is left: nothing is excluded from any comparison."""
    key = (C, R, S)
    if key in _mlp_cache:
        return _mlp_cache[key]
    g = gen(1000 * C + 10 * R + S)
    p = O.init_codenerf_params(C, 32, 32, g)
    trunk = pack_trunk({k: v.to(F32) for k, v in p.items()})
    assert trunk.shape == (C, TRUNK_SIZE)
    B = unidirs_B(g, C)
    zlat = torch.relu(randn(g, C, R, 4, 32) * 0.5).contiguous()
    pts = rand(g, C, R, S, 3) * 2 - 1
    redrawn = 0
    for _ in range(64):
        e = O.unidirs_embed(pts, B, 1.0).to(F32).contiguous()
        tie = torch.zeros(C, R, S, dtype=torch.bool)
        for a in preacts(torch.float64, e, zlat, trunk):
            tie |= (a.abs() < TIE_MARGIN).any(-1)
        n = int(tie.sum())
        if n == 0:
            break
        pts[tie] = rand(g, n, 3) * 2 - 1
        redrawn += n
    else:
        raise AssertionError("ReLU ties did not clear")
    _mlp_cache[key] = dict(e=e, zlat=zlat, trunk=trunk, pts=pts, B=B, redrawn=redrawn)
    return _mlp_cache[key]


def mlp_fwd_case(C, R, S):
    m = mlp_inputs(C, R, S)
    return ("cnr_mlp_fwd_f32", (m["e"], m["zlat"], m["trunk"], nan(C, R, S), nan(C, R, S, 3), C, R, S))


def mlp_zero_rays(R):
    return torch.arange(R) % 3 == 1


def mlp_bwd_case(C, R, S, zero_rays=False):
    """zero_rays: dsig = drgb = 0 on the rays mlp_zero_rays(R); their de and dzlat rows get exactly nothing"""
    m = mlp_inputs(C, R, S)
    g = gen(7 + 1000 * C + 10 * R + S)
    dsig, drgb = randn(g, C, R, S), randn(g, C, R, S, 3)
    if zero_rays:
        dsig[:, mlp_zero_rays(R)] = 0.0
        drgb[:, mlp_zero_rays(R)] = 0.0
    return ("cnr_mlp_bwd_f32", (m["e"], m["zlat"], m["trunk"], dsig, drgb, nan(C, R, S, E), pattern(C, R, 4, 32),
                                pattern(C, TRUNK_SIZE), C, R, S))


# ---- cnr_composite_fwd / cnr_composite_bwd ----------------------------------------------------------------------
COMPOSITE_FWD_S = [1, 63, 64, 65, 128, 129, 200, 512, 600]
COMPOSITE_BWD_S = [1, 63, 64, 65, 128, 129, 200, 512]
COMPOSITE_NR = [1, 5, 9]
REGIMES = ["ordinary", "saturated", "empty", "thin"]
SATURATED_AT = [0, 62, 63, 64, 65, -1]
UPSTREAMS = ["all", "d_term", "d_depth", "d_rgb+d_opacity"]


def saturated_index(ray, S):
    """where ray `ray` of a saturated case has its alpha = +30: 0, 62, 63, 64, 65, S - 1 in turn, where they exist"""
    at = sorted({S - 1 if i < 0 else i for i in SATURATED_AT if i < S})
    return at[ray % len(at)]


def composite_inputs(NR, S, in_is_occ, regime, seed=0):
    """-> g, alpha (NR, S), color (NR, S, 3), z (NR, S), each regime in its own tensor.
    ordinary: alpha ~ 3 N(0, 1); saturated: one +30 per ray (saturated_index); empty: -30 throughout; thin:
    alpha ~ -5 + N(0, 1) / 2, occupancies of about 0.007, so that a fifth of the transmittance is still there after 256
    samples and every chunk's carry -- the transmittance forward, the suffix sum backward -- weighs in the result (in the
    other three the transmittance is gone, or nothing is absorbed, long before the first chunk ends).  With in_is_occ the
    kernel gets sigmoid(alpha) rounded to float32, and the ordinary regime holds occupancies of exactly 0 and exactly 1."""
    g = gen(seed + 100000 * in_is_occ + 1000 * NR + S + 7 * REGIMES.index(regime))
    alpha = randn(g, NR, S) * 3
    if regime == "saturated":
        for r in range(NR):
            alpha[r, saturated_index(r, S)] = 30.0
    elif regime == "empty":
        alpha[:] = -30.0
    elif regime == "thin":
        alpha = alpha / 6 - 5.0
    if in_is_occ:
        alpha = torch.sigmoid(alpha)
        if regime == "ordinary":
            for r in range(NR):
                i0 = (3 * r + 1) % S
                i1 = (5 * r + S // 2) % S
                alpha[r, i0] = 0.0
                if S > 1:
                    alpha[r, i1 if i1 != i0 else (i1 + 1) % S] = 1.0
                elif r % 2:
                    alpha[r, 0] = 1.0
    color = rand(g, NR, S, 3)
    z = (rand(g, NR, S).sort(dim=-1).values * 4 + 0.1)
    return g, alpha.contiguous(), color.contiguous(), z.contiguous()


def composite_fwd_case(NR, S, in_is_occ, regime, outputs="all"):
    """outputs: 'all', 'term' (color = z = None, as TerminationFn calls it) or 'no_term'"""
    _, alpha, color, z = composite_inputs(NR, S, in_is_occ, regime)
    if outputs == "term":
        return ("cnr_composite_fwd", (alpha, None, None, nan(NR, S), None, None, None, None, NR, S, in_is_occ))
    term = None if outputs == "no_term" else nan(NR, S)
    return ("cnr_composite_fwd", (alpha, color, z, term, nan(NR), nan(NR), nan(NR, 3), nan(NR), NR, S, in_is_occ))


def composite_depth_bound(args):
    """The order-independent bound of composite_fwd_kernel's `depth`: lane l adds its ceil(S / 64) products term_s z_s
    (s = l, l + 64, ...) one after the other, then wave_sum adds the 64 lanes in 6 steps: n = ceil(S / 64) + 6."""
    alpha, _, z = args[:3]
    NR, S, in_is_occ = args[8:11]
    a = alpha.double().reshape(NR, S)
    occ = a if in_is_occ else torch.sigmoid(a)
    f = 1.0 - occ + 1e-10
    T = torch.cat([torch.ones(NR, 1, dtype=torch.float64), torch.cumprod(f, -1)[:, :-1]], -1)
    return summation_bound(occ * T * z.double().reshape(NR, S), (S + 63) // 64 + 6)


def composite_bwd_case(NR, S, in_is_occ, regime, upstream="all"):
    g, alpha, color, z = composite_inputs(NR, S, in_is_occ, regime, seed=1)
    dd, dr, do, dt = randn(g, NR), randn(g, NR, 3), randn(g, NR), randn(g, NR, S)
    if upstream == "d_term":
        return ("cnr_composite_bwd", (alpha, None, None, None, None, None, dt, nan(NR, S), None, NR, S, in_is_occ))
    if upstream == "d_depth":
        dr, do, dt = None, None, None
    elif upstream == "d_rgb+d_opacity":
        dd, dt = None, None
    else:
        assert upstream == "all"
    return ("cnr_composite_bwd", (alpha, color, z, dd, dr, do, dt, nan(NR, S), nan(NR, S, 3), NR, S, in_is_occ))


def composite_closed_form(alpha, color, z, dd, dr, do, dt, in_is_occ):
    """numpy float64 evaluation of the closed form in csrc/render_common.h's comment on the ray compositor -> d_alpha (NR, S):
    d occ_i = T_i g_i - Suf_i / f_i with g_i = dD z_i + dC.c_i + dO + d_term_i and Suf_i = sum_{k>i} term_k g_k"""
    n = lambda t: None if t is None else t.detach().double().numpy()
    a, c, zz, dd, dr, do, dt = n(alpha), n(color), n(z), n(dd), n(dr), n(do), n(dt)
    occ = a if in_is_occ else 1.0 / (1.0 + np.exp(-a))
    f = 1.0 - occ + 1e-10
    T = np.concatenate([np.ones_like(f[:, :1]), np.cumprod(f, axis=1)[:, :-1]], axis=1)
    term = occ * T
    gsum = np.zeros_like(a)
    if dd is not None: gsum = gsum + dd[:, None] * zz
    if dr is not None: gsum = gsum + (c * dr[:, None, :]).sum(-1)
    if do is not None: gsum = gsum + do[:, None]
    if dt is not None: gsum = gsum + dt
    tg = term * gsum
    incl = np.cumsum(tg[:, ::-1], axis=1)[:, ::-1]
    suf = np.concatenate([incl[:, 1:], np.zeros_like(incl[:, :1])], axis=1)      # k > i, with no cancellation
    docc = T * gsum - suf / f
    return docc if in_is_occ else docc * occ * (1.0 - occ)


# ---- cnr_loss_fwd_bwd -----------------------------------------------------------------------------------------------
LOSS_R = [1, 255, 256, 257, 1000]
LOSS_SCALINGS = [(5.0, 10.0, 0.5), (1.0, 1.0, 1.0)]
MIN_RESIDUAL = 1e-3


def loss_zero_rows(R):
    """rows with an exactly-zero depth / colour / opacity residual, and the rows with var exactly 0"""
    r = torch.arange(R)
    return dict(depth=r % 5 == 0, rgb=r % 5 == 1, opacity=r % 5 == 2, var=r % 4 == 3)


def loss_case(C, R, scalings, variant="ordinary"):
    """variant: 'ordinary'; 'empty_depth' / 'empty_object' / 'empty_surface' (class 1 of C = 3: depth mask all zero with
    objects present; labels all 0; labels all 2); 'explode' (the last class: var = 0, residuals >= 200, so its depth
    loss is >= 1e6 = 10 x the threshold).
    Residuals are either exactly 0 (loss_zero_rows) or of magnitude >= 2e-3 before the float32 rounding of
    rendered = target + residual, i.e. >= MIN_RESIDUAL after it.  Row 0 of every class has label 1 and a set depth bit,
    so no mask is empty unless the variant empties it."""
    g = gen(31 * C + R + int(10 * scalings[0]) + 1000 * len(variant))
    labels = torch.randint(0, 3, (C, R), generator=g).to(torch.uint8)
    dmask = (rand(g, C, R) > 0.2).to(torch.uint8)
    labels[:, 0], dmask[:, 0] = 1, 1
    if variant == "empty_depth":
        dmask[1] = 0
    elif variant == "empty_object":
        labels[1] = 0
    elif variant == "empty_surface":
        labels[1] = 2
    zr = loss_zero_rows(R)
    res = lambda amp, *s: (2e-3 + rand(g, *s) * amp) * (torch.randint(0, 2, s, generator=g).to(F32) * 2 - 1)
    gt_d, gt_c = rand(g, C, R) * 4 + 0.5, rand(g, C, R, 3)
    rd, rc, ro = res(2.0, C, R), res(0.5, C, R, 3), res(0.5, C, R)
    var = rand(g, C, R) * 0.5
    var[:, zr["var"]] = 0.0
    if variant == "explode":
        var[-1] = 0.0
        rd[-1] = rd[-1].sign() * (200.0 + rd[-1].abs())
    rd[:, zr["depth"]] = 0.0
    rc[:, zr["rgb"]] = 0.0
    ro[:, zr["opacity"]] = 0.0
    if variant == "explode":
        rd[-1, 0] = 250.0            # R = 1: the one row is a zero-residual row otherwise
    depth, rgb, opa = gt_d + rd, gt_c + rc, (labels != 0).to(F32) + ro
    cs, os_, gs = scalings
    return ("cnr_loss_fwd_bwd", (depth, var, rgb, opa, gt_d, gt_c, labels, dmask, cs, os_, gs, nan(3, C),
                                 torch.full((C,), -1, dtype=torch.int32), nan(C, R), nan(C, R, 3), nan(C, R), C, R))


def loss_direct(dtype, args):
    """The masked means and their gradients written out directly (csrc/loss.hip's header), WITHOUT the oracle's stop at an
    exploding loss: what the explode case is compared with.  -> dict like oracle()'s."""
    depth, var, rgb, opa, gt_d, gt_c, labels, dmask, cs, os_, gs = args[:11]
    t = lambda x: x.to(dtype)
    mo, ms = labels != 0, labels != 2
    md = (dmask != 0) & mo
    empty = [bool((m.sum(-1) == 0).any()) for m in (md, mo, ms)]
    w = [torch.zeros(labels.shape[0], dtype=dtype) if e else 1.0 / (m.sum(-1).to(dtype) + 1e-10)
         for e, m in zip(empty, (md, mo, ms))]
    info = 1.0 / (torch.sqrt(t(var)) + 1e-4)
    rd, rc, ro = t(depth) - t(gt_d), t(rgb) - t(gt_c), t(opa) - mo.to(dtype)
    ld = (rd.abs() * md * info).sum(-1) * w[0]
    lc = (rc.abs().sum(-1) * mo).sum(-1) * w[1]
    lo = (ro.abs() * ms).sum(-1) * w[2]
    flags = (((ld > 1e5) | (lc > 1e5) | (lo > 1e5)).to(torch.int32)
             | (2 * empty[0] + 4 * empty[1] + 8 * empty[2]))
    return {"losses": torch.stack([ld, lc, lo]), "flags": flags.to(torch.int32),
            "d_depth": gs * torch.sign(rd) * md * info * w[0][:, None],
            "d_rgb": gs * cs * torch.sign(rc) * mo[..., None] * w[1][:, None, None],
            "d_opacity": gs * os_ * torch.sign(ro) * ms * w[2][:, None]}


# ---- cnr_adamw_step -----------------------------------------------------------------------------------------------
ADAMW_N = [1, 257, 2048 * 256 + 300]
f32 = lambda v: float(np.float32(v))
# the hyper-parameters the kernel receives are floats: the restatements get the same float32 values
ADAMW_HYPER = dict(lr=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), weight_decay=f32(0.013))
ADAMW_STEPS = 3


def adamw_case(n, seed=5):
    """-> p0 (n,), grads (3, n): the RAW gradients the kernel reads (the true ones are grads * grad_unscale); some exactly 0"""
    g = gen(seed + n)
    p0 = randn(g, n)
    grads = randn(g, ADAMW_STEPS, n) * 0.1
    grads[:, ::7] = 0.0
    if n > 1:
        grads[1, 1] = 0.0
    return p0, grads


def adamw_fp64(p0, grads, unscale, lr, beta1, beta2, eps, weight_decay):
    """torch.optim.AdamW's step restated in float64: decoupled decay, bias corrections.  -> p, exp_avg, exp_avg_sq"""
    p = p0.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t in range(1, grads.shape[0] + 1):
        gr = grads[t - 1].double() * unscale
        p = p * (1.0 - lr * weight_decay)
        m = beta1 * m + (1.0 - beta1) * gr
        v = beta2 * v + (1.0 - beta2) * gr * gr
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adamw_torch(dtype, p0, grads, unscale, lr, beta1, beta2, eps, weight_decay):
    """torch.optim.AdamW itself on CPU in `dtype` -> p, exp_avg, exp_avg_sq"""
    p = p0.to(dtype).clone().requires_grad_()
    opt = torch.optim.AdamW([p], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, foreach=False)
    for t in range(grads.shape[0]):
        p.grad = grads[t].to(dtype) * unscale
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]
