"""GPU: every modular exact-fp32 kernel (csrc/pe.hip, mlp_f32.hip, composite.hip, loss.hip), entry point by entry point
through _C.call, against tests/cpu_double.py's restatement evaluated in float64 -- at the shapes where these kernels can go
wrong (chunk carries, grid-stride wraps, ragged and dead waves, rays longer than a wave, empty masks).

The rule (modular_cases.check): e_k = max|kernel - fp64| <= 5 * e_r + 2^-22 * max|fp64| for every output tensor, with
e_r = max|fp32 oracle - fp64| the error of the same oracle in the reference's own precision.  Each numerical regime has
its own call, so a hard regime's e_r does not loosen an easy one.  Buffers a kernel must overwrite start as NaN, buffers it
adds to (dB, dzlat, dtrunk) start as a non-zero pattern, and the whole buffer is compared."""
import pytest
import torch

import modular_cases as M

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def _C(dev):
    import cnr_amd
    assert cnr_amd._C.device_info()["gfx950"], "these kernels are built for gfx950 only"
    return cnr_amd._C


def launch(_C, dev, case):
    """one launch of the case's entry point on device copies of its arguments -> {output name: CPU tensor}"""
    name, args = case
    dargs = [a.to(dev, copy=True) if torch.is_tensor(a) else a for a in args]
    _C.call(name, *dargs)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in M.outputs_of(name, dargs).items()}


def compare(_C, dev, case, what, split=None, sum_bounds=None):
    """sum_bounds: {output name: order-independent bound} for the summed outputs that take it (modular_cases.check)"""
    name, args = case
    got = launch(_C, dev, case)
    want, ref = M.oracle(name, F64, *args), M.oracle(name, F32, *args)
    assert set(got) == set(want) == set(ref)
    for k in got:
        if split and k in split:      # report the parts (layers) of a packed buffer one by one, each with its own e_r
            for (part, g), (_, w), (_, r) in zip(split[k](got[k]), split[k](want[k]), split[k](ref[k])):
                M.check(g, w, r, f"{what} {k}[{part}]")
        else:
            M.check(got[k], want[k], ref[k], f"{what} {k}", (sum_bounds or {}).get(k))
    return got, want, ref


# ---- cnr_pe_fwd / cnr_pe_bwd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N", [(1, 1), (3, 255), (2, 257)])
@pytest.mark.parametrize("scale", [1.0, 2.0, 10.0])
def test_pe_fwd(_C, dev, C, N, scale):
    case = M.pe_fwd_case(C, N, scale)
    got, _, _ = compare(_C, dev, case, f"pe_fwd C={C} N={N} scale={scale}")
    if N > 1:
        M.check_exact(got["e"][:, N // 2], torch.zeros(C, M.E), "pe_fwd row of x = 0")


@pytest.mark.parametrize("C,N", [(1, 1), (2, 300), (2, 65536 + 300)])
def test_pe_bwd_dB_alone(_C, dev, C, N):
    """pe_bwd_dir_kernel; 65 836 samples make the 256-block cap wrap the grid-stride loop"""
    compare(_C, dev, M.pe_bwd_case(C, N, 2.0, with_dx=False), f"pe_bwd_dir C={C} N={N}")


@pytest.mark.parametrize("C,N", [(1, 1), (2, 300), (1, 262144 + 77)])
def test_pe_bwd_with_dx(_C, dev, C, N):
    """pe_bwd_kernel; 262 221 samples wrap the 1024-block cap.  dx row by row, the last row included"""
    got, want, ref = compare(_C, dev, M.pe_bwd_case(C, N, 2.0, with_dx=True), f"pe_bwd C={C} N={N}")
    # every row against the oracle's error over the whole buffer and the floor of ITS OWN largest value, not the buffer's
    e_k = (got["dx"].double() - want["dx"]).abs().amax(-1)
    e_r = float((ref["dx"].double() - want["dx"]).abs().max())
    bound = M.FACTOR * e_r + M.FLOOR * want["dx"].abs().amax(-1)
    worst = int((e_k / bound).argmax())
    print(f"pe_bwd C={C} N={N} dx row by row: worst row {worst} of {C * N} at e_k / bound {float((e_k / bound).max()):.3f}; "
          f"last row {float(e_k[-1, -1] / bound[-1, -1]):.3f}")
    assert bool((e_k <= bound).all()), (e_k > bound).nonzero()[:8].tolist()


# ---- cnr_mlp_fwd_f32 / cnr_mlp_bwd_f32 -------------------------------------------------------------------------------
@pytest.mark.parametrize("C,R,S", M.MLP_SHAPES)
def test_mlp_fwd(_C, dev, C, R, S):
    compare(_C, dev, M.mlp_fwd_case(C, R, S), f"mlp_fwd {C}x{R}x{S}")


@pytest.mark.parametrize("C,R,S", M.MLP_BWD_SHAPES)
def test_mlp_bwd(_C, dev, C, R, S):
    compare(_C, dev, M.mlp_bwd_case(C, R, S), f"mlp_bwd {C}x{R}x{S}", split={"dtrunk": M.split_trunk})


@pytest.mark.parametrize("C,R,S", [(2, 7, 37), (1, 3, 100)])
def test_mlp_bwd_rays_without_upstream(_C, dev, C, R, S):
    """dsig = drgb = 0 on a subset of rays: their de rows are exactly 0, their dzlat rows exactly the pre-fill"""
    case = M.mlp_bwd_case(C, R, S, zero_rays=True)
    got, _, _ = compare(_C, dev, case, f"mlp_bwd {C}x{R}x{S} zero rays", split={"dtrunk": M.split_trunk})
    zr = M.mlp_zero_rays(R)
    M.check_exact(got["de"][:, zr], torch.zeros(C, int(zr.sum()), S, M.E), "de rows of rays without upstream")
    M.check_exact(got["dzlat"][:, zr], M.pattern(C, R, 4, 32)[:, zr], "dzlat rows of rays without upstream")


# ---- cnr_composite_fwd / cnr_composite_bwd -----------------------------------------------------------------------
@pytest.mark.parametrize("regime", M.REGIMES)
@pytest.mark.parametrize("in_is_occ", [0, 1])
@pytest.mark.parametrize("NR", M.COMPOSITE_NR)
@pytest.mark.parametrize("S", M.COMPOSITE_FWD_S)
def test_composite_fwd(_C, dev, S, NR, in_is_occ, regime):
    """The thin regime is the one in which the transmittance carried from chunk to chunk weighs in every output.
    Its `depth` at S = 600 -- ten products of like size per lane, then the wave -- takes the order-independent bound
    n 2^-24 sum|term z|, n = ceil(600 / 64) + 6 = 16 read off the kernel, in place of the rule: under the rule the lone ray
    with in_is_occ = 1 missed (e_k 2.981e-07 = 2.5 ulp, bound 2.201e-07) against an fp32 oracle that happened to be exact
    (e_r 5.822e-11).  Every other output, shape and regime stays under the rule, `term` (elementwise) included."""
    case = M.composite_fwd_case(NR, S, in_is_occ, regime)
    sum_bounds = {"depth": M.composite_depth_bound(case[1])} if (regime, S) == ("thin", 600) else None
    compare(_C, dev, case, f"composite_fwd S={S} NR={NR} occ={in_is_occ} {regime}", sum_bounds=sum_bounds)


@pytest.mark.parametrize("outputs", ["term", "no_term"])
@pytest.mark.parametrize("in_is_occ", [0, 1])
@pytest.mark.parametrize("S", [1, 65, 200])
def test_composite_fwd_optional_outputs(_C, dev, S, in_is_occ, outputs):
    got, _, _ = compare(_C, dev, M.composite_fwd_case(5, S, in_is_occ, "ordinary", outputs),
                        f"composite_fwd S={S} occ={in_is_occ} outputs={outputs}")
    assert set(got) == ({"term"} if outputs == "term" else {"depth", "var", "rgb", "opacity"})


def test_composite_argument_errors(_C, dev):
    name, a = M.composite_fwd_case(5, 65, 0, "ordinary")
    d = [t.to(dev) if torch.is_tensor(t) else t for t in a]
    with pytest.raises(_C.CnrError):                       # rgb without color
        _C.call(name, d[0], None, d[2], d[3], d[4], d[5], d[6], d[7], *d[8:])
    with pytest.raises(_C.CnrError):                       # depth without z
        _C.call(name, d[0], d[1], None, d[3], d[4], d[5], d[6], d[7], *d[8:])
    alpha513, dalpha513 = torch.zeros(1, 513, device=dev), torch.zeros(1, 513, device=dev)
    with pytest.raises(_C.CnrError):                       # S = 513: CNR_E_SHAPE (carry_in[8]); nothing is launched
        _C.call("cnr_composite_bwd", alpha513, None, None, None, None, None, None, dalpha513, None, 1, 513, 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("regime", M.REGIMES)
@pytest.mark.parametrize("in_is_occ", [0, 1])
@pytest.mark.parametrize("NR", M.COMPOSITE_NR)
@pytest.mark.parametrize("S", M.COMPOSITE_BWD_S)
def test_composite_bwd(_C, dev, S, NR, in_is_occ, regime):
    compare(_C, dev, M.composite_bwd_case(NR, S, in_is_occ, regime), f"composite_bwd S={S} NR={NR} occ={in_is_occ} {regime}")


@pytest.mark.parametrize("upstream", M.UPSTREAMS[1:])
@pytest.mark.parametrize("regime", M.REGIMES)
@pytest.mark.parametrize("in_is_occ", [0, 1])
@pytest.mark.parametrize("S", M.COMPOSITE_BWD_S)
def test_composite_bwd_upstream_sets(_C, dev, S, in_is_occ, regime, upstream):
    """d_term alone with color = z = d_color = None (TerminationFn), d_depth alone, d_rgb + d_opacity."""
    got, _, _ = compare(_C, dev, M.composite_bwd_case(5, S, in_is_occ, regime, upstream),
                        f"composite_bwd S={S} occ={in_is_occ} {regime} upstream={upstream}")
    if upstream == "d_depth":
        M.check_exact(got["d_color"], torch.zeros(5, S, 3), "d_color without d_rgb")


# ---- cnr_loss_fwd_bwd ----------------------------------------------------------------------------------------------
def _loss_zero_rows_exact(got, R):
    zr = M.loss_zero_rows(R)
    C = got["d_depth"].shape[0]
    for k, rows in (("d_depth", zr["depth"]), ("d_rgb", zr["rgb"]), ("d_opacity", zr["opacity"])):
        if bool(rows.any()):
            M.check_exact(got[k][:, rows], torch.zeros_like(got[k][:, rows]), f"{k} of exact-tie rows")
    assert C == got["flags"].shape[0]


@pytest.mark.parametrize("scalings", M.LOSS_SCALINGS)
@pytest.mark.parametrize("R", M.LOSS_R)
@pytest.mark.parametrize("C", [1, 3])
def test_loss(_C, dev, C, R, scalings):
    got, _, _ = compare(_C, dev, M.loss_case(C, R, scalings), f"loss C={C} R={R} scalings={scalings}")
    assert got["flags"].tolist() == [0] * C
    _loss_zero_rows_exact(got, R)


@pytest.mark.parametrize("variant,flag", [("empty_depth", 2), ("empty_object", 6), ("empty_surface", 8)])
def test_loss_empty_masks(_C, dev, variant, flag):
    """the emptied mask is in class 1 only; the rule zeroes the term, and raises the flag, for every class"""
    got, _, _ = compare(_C, dev, M.loss_case(3, 257, M.LOSS_SCALINGS[0], variant), f"loss {variant}")
    assert got["flags"].tolist() == [flag] * 3
    _loss_zero_rows_exact(got, 257)


@pytest.mark.parametrize("C,R", [(1, 1), (3, 257)])
def test_loss_explode_flag(_C, dev, C, R):
    """var = 0 and depth residuals >= 200 in the last class: its depth loss is >= 10 x the 1e5 threshold.  The oracle
    stops there like the reference does, so the values are compared with the masked means written out directly."""
    case = M.loss_case(C, R, M.LOSS_SCALINGS[0], "explode")
    got = launch(_C, dev, case)
    want, ref = M.loss_direct(F64, case[1]), M.loss_direct(F32, case[1])
    assert want["flags"].tolist() == [0] * (C - 1) + [1]
    for k in ("flags", "losses", "d_depth", "d_rgb", "d_opacity"):
        M.check(got[k], want[k], ref[k], f"loss explode C={C} R={R} {k}")


# ---- cnr_adamw_step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unscale", [1.0, 1.0 / 1024])
@pytest.mark.parametrize("n", M.ADAMW_N)
def test_adamw(_C, dev, n, unscale):
    """three steps; 2048 * 256 + 300 elements wrap the grid-stride loop.  Host step count and the device's d_state[2] + 1
    agree bit for bit; both against the fp64 restatement of torch.optim.AdamW, with torch's own fp32 AdamW as yardstick."""
    p0, grads = M.adamw_case(n)
    h = M.ADAMW_HYPER

    def run(device_step):
        p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        for t in range(1, M.ADAMW_STEPS + 1):
            state = torch.tensor([0, 0, t - 1], dtype=torch.int64, device=dev) if device_step else None
            _C.call("cnr_adamw_step", p, grads[t - 1].to(dev), m, v, n, h["lr"], h["beta1"], h["beta2"], h["eps"],
                    h["weight_decay"], 0 if device_step else t, unscale, state)
        torch.cuda.synchronize()
        return p.cpu(), m.cpu(), v.cpu()

    host, device = run(False), run(True)
    want, ref = M.adamw_fp64(p0, grads, unscale, **h), M.adamw_torch(F32, p0, grads, unscale, **h)
    for a, b, w, r, k in zip(host, device, want, ref, ("param", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), f"{k}: host step count and d_state disagree"
        M.check(a, w, r, f"adamw n={n} unscale={unscale} {k}")
