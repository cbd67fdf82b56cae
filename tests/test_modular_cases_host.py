"""No GPU: the case builders of tests/modular_cases.py meet their stated conditions, and the fp64 double the GPU tests
trust is itself checked against something independent of it (the closed form of the composite backward, exact-tie loss
rows, torch.optim.AdamW in fp64)."""
import numpy as np
import pytest
import torch

import modular_cases as M
from oracle import ref_cpu as O

F64, F32 = torch.float64, torch.float32


# ---- builders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N", [(1, 1), (3, 255), (2, 257), (2, 300)])
@pytest.mark.parametrize("scale", [1.0, 2.0, 10.0])
def test_pe_builder(C, N, scale):
    _, x, B = M.pe_inputs(C, N, scale, 11)
    assert x.dtype == F32 and B.dtype == F32 and x.shape == (C, N, 3) and B.shape == (C, 21, 3)
    assert (N * 129) % 256 != 0
    assert float((x / scale).abs().max()) <= 1.0
    if N > 1:
        assert bool((x[:, N // 2] == 0).all())
    p = torch.matmul(x.double() / scale, B.double().transpose(-1, -2)).abs().amax((1, 2))
    if C > 1:
        assert 2.9 < float(p[-1]) < 3.1 and float(p[:-1].max()) < 2.0
    name, args = M.pe_bwd_case(C, N, scale, True)
    assert bool(torch.isnan(args[4]).all()) and bool((args[3] != 0).all())
    assert M.pe_bwd_case(C, N, scale, False)[1][4] is None


@pytest.mark.parametrize("C,R,S", M.MLP_BWD_SHAPES)
def test_mlp_builder_has_no_relu_tie_in_either_precision(C, R, S):
    m = M.mlp_inputs(C, R, S)
    assert m["e"].dtype == F32 and m["e"].shape == (C, R, S, 129) and m["trunk"].shape == (C, M.TRUNK_SIZE)
    assert float(m["zlat"].min()) >= 0.0 and float(m["zlat"].max()) > 0.0 and float(m["pts"].abs().max()) <= 1.0
    assert torch.equal(m["e"], O.unidirs_embed(m["pts"], m["B"], 1.0))
    a64, a32 = M.preacts(F64, m["e"], m["zlat"], m["trunk"]), M.preacts(F32, m["e"], m["zlat"], m["trunk"])
    assert [a.shape[-1] for a in a64] == [32, 32, 32, 32, 32, 32, 16]
    closest = min(float(a.abs().min()) for a in a64)
    moved = max(float((b.double() - a).abs().max()) for a, b in zip(a64, a32))
    print(f"mlp {C}x{R}x{S}: {m['redrawn']} samples redrawn, closest pre-activation {closest:.3e}, "
          f"fp32 vs fp64 pre-activation max {moved:.3e}")
    assert closest >= M.TIE_MARGIN
    assert moved < 1e-5          # the tie margin is ten times what fp32 can move a pre-activation
    # the masks both precisions take are therefore the same
    assert all(torch.equal(a > 0, b > 0) for a, b in zip(a64, a32))
    # building twice gives the same case (seeded redraws)
    M._mlp_cache.pop((C, R, S))
    assert torch.equal(M.mlp_inputs(C, R, S)["e"], m["e"])
    if R >= 3:
        _, args = M.mlp_bwd_case(C, R, S, zero_rays=True)
        zr = M.mlp_zero_rays(R)
        assert bool(zr.any()) and not bool(zr.all())
        assert float(args[3][:, zr].abs().max()) == 0 and float(args[4][:, zr].abs().max()) == 0
        assert float(args[3][:, ~zr].abs().min()) > 0


def test_mlp_shapes_reach_the_paths_they_are_for():
    N = 2053 * 64
    tiles = (N + 255) // 256
    blocks = min(tiles, 512)
    tpb = (tiles + blocks - 1) // blocks
    blocks = (tiles + tpb - 1) // tpb
    assert N > 131072 and tpb == 2
    last_tile_rows = N - (tiles - 1) * 256
    assert (tiles - 1) % 2 == 1 and 0 < last_tile_rows <= 64      # the last block's SECOND tile, one live wave
    assert 7 * 37 == 259 and 100 > 64


@pytest.mark.parametrize("S", sorted(set(M.COMPOSITE_FWD_S)))
@pytest.mark.parametrize("in_is_occ", [0, 1])
def test_composite_builder(S, in_is_occ):
    for NR in M.COMPOSITE_NR:
        _, a, c, z = M.composite_inputs(NR, S, in_is_occ, "ordinary")
        assert a.dtype == F32 and a.shape == (NR, S) and bool((z[:, 1:] >= z[:, :-1]).all())
        if in_is_occ:
            if S > 1:
                assert bool(((a == 0).sum(-1) >= 1).all()) and bool(((a == 1).sum(-1) >= 1).all())
            else:
                assert float(a[0, 0]) == 0.0 and (NR == 1 or float(a[1, 0]) == 1.0)
        _, a, _, _ = M.composite_inputs(NR, S, in_is_occ, "saturated")
        top = 1.0 if in_is_occ else 30.0
        hit = {int(i) for i in (a == top).double().argmax(-1)}
        assert bool(((a == top).sum(-1) >= 1).all())
        want = {S - 1 if i < 0 else i for i in M.SATURATED_AT if i < S}
        assert hit <= want and (NR < 9 or hit == want)
        _, a, _, _ = M.composite_inputs(NR, S, in_is_occ, "thin")
        occ = a.double() if in_is_occ else torch.sigmoid(a.double())
        assert float(torch.cumprod(1 - occ, -1)[:, -1].min()) > (0.01 if S <= 512 else 0.005)   # transmittance survives
        assert S < 129 or float((occ[:, 128:].sum(-1)).min()) > 1e-3                             # and is absorbed late
        _, a, _, _ = M.composite_inputs(NR, S, in_is_occ, "empty")
        assert bool((a == (torch.sigmoid(torch.tensor(-30.0)) if in_is_occ else -30.0)).all())


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("R", M.LOSS_R)
@pytest.mark.parametrize("scalings", M.LOSS_SCALINGS)
def test_loss_builder_and_exact_tie_rows(C, R, scalings):
    name, args = M.loss_case(C, R, scalings)
    depth, var, rgb, opa, gt_d, gt_c, labels, dmask = args[:8]
    zr = M.loss_zero_rows(R)
    rd = (depth.double() - gt_d.double()).abs()
    rc = (rgb.double() - gt_c.double()).abs()
    ro = (opa.double() - (labels != 0).double()).abs()
    for r, rows, k in ((rd, zr["depth"], "depth"), (rc, zr["rgb"], "rgb"), (ro, zr["opacity"], "opacity")):
        assert bool((r[:, rows] == 0).all()) and (bool(rows.any()) or R < 3), k
        if bool((~rows).any()):
            assert float(r[:, ~rows].min()) >= M.MIN_RESIDUAL, k
    assert R < 4 or bool((var[:, zr["var"]] == 0).all()) and float(var[:, ~zr["var"]].min()) > 0
    assert labels.dtype == torch.uint8 and dmask.dtype == torch.uint8
    # the double: an exact-tie row has gradient exactly 0, and no flag is raised
    for dtype in (F64, F32):
        out = M.oracle(name, dtype, *args)
        assert np.array_equal(out["flags"].numpy(), np.zeros(C, np.int32))
        assert bool((out["d_depth"][:, zr["depth"]] == 0).all())
        assert bool((out["d_rgb"][:, zr["rgb"]] == 0).all())
        assert bool((out["d_opacity"][:, zr["opacity"]] == 0).all())
        assert float(out["losses"].max()) < 1e4
        # and agrees with the masked means written out directly
        d = M.loss_direct(dtype, args)
        tol = 1e-12 if dtype == F64 else 1e-5
        for k in ("losses", "d_depth", "d_rgb", "d_opacity"):
            assert float((out[k] - d[k]).abs().max()) <= tol * float(d[k].abs().max()), k


@pytest.mark.parametrize("variant,flag", [("empty_depth", 2), ("empty_object", 6), ("empty_surface", 8)])
def test_loss_builder_empty_masks(variant, flag):
    name, args = M.loss_case(3, 257, M.LOSS_SCALINGS[0], variant)
    labels, dmask = args[6], args[7]
    mo, ms = labels != 0, labels != 2
    md = (dmask != 0) & mo
    counts = [(m.sum(-1) == 0).tolist() for m in (md, mo, ms)]
    want = {"empty_depth": [[0, 1, 0], [0, 0, 0], [0, 0, 0]], "empty_object": [[0, 1, 0], [0, 1, 0], [0, 0, 0]],
            "empty_surface": [[0, 0, 0], [0, 0, 0], [0, 1, 0]]}[variant]
    assert counts == [[bool(v) for v in row] for row in want]
    if variant == "empty_depth":
        assert int(mo[1].sum()) > 0
    out = M.oracle(name, F64, *args)
    assert out["flags"].tolist() == [flag] * 3          # the rule zeroes the term for EVERY class
    term = {"empty_depth": [0], "empty_object": [0, 1], "empty_surface": [2]}[variant]
    for t in term:
        assert float(out["losses"][t].abs().max()) == 0.0
    assert np.array_equal(M.loss_direct(F64, args)["flags"].numpy(), out["flags"].numpy())


@pytest.mark.parametrize("C,R", [(1, 1), (3, 257)])
def test_loss_builder_explode(C, R):
    name, args = M.loss_case(C, R, M.LOSS_SCALINGS[0], "explode")
    for dtype in (F64, F32):
        with pytest.raises(O.LossExplode):               # the oracle stops here, like the reference
            M.oracle(name, dtype, *args)
        d = M.loss_direct(dtype, args)
        assert d["flags"].tolist() == [0] * (C - 1) + [1]
        assert float(d["losses"][0, -1]) >= 1e6          # ten times the threshold: the flag cannot depend on rounding
        assert float(d["losses"][:, :-1].max() if C > 1 else 0.0) < 1e4 and float(d["losses"][1:, -1].max()) < 1e4


# ---- the double against something independent of it ------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 65, 130])
@pytest.mark.parametrize("in_is_occ", [0, 1])
@pytest.mark.parametrize("upstream", M.UPSTREAMS)
def test_composite_double_equals_closed_form(S, in_is_occ, upstream):
    worst = 0.0
    for regime in M.REGIMES:
        name, args = M.composite_bwd_case(5, S, in_is_occ, regime, upstream)
        alpha, color, z, dd, dr, do, dt = args[:7]
        out = M.oracle(name, F64, *args)
        want = M.composite_closed_form(alpha, color, z, dd, dr, do, dt, in_is_occ)
        got = out["d_alpha"].numpy()
        rel = float(np.abs(got - want).max() / np.abs(want).max())
        worst = max(worst, rel)
        assert rel <= 1e-12, (regime, rel)
        if "d_color" in out and dr is not None:
            occ = alpha.double() if in_is_occ else torch.sigmoid(alpha.double())
            f = 1.0 - occ + 1e-10
            T = torch.cat([torch.ones(5, 1, dtype=F64), torch.cumprod(f, -1)[:, :-1]], -1)
            dc = (occ * T)[..., None] * dr.double()[:, None, :]
            assert float((out["d_color"] - dc).abs().max()) <= 1e-12 * float(dc.abs().max())
    print(f"composite closed form vs the double's autograd, S={S} in_is_occ={in_is_occ} {upstream}: max rel {worst:.2e}")


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("unscale", [1.0, 1.0 / 1024])
def test_adamw_restatement_equals_torch_in_fp64(n, unscale):
    p0, grads = M.adamw_case(n)
    assert grads.shape == (3, n) and bool((grads[:, 0] == 0).all())
    for v in M.ADAMW_HYPER.values():
        assert float(np.float32(v)) == v
    want = M.adamw_torch(F64, p0, grads, unscale, **M.ADAMW_HYPER)
    got = M.adamw_fp64(p0, grads, unscale, **M.ADAMW_HYPER)
    for a, b, k in zip(got, want, ("param", "exp_avg", "exp_avg_sq")):
        assert float((a - b).abs().max()) <= 1e-14, k


def test_oracle_restores_the_default_dtype_and_leaves_inputs_alone():
    name, args = M.composite_fwd_case(5, 65, 0, "ordinary")
    before = [a.clone() if torch.is_tensor(a) else a for a in args]
    out = M.oracle(name, F64, *args)
    assert torch.get_default_dtype() == F32
    assert all(o.dtype == F64 for o in out.values()) and set(out) == {"term", "depth", "var", "rgb", "opacity"}
    for a, b in zip(args, before):
        assert (a is b) or torch.equal(a, b) or bool(torch.isnan(a).all())
    name, args = M.composite_fwd_case(5, 65, 0, "ordinary", "term")
    assert set(M.oracle(name, F32, *args)) == {"term"}


def test_order_independent_bound():
    name, args = M.composite_fwd_case(5, 600, 1, "thin")
    b = M.composite_depth_bound(args)
    out = M.oracle(name, F64, *args)
    assert b.shape == (5,) and torch.allclose(b, 16 * 2.0 ** -24 * out["depth"].abs())      # all addends positive
    w = out["depth"]
    M.check((w + 0.9 * b).float(), w, w.float(), "inside", sum_bound=b * 1.2)
    with pytest.raises(AssertionError):
        M.check((w + 2 * b).float(), w, w.float(), "outside", sum_bound=b)


def test_check_rule():
    w = torch.tensor([1.0, 2.0], dtype=F64)
    r = (w + torch.tensor([0.0, 1e-7])).float()
    M.check((w + 4e-7).float(), w, r, "inside")
    with pytest.raises(AssertionError):
        M.check((w + 2e-6).float(), w, r, "outside")
    with pytest.raises(AssertionError):
        M.check(torch.tensor([1.0, float("nan")]), w, r, "nan")
    with pytest.raises(AssertionError):
        M.check(torch.tensor([1, 2], dtype=torch.int32), torch.tensor([1, 3], dtype=torch.int32),
                torch.tensor([1, 3], dtype=torch.int32), "flags")
