"""CPU: the record-noise statistics of tests/record_noise.py on synthetic records, no kernel involved -- what the three GPU
gradient-equivalence tests (test_trainer_gpu, test_multigpu_gpu, test_fused_gpu) rely on.

512 contributions to 13 892 trunk entries (per-entry scales over 6 binades, every 17th column dead; one variant with
zero-mean columns, one with a coherent part) are split into nwg_A and nwg_B partial sums, each partial rounded fp32 -> bf16 into
a record, the records summed in fp32.  The two sides then differ by independent record rounding alone (the null), or by that
plus a planted error.  Expected under the null: chi2 = 1 with standard deviation sqrt(2 / n) (0.012 at n = 13 000, 0.044 at
n = 1024), z standard normal.  Measured here (both variants, the five splits): whole-trunk chi2 0.97 .. 1.01, |z| <= 1.9;
a planted 3e-4 scale error gives z = 4.3 .. 37, 1e-3 gives 16 .. 125, 2e-3 on one 1024-entry layer gives that layer's z >= 4.
"""
import math

import pytest
import torch

import record_noise as rn
from conftest import rel_l2
from record_noise import LATENT_BIASES, TR

K = 512
E = ((TR + 126 + rn.ROWS_MAX * 128 + 255) // 256) * 256          # csrc/records_common.h REC_ENTRIES (test_layout checks the library's)
SPLITS = [(1, 4), (3, 37), (8, 32), (32, 16), (256, 64)]
NAN_PATTERNS = [0x7fc0, -1, 0x7f81, -0x7f]                          # bf16 NaNs, both signs, quiet and signalling


@pytest.fixture(scope="module")
def cnr():
    import cnr_amd
    return cnr_amd


@pytest.fixture(scope="module")
def lay(cnr):
    return cnr.fused.ParamLayout(32, 4)


@pytest.fixture(scope="module")
def groups(cnr, lay):
    return rn.gradient_groups(lay, cnr.ops.TRUNK_LAYERS)


@pytest.fixture(scope="module", params=["zero_mean", "coherent"])
def chunks(request):
    """(variant, (K, TR) float64 contributions): computed once, never modified"""
    gen = torch.Generator().manual_seed(20 if request.param == "zero_mean" else 21)
    scale = torch.exp2(6 * torch.rand(1, TR, generator=gen, dtype=torch.float64)) * 1e-3
    x = torch.randn(K, TR, generator=gen, dtype=torch.float64) * scale
    if request.param == "coherent":
        x = x + 0.5 * scale * torch.randn(1, TR, generator=gen, dtype=torch.float64)
    x[:, torch.arange(TR) % 17 == 0] = 0.0
    return request.param, x


def _side(x, nwg, lay, n_obj=4, sums=False):
    """contributions (k, TR) -> what one launch leaves: nwg bf16 records (NaN patterns in the entries no launch writes), their
    fp32 sum and the predicted variance, both in the flat gradient's layout (1, P); sums: also step_record_sum of the workspace"""
    part = torch.zeros(nwg, TR, dtype=torch.float64).index_add_(0, torch.arange(x.shape[0]) % nwg, x)
    rec = torch.zeros(nwg, E, dtype=torch.bfloat16)
    rec[:, :TR] = part.float().to(torch.bfloat16)
    mask = rn.written_mask(E, n_obj, rows_in_record=False)
    bits = rec.view(torch.int16)
    bits[:, ~mask] = torch.tensor(NAN_PATTERNS, dtype=torch.int16)[torch.arange(int((~mask).sum())) % 4]
    ws = rec.reshape(-1).view(torch.uint8)                            # the workspace as the trainers hold it
    s = rn.class_records(ws, 1, nwg, E).float().sum(1)               # fp32 sum of the records
    s[:, ~mask] = 0.0
    g = rn.to_gradient_layout(s.double(), lay)
    v = rn.to_gradient_layout(rn.record_variance(ws, 1, nwg, E, mask), lay)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(v).all())
    if sums:
        assert torch.equal(rn.step_variance(ws, 1, nwg, E, n_obj, lay), v)
        return g, v, rn.step_record_sum(ws, 1, nwg, E, n_obj, lay)
    return g, v


def _report(xa, xb, na, nb, lay, groups):
    ga, va = _side(xa, na, lay)
    gb, vb = _side(xb, nb, lay)
    return rn.noise_report(ga - gb, gb, va + vb, groups), rel_l2(ga, gb)


def test_bf16_ulp_is_the_distance_to_the_next_bf16_for_every_pattern():
    bits = torch.arange(65536, dtype=torch.int32)
    mag = bits & 0x7FFF
    finite = mag < 0x7F80                                            # not inf, not NaN
    as_bf16 = lambda b: ((b + 32768) % 65536 - 32768).to(torch.int16).view(torch.bfloat16)     # 16-bit pattern -> bf16
    r = as_bf16(bits)
    got = rn.bf16_ulp(r)
    assert got.dtype == torch.float64 and bool(torch.isfinite(got).all())
    cur, nxt = as_bf16(mag).double(), as_bf16(mag + 1).double()
    want = nxt - cur
    top = mag == 0x7F7F                                              # the largest finite value: the next pattern is inf
    want[top] = 2.0 ** 120                                           # ... its binade's spacing, 2^(127 - 7)
    want[mag == 0] = 0.0                                             # r = 0 carries no rounding error: 0 by definition
    assert torch.equal(got[finite], want[finite])
    # the closed form, spelled out at the edges: smallest subnormal, largest subnormal, smallest normal, 1, -1
    for pattern, ulp in ((0x0001, 2.0 ** -133), (0x007F, 2.0 ** -133), (0x0080, 2.0 ** -133), (0x0100, 2.0 ** -132),
                         (0x3F80, 2.0 ** -7), (0xBF80, 2.0 ** -7), (0x0000, 0.0), (0x8000, 0.0)):
        assert float(got[pattern]) == ulp, hex(pattern)


@pytest.mark.parametrize("na,nb", SPLITS)
def test_null_is_chi2_one_and_z_normal(chunks, lay, groups, na, nb):
    variant, x = chunks
    rep, rl = _report(x, x, na, nb, lay, groups)
    print(rn.format_report(f"null {variant} {na}/{nb}", rep))
    t = rep["trunk"]
    dead = (torch.arange(TR) % 17 == 0) | ~rn.written_mask(E, 4)[:TR]
    assert t["n"] == TR and t["n_v0"] == int(dead.sum())             # dead columns + latent biases, nothing else
    assert 0.9 <= t["chi2"] <= 1.1, t
    assert abs(t["z"]) <= 4, t
    for name, r in rep.items():
        if r["n"] >= 1024:
            assert 0.8 <= r["chi2"] <= 1.2, (name, r)


@pytest.mark.parametrize("na,nb", SPLITS)
def test_planted_errors_are_found_below_the_backstop(chunks, lay, groups, na, nb):
    """what the 4e-3 relative-L2 backstop of the GPU tests cannot see: a scale error of 3e-4 / 1e-3 on one side, 2e-3 on one
    layer; a contribution left out"""
    variant, x = chunks
    for delta, zmin in ((3e-4, 4), (1e-3, 12)):
        rep, rl = _report(x * (1 + delta), x, na, nb, lay, groups)
        print(rn.format_report(f"scale {delta:g} {variant} {na}/{nb}", {"trunk": rep["trunk"]}))
        assert abs(rep["trunk"]["z"]) >= zmin, (delta, rep["trunk"])
        if delta == 3e-4:
            assert rl < 4e-3, rl                                     # today's assertion is blind to it
    # one layer-sized group (encoding_shape.weight: 1024 entries) scaled by 1 + 2e-3 on one side
    name = "encoding_shape.weight"
    sl = groups[name]
    assert sl.stop - sl.start == 1024
    xs = x.clone()
    xs[:, sl.start - lay.trunk[0]:sl.stop - lay.trunk[0]] *= 1 + 2e-3
    rep, rl = _report(xs, x, na, nb, lay, groups)
    print(rn.format_report(f"layer 2e-3 {variant} {na}/{nb}", {name: rep[name], "trunk": rep["trunk"]}))
    assert abs(rep[name]["z"]) >= 4, rep[name]
    assert rl < 4e-3, rl
    # one chunk of the 512 left out on one side
    rep, rl = _report(x[:-1], x, na, nb, lay, groups)
    print(rn.format_report(f"chunk dropped {variant} {na}/{nb}", {"trunk": rep["trunk"]}))
    assert rep["trunk"]["chi2"] > 1.25, rep["trunk"]


def test_split_difference_hands_the_latent_term_to_the_exact_channel(chunks, lay, groups):
    """A trunk entry of a latent-conditioned layer whose sample-path input is a nearly dead unit: its records hold 1e-10, its
    gradient is the latent path's term (0.1 here), and the two steps' terms differ by one fp32 ulp.  Against v_i ~ 1e-26 that
    ulp alone takes chi2 of the plain difference to 1e4 and more; split_difference takes it out exactly and chi2 is the null's."""
    variant, x = chunks
    j = 4928 + 5 * 119 + 17                                          # cat_layer.0.weight[5, 17]: a latent column
    x = x.clone()
    x[:, j] = 0.0
    x[3, j] = 1e-10
    (ga, va, sa), (gb, vb, sb) = [_side(x, n, lay, sums=True) for n in (8, 32)]
    lat = torch.zeros_like(ga)
    lat[0, lay.trunk[0] + j] = 0.1
    ga, gb = ga + lat * (1 + 2.0 ** -23), gb + lat
    d = ga - gb
    plain = rn.noise_report(d, gb, va + vb, groups)["trunk"]
    assert plain["chi2"] > 1e4, plain
    d_rec, d_exact = rn.split_difference(d, [sa], [sb])
    assert float((d_rec + d_exact - d).abs().max()) <= 1e-15 * float(d.abs().max())
    rep = rn.noise_report(d, gb, va + vb, groups, d_records=d_rec)["trunk"]
    print(rn.format_report(f"split {variant}", {"plain": plain, "split": rep}))
    assert 0.9 <= rep["chi2"] <= 1.1 and rep["over"] == 0, rep
    assert rep["delta"] == plain["delta"] and rep["d2"] == plain["d2"]           # every figure but chi2 is of d itself
    assert 0 < float(d_exact.norm()) / float(gb.norm()) < 1e-8


def test_layout(cnr, lay):
    """to_gradient_layout: entry TR + j and entry TR + 63 + j both land on B's element j, trunk entry i on trunk element i,
    nothing on the latent layers, their biases or the codes; record_variance: zero at the entries no launch writes, whatever
    their bits; written_mask is rec_entry_written."""
    assert rn.record_entries(cnr._C) == E
    C = 2
    x = torch.zeros(C, E, dtype=torch.float64)
    x[:, :TR] = 1.0 + torch.arange(TR, dtype=torch.float64)
    x[:, TR:TR + 63] = 1e6 * (1 + torch.arange(63, dtype=torch.float64))
    x[:, TR + 63:TR + 126] = 1e9 * (1 + torch.arange(63, dtype=torch.float64))
    x[:, TR + 126:] = 7e12                                           # row sums, padding: belong to no gradient entry here
    x[1] *= 2
    y = rn.to_gradient_layout(x, lay)
    assert y.shape == (C, lay.total)
    v = lay.views(y)
    for c in range(C):
        assert torch.equal(v["trunk"][c], x[c, :TR])
        assert torch.equal(v["B"][c].reshape(-1), x[c, TR:TR + 63] + x[c, TR + 63:TR + 126])
    for k in ("latW", "latb", "shape", "tex"):
        assert float(v[k].abs().sum()) == 0.0, k
    # masks
    for n_obj, rows in ((4, True), (4, False), (15, True), (16, True)):
        m = rn.written_mask(E, n_obj, rows)
        carried = n_obj * 128 if (rows and n_obj <= rn.ROWS_MAX) else 0
        assert int(m.sum()) == TR - 128 + 126 + carried
        for off in LATENT_BIASES:
            assert not bool(m[off:off + 32].any()) and bool(m[off - 1]) and bool(m[off + 32])
        assert bool(m[TR:TR + 126 + carried].all()) and not bool(m[TR + 126 + carried:].any())
    # variance: NaN patterns in the unwritten entries (planted as tests/test_tail_reduce_gpu.py plants them) change nothing
    gen = torch.Generator().manual_seed(5)
    nwg, n_obj = 5, 3
    recs = (torch.randn(C, nwg, E, generator=gen) * torch.exp2(4 * torch.rand(C, nwg, E, generator=gen)) * 1e-2).to(torch.bfloat16)
    mask = rn.written_mask(E, n_obj)
    clean = recs.clone()
    clean[:, :, ~mask] = 0
    dirty = recs.view(torch.int16).clone()
    dirty[:, :, ~mask] = torch.tensor(NAN_PATTERNS, dtype=torch.int16)[torch.arange(int((~mask).sum())) % 4]
    dirty = dirty.view(torch.bfloat16)
    assert bool(torch.isnan(dirty[:, :, ~mask].float()).all())
    v_clean = rn.record_variance(clean.reshape(-1).view(torch.uint8), C, nwg, E, mask)
    v_dirty = rn.record_variance(dirty.reshape(-1).view(torch.uint8), C, nwg, E, mask)
    assert v_clean.shape == (C, E) and v_clean.dtype == torch.float64
    assert torch.equal(v_clean, v_dirty) and bool(torch.isfinite(v_dirty).all())
    assert float(v_dirty[:, ~mask].abs().sum()) == 0.0 and bool((v_dirty[:, mask] > 0).all())
    want = (rn.bf16_ulp(clean[1, :, 100]) ** 2).sum() / 12
    assert math.isclose(float(v_clean[1, 100]), float(want), rel_tol=1e-15)
    # the stand-alone call's output order: dtrunk | dB | bias-row sums, class-major inside each
    flat = rn.to_standalone_layout(x, n_obj)
    assert flat.numel() == C * (TR + 63 + n_obj * 128)
    assert torch.equal(flat[TR:2 * TR], x[1, :TR]) and float(flat[C * TR]) == float(x[0, TR] + x[0, TR + 63])
    assert float(flat[C * (TR + 63)]) == 7e12
