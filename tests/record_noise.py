"""The rounding noise of the field backward's bf16 gradient records, predicted from the records themselves (CPU, float64).

A workgroup leaves its partial sums in a record of E bf16 entries (csrc/records_common.h); the step's last launch adds the nwg
records of a class in a fixed order, in fp32 (tests/test_tail_reduce_gpu.py pins that sum bit for bit).  Every entry was
rounded to nearest even ONCE, so its error lies within half a unit in the last place (ulp) and has variance ~ulp^2 / 12; the sum
is linear, so the variance of the rounding noise in gradient entry i is

    v_i = sum over the class's records of ulp(record entry i)^2 / 12

-- a number that can be read off the workspace after the step.  Two launches round independently, so for the difference
d = g_A - g_B of two paths that compute the same gradient v = v_A + v_B, and a test can ask whether d is EXPLAINED by the
records' rounding instead of holding it to a fixed bar that has to sit above the noise:

  * chi2  = mean over entries with v_i > 0 of d_i^2 / v_i: 1 under the null (standard deviation sqrt(2 / n)); anything in d
            that is not record rounding adds to it;
  * delta = <d, g> / <g, g>: a normalisation error is PARALLEL to the gradient, rounding noise is white across entries, so
            the projection has the standard deviation sd = sqrt(sum v_i g_i^2) / <g, g> -- a few 1e-5 where the noise's own
            relative size rho = sqrt(sum v_i) / |g| is a few 1e-3; z = delta / sd;
  * the same per group of entries (the whole trunk, each layer's weight, B).

What does NOT pass through a record carries v = 0 and belongs to no statistic of the record channel: the latent layers, their
biases inside the trunk and the code tables come from the per-object bias-row sums, which the trainers move through the exact
int64 fixed-point table -- and so does the term the latent path adds to the trunk entries of the four latent-conditioned
layers.  split_difference takes that part out of d (the record sums are recomputed here in float64) and hands it to the
"exact channel", which the tests hold to the bars the whole gradient had with fp32 records.
Two things to know when reading the figures (measured on MI355X, see the tests' docstrings):
  * the prediction assumes INDEPENDENT rounding.  Two launches that split a class's tiles over the same number of workgroups form
    the same partial sums to fp32 order and round them to the same bf16: d is then far below the prediction (chi2 ~ 0), and
    the checks are upper bounds;
  * chi2 has no floor.  An entry whose records hold ~1e-10 has v_i ~ 1e-26; any arithmetic difference of the two paths below
    the records' own size (an f16-subnormal upstream gradient present in one path only) is then 1e5 x v_i.  Such cases are named,
    with their cause, where they occur; "over5sd" in the [noise] lines counts the entries that carry them.
tests/test_record_noise_host.py proves the statistics on synthetic records, planted errors included.
"""
import math

import torch

TR = 13892                                   # trunk parameters = first dB record entry
LATENT_BIASES = (3840, 8736, 4896, 13281)    # biases of the latent-conditioned layers: no record entry is written for them
ROWS_MAX = 15                                # up to this many rows per class the record carries their sums behind the dB halves


def record_entries(_C):
    """E: entries of one record (bf16 each)"""
    return _C.field_bwd_workspace_bytes(1, 1) // 2


def bf16_ulp(r):
    """bf16 tensor -> float64: the spacing of bf16 at |r| (2^(floor(log2 |r|) - 7); the fixed 2^-133 below the normal range),
    0 for r = 0.  Reads the bit pattern alone: whatever the pattern, the result is finite."""
    assert r.dtype == torch.bfloat16
    bits = r.contiguous().view(torch.int16).to(torch.int32) & 0x7FFF
    e = (bits >> 7).clamp(min=1)                                     # biased exponent; subnormals share the first binade's spacing
    ulp = torch.exp2((e - 134).double())                             # 2^(e - 127 - 7)
    return torch.where(bits == 0, torch.zeros_like(ulp), ulp)


def written_mask(E, n_obj, rows_in_record=True):
    """(E,) bool: the entries a launch writes (csrc/records_common.h, rec_entry_written).  The rest is uncleared memory and must
    never reach a statistic.  rows_in_record: whether the per-object bias-row sums (up to ROWS_MAX rows per class) travel in the
    record and are to be read -- the trainers take them from the fixed-point table instead."""
    m = torch.ones(E, dtype=torch.bool)
    for off in LATENT_BIASES:
        m[off:off + 32] = False
    m[TR + 126 + (n_obj * 128 if (rows_in_record and n_obj <= ROWS_MAX) else 0):] = False
    return m


def class_records(ws, C, nwg, E):
    """the record workspace (any dtype, on the CPU) -> (C, nwg, E) bf16 view: class c's records are entries [c nwg E, (c + 1) nwg E)"""
    flat = ws.reshape(-1).view(torch.bfloat16)
    assert flat.numel() >= C * nwg * E, (flat.numel(), C, nwg, E)
    return flat[:C * nwg * E].view(C, nwg, E)


def record_variance(ws, C, nwg, E, mask):
    """(C, E) float64: sum over the class's records of ulp^2 / 12; 0 at the entries `mask` (written_mask) leaves out."""
    u = bf16_ulp(class_records(ws, C, nwg, E))
    v = (u * u).sum(1) / 12.0
    v[:, ~mask] = 0.0
    return v


def record_sum(ws, C, nwg, E, mask):
    """(C, E) float64: the sum of the class's records (exact in float64 up to its own 2^-53), 0 at the entries `mask` leaves out"""
    s = class_records(ws, C, nwg, E).double()
    s[:, :, ~mask] = 0.0
    return s.sum(1)


def to_gradient_layout(x, lay):
    """(C, E) per-entry quantities -> (C, lay.total) in the flat gradient's layout: trunk entry i at lay.trunk[0] + i, B entry j
    the SUM of entries TR + j and TR + 63 + j (variances add as the values do), every other slice 0."""
    out = torch.zeros(x.shape[0], lay.total, dtype=x.dtype)
    out[:, lay.trunk[0]:lay.trunk[0] + TR] = x[:, :TR]
    out[:, lay.B[0]:lay.B[0] + 63] = x[:, TR:TR + 63] + x[:, TR + 63:TR + 126]
    return out


def step_variance(ws, C, nwg, E, n_obj, lay):
    """a trainer's record workspace after a step -> (C, lay.total) predicted variance of the step's gradient (the bias-row sums
    a record may carry beside the fixed-point table are not read)"""
    return to_gradient_layout(record_variance(ws.cpu(), C, nwg, E, written_mask(E, n_obj, rows_in_record=False)), lay)


def step_record_sum(ws, C, nwg, E, n_obj, lay):
    """a trainer's record workspace after a step -> (C, lay.total) float64: what the records alone contribute to the gradient"""
    return to_gradient_layout(record_sum(ws.cpu(), C, nwg, E, written_mask(E, n_obj, rows_in_record=False)), lay)


def split_difference(d, record_sums_a, record_sums_b):
    """d = g_A - g_B of two steps -> (d_records, d_exact) with d = d_records + d_exact (float64):
      * d_records = (sum of A's record sums) - (sum of B's): the only part the records' rounding explains -- chi2 weighs it;
      * d_exact: everything else in the gradients -- the latent layers, their biases and the codes (no record at all), the term
        the latent path adds to the trunk entries of the four latent-conditioned layers, and the fp32 rounding of the reduction.
        It comes through the exact fixed-point table and is held to the bar the whole gradient had with fp32 records.
    The split is needed because chi2 = mean d_i^2 / v_i has no floor: on a trunk entry whose sample-path input is a (nearly) dead
    unit the records hold 0 or 1e-10 (v_i ~ 1e-26) while the latent path's term is a real gradient, and ONE fp32 ulp of that
    term (measured: d_i = 2^-33 on an entry of 1e-3, all records zero but one) is then 1e5 .. 1e15 times v_i."""
    d_records = sum(record_sums_a) - sum(record_sums_b)
    return d_records, d.detach().double().cpu() - d_records


def to_standalone_layout(x, n_obj):
    """(C, E) -> flat [dtrunk (C, TR) | dB (C, 63) | dbiasrows (C, n_obj, 128)]: the outputs of a stand-alone cnr_field_bwd_pipe
    call, whose bias-row sums come out of the record too (n_obj <= ROWS_MAX)."""
    assert n_obj <= ROWS_MAX
    return torch.cat([x[:, :TR].reshape(-1), (x[:, TR:TR + 63] + x[:, TR + 63:TR + 126]).reshape(-1),
                      x[:, TR + 126:TR + 126 + n_obj * 128].reshape(-1)])


def gradient_groups(lay, trunk_layers):
    """{name: column slice of the flat (C, lay.total) gradient}: the whole trunk, each trunk layer's weight tensor
    (trunk_layers = cnr.ops.TRUNK_LAYERS: (name, out, in) in blob order), B"""
    groups = {"trunk": slice(lay.trunk[0], lay.trunk[0] + TR)}
    off = lay.trunk[0]
    for n, o, i in trunk_layers:
        groups[n + ".weight"] = slice(off, off + o * i)
        off += o * i + o
    assert off == lay.trunk[0] + TR
    groups["B"] = slice(lay.B[0], lay.B[0] + 63)
    return groups


def noise_report(d, g, v, groups, d_records=None):
    """d = g_A - g_B, g the gradient to project on, v the predicted variance of d's rounding noise, all (..., P);
    groups {name: index into the last dimension}.  -> {name: dict(n, n_v0, left_out, chi2, over, delta, sd, z, rho, d2, g2,
    v_sum)}, everything in float64: n entries, n_v0 of them with v = 0 (left_out = their share), over = entries with
    d_i^2 > 25 v_i, d2 = |d|^2, g2 = |g|^2, v_sum = sum v.  chi2 is nan for a group without a single v > 0 entry; z is 0 where
    delta and sd both vanish.
    d_records: the part of d that is the difference of the RECORD sums (step_record_sum), where d has another part as well; chi2
    then weighs that part alone (see split_difference), every other figure is of d itself."""
    d, g, v = d.detach().double().cpu(), g.detach().double().cpu(), v.detach().double().cpu()
    dr = d if d_records is None else d_records.detach().double().cpu()
    out = {}
    for name, ix in groups.items():
        dk, gk, vk = d[..., ix].reshape(-1), g[..., ix].reshape(-1), v[..., ix].reshape(-1)
        pos = vk > 0
        n, n_v0 = dk.numel(), int((~pos).sum())
        q = dr[..., ix].reshape(-1)[pos] ** 2 / vk[pos]
        chi2 = float(q.mean()) if n_v0 < n else float("nan")
        over = int((q > 25).sum())                                   # entries beyond 5 sd: 6e-7 of them under the null
        g2, d2, v_sum = float(gk @ gk), float(dk @ dk), float(vk.sum())
        delta = float(dk @ gk) / g2 if g2 > 0 else 0.0
        sd = math.sqrt(float((vk * gk * gk).sum())) / g2 if g2 > 0 else 0.0
        z = delta / sd if sd > 0 else (0.0 if delta == 0 else math.copysign(math.inf, delta))
        rho = math.sqrt(v_sum / g2) if g2 > 0 else 0.0
        out[name] = dict(n=n, n_v0=n_v0, left_out=n_v0 / max(n, 1), chi2=chi2, over=over, delta=delta, sd=sd, z=z, rho=rho, d2=d2,
                         g2=g2, v_sum=v_sum)
    return out


def format_report(tag, rep):
    """one "[noise]" line per group"""
    return "\n".join(f"[noise] {tag} {name}: n={r['n']} v0={r['n_v0']} ({r['left_out']:.3f}) chi2={r['chi2']:.3f} over5sd={r['over']} "
                     f"delta={r['delta']:+.2e} sd={r['sd']:.2e} z={r['z']:+.2f} rho={r['rho']:.2e} "
                     f"rel_l2={math.sqrt(r['d2'] / r['g2']) if r['g2'] > 0 else 0.0:.2e}" for name, r in rep.items())
