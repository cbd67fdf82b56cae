"""The depth-guided ray sampler (csrc/sample_common.h, csrc/sample.hip) restated on the CPU, for tests/test_sampler_host.py
(no GPU) and tests/test_sampler_gpu.py.

Written from the definitions, not from the device code: Philox4x32-10 as published (Salmon et al., Random123), the
counter layout include/cnr_hip.h states, Box-Muller, and the reference's sample_3d_points (oracle/ref_cpu.py) for the z
arithmetic.  Every floating input of a case is DRAWN in float32; `expected` evaluates the oracle on float64 copies (the
truth) and on the float32 originals (the yardstick), the two-evaluation scheme of tests/modular_cases.py."""
import collections

import numpy as np
import torch

import modular_cases as M
from oracle import ref_cpu as O

F32, F64 = torch.float32, torch.float64
MASK64 = (1 << 64) - 1
U32 = np.uint64(0xFFFFFFFF)
SH32, SH8 = np.uint64(32), np.uint64(8)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # the two multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85                            # the key schedule's two Weyl increments
GAUSS_HI_XOR = 0x9E3779B97F4A7C15                                        # high counter word of the Gaussian draws: offset ^ this
TWO_PI_F32 = np.float32(6.28318530718)                                   # the constant as a float32 holds it
EPS, STOP_EPS = 0.1, 0.05
MAX_IN_KERNEL_S = 256                                                    # uniform column blocks 0..3: what one step's stride of 4 holds


def f32(v):
    """the value a float parameter of the C ABI has"""
    return float(np.float32(v))


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter: four, key: two arrays of 32-bit words (held in uint64, broadcast together) -> uint32 (..., 4).
    Ten rounds of: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2, c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is
    raised by (W0, W1) between rounds."""
    c = [_u64(w) & U32 for w in counter]
    k = [_u64(w) & U32 for w in key]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(PHILOX_W0)) & U32, (k[1] + np.uint64(PHILOX_W1)) & U32]
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> SH32) ^ c[1] ^ k[0], p1 & U32, (p0 >> SH32) ^ c[3] ^ k[1], p0 & U32]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def philox4(seed, ctr_lo, ctr_hi):
    """The sampler's use of it: key = the 64-bit seed, counter = (ctr_lo, ctr_hi), each as (low word, high word)."""
    lo, hi, s = _u64(ctr_lo), _u64(ctr_hi), _u64(int(seed) & MASK64)
    return philox4x32_10((lo & U32, lo >> SH32, hi & U32, hi >> SH32), (s & U32, s >> SH32))


def u01(x):
    """the top 24 bits of a word as a multiple of 2^-24 in [0, 1): exact in float32 (and in float64, returned here)"""
    return (_u64(x) >> SH8).astype(np.float64) * 2.0 ** -24


# ---- the counter layout -----------------------------------------------------------------------------------------------
def counters(offset, step, rng_ray, lane, block):
    """-> (low word, high word of the Gaussians, high word of the uniforms of column block `block`), all mod 2^64"""
    o = (int(offset) + 4 * int(step)) & MASK64
    with np.errstate(over="ignore"):
        lo = _u64(rng_ray) * np.uint64(64) + _u64(lane)
        hi_u = _u64((o + 1) & MASK64) + _u64(block)
    return lo, _u64(o ^ GAUSS_HI_XOR), hi_u


def draw_words(seed, offset, step, rng_ray, lane, block):
    """-> (the four Gaussian words of lane `lane` of the ray with Philox index rng_ray, (..., 4) uint32;
           the uniform word of that lane in column block `block`, (...) uint32) at rng step `step`"""
    lo, hi_g, hi_u = counters(offset, step, rng_ray, lane, block)
    return philox4(seed, lo, hi_g), philox4(seed, lo, hi_u)[..., 0]


def rng_index(c, r, R, rng=(0, 0, 0, 0)):
    """Philox index of ray r of local class c; rng = (c0, cstride, R_global, r0): the ray's index in the global batch of which
    this call holds classes c0, c0 + cstride, ... and rays r0 .. r0 + R - 1.  R_global = 0: the local index c R + r."""
    c0, cstride, R_global, r0 = rng
    c, r = np.asarray(c, dtype=np.uint64), np.asarray(r, dtype=np.uint64)
    if R_global <= 0:
        return c * np.uint64(R) + r
    return (c * np.uint64(max(cstride, 1)) + np.uint64(c0)) * np.uint64(R_global) + np.uint64(r0) + r


def ray_indices(C, R, rng=(0, 0, 0, 0)):
    return rng_index(np.arange(C)[:, None], np.arange(R)[None, :], R, rng).reshape(-1)


def ray_uniforms(seed, offset, step, rays, S):
    """u (N, S) float32 of the rays with Philox indices `rays`: column s is lane s % 64 of block s // 64"""
    s = np.arange(S)
    _, w = draw_words(seed, offset, step, np.asarray(rays)[:, None], (s % 64)[None, :], (s // 64)[None, :])
    return u01(w).astype(np.float32)


def ray_gauss_words(seed, offset, step, rays):
    """(N, 64, 4) uint32: the Gaussian words of the 64 lanes of each ray"""
    w, _ = draw_words(seed, offset, step, np.asarray(rays)[:, None], np.arange(64)[None, :], 0)
    return w


# ---- Box-Muller -------------------------------------------------------------------------------------------------------
def _pairs(words):
    words = np.asarray(words)
    return ((words[..., 0], words[..., 1]), (words[..., 2], words[..., 3]))


def gauss(words, eps, dtype=np.float64):
    """words (..., 4) -> (..., 2): element `lane` from words 0, 1 and element `lane + 64` from words 2, 3, each
    sd * sqrt(-2 log(1 - u01(w0))) * cos(2 pi u01(w1)) with sd = float32(eps) / 3 formed in float32 and the float32 2 pi.
    dtype float64: the value; float32: the same with every operation rounded on its own."""
    t = np.dtype(dtype).type
    sd = t(np.float32(eps) / np.float32(3.0))
    out = []
    for w0, w1 in _pairs(words):
        u0, u1 = u01(w0).astype(t), u01(w1).astype(t)
        r = np.sqrt(t(-2.0) * np.log(t(1.0) - u0))
        out.append(sd * r * np.cos(t(TWO_PI_F32) * u1))
    return np.stack(out, -1)


def gauss_tol(words, eps):
    """How far a draw moves when either of its uniforms moves by 64 steps of the 2^-24 grid, from the derivatives
    dg/du0 = sd cos a / (r (1 - u0)) and dg/du1 = -2 pi sd r sin a: sd 2^-18 (|cos a| / (r (1 - u0)) + 2 pi r |sin a|).
    (inf where u0 = 0: r = 0 there)"""
    sd = float(np.float32(eps) / np.float32(3.0))
    out = []
    for w0, w1 in _pairs(words):
        u0, a = u01(w0), float(TWO_PI_F32) * u01(w1)
        r = np.sqrt(-2.0 * np.log(1.0 - u0))
        with np.errstate(divide="ignore"):
            out.append(sd * 2.0 ** -18 * (np.abs(np.cos(a)) / (r * (1.0 - u0)) + 2.0 * np.pi * r * np.abs(np.sin(a))))
    return np.stack(out, -1)


def per_ray(x, n2):
    """(N, 64, 2) per-lane pairs -> (N, n2): element e of a ray is pair e // 64 of lane e % 64"""
    return np.concatenate([x[..., 0], x[..., 1]], -1)[:, :n2]


# ---- cases ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "rgbs depth dirs T u g")
INVALID, THIS, OTHER0, OTHER2 = 0, 1, 2, 3
# five row kinds in turn: a class of R >= 5 rows holds all of them, and since 5 and the block's four waves share no factor a
# kind moves through the waves of the blocks
PATTERN = (THIS, INVALID, OTHER0, THIS, OTHER2)
TINY_DEPTH = 2.0 ** -20


def row_kinds(C, R, rot=0):
    return torch.tensor([[PATTERN[(r + c + rot) % 5] for r in range(R)] for c in range(C)])


def sim3_poses(g, n):
    """n poses (4, 4): rotation x scale in [0.5, 2], translation ~ N(0, 1); values rounded to float32"""
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=F64))
    q = q * torch.linalg.det(q).sign()[:, None, None]
    s = 0.5 + 1.5 * torch.rand(n, generator=g, dtype=F64)
    T = torch.zeros(n, 4, 4, dtype=F64)
    T[:, :3, :3] = q * s[:, None, None]
    T[:, :3, 3] = torch.randn(n, 3, generator=g, dtype=F64)
    T[:, 3, 3] = 1.0
    return T.to(F32)


def build_case(C, R, n1, n2, min_bound=0.0, seed=0, rot=0, tiny=False, eps=EPS):
    """-> Case(rgbs (C, R, 4) u8, depth (C, R), dirs (C, R, 3), T (C, R, 4, 4), u (C, R, n1 + n2), g (C, R, n2)).
    Row r of class c is of kind PATTERN[(r + c + rot) % 5]: depth <= min_bound (any state), or a valid depth in [0.5, 3.5]
    with state 1 (this object), 0 or 2.  Invalid row j of a class has depth == min_bound exactly when j is even, else a
    depth below it (0 when min_bound is 0); with R >= 5 the last valid row of a class has depth nextafter(min_bound, inf).
    tiny (min_bound = 0): the second this-object row of each class has depth 2^-20, so that z = d + g rounds g by far
    less than the Gaussian bar."""
    gen = M.gen(7919 * seed + 1000 * C + 100 * R + 10 * n1 + n2 + (5 if min_bound else 0))
    kinds = row_kinds(C, R, rot)
    depth = 0.5 + 3.0 * M.rand(gen, C, R)
    state = torch.randint(0, 3, (C, R), generator=gen)
    state[kinds == THIS], state[kinds == OTHER0], state[kinds == OTHER2] = 1, 0, 2
    below = min_bound * M.rand(gen, C, R)
    nxt = float(np.nextafter(np.float32(min_bound), np.float32(np.inf)))
    for c in range(C):
        inv = torch.nonzero(kinds[c] == INVALID).flatten().tolist()
        for j, r in enumerate(inv):
            depth[c, r] = min_bound if j % 2 == 0 else below[c, r]
        val = torch.nonzero(kinds[c] != INVALID).flatten().tolist()
        if R >= 5:
            depth[c, val[-1]] = nxt
        this = torch.nonzero(kinds[c] == THIS).flatten().tolist()
        if tiny and min_bound == 0.0 and len(this) >= 2 and this[1] != val[-1]:
            depth[c, this[1]] = TINY_DEPTH
    rgbs = torch.randint(0, 256, (C, R, 4), generator=gen).to(torch.uint8)
    rgbs[..., 3] = state.to(torch.uint8)
    dirs = torch.cat([M.rand(gen, C, R, 2) - 0.5, torch.ones(C, R, 1)], -1)
    T = sim3_poses(gen, C * R).view(C, R, 4, 4)
    u = M.rand(gen, C, R, n1 + n2)
    g = M.randn(gen, C, R, n2) * f32(np.float32(eps) / np.float32(3.0))
    return Case(rgbs.contiguous(), depth.contiguous(), dirs.contiguous(), T.contiguous(), u.contiguous(), g.contiguous())


def branches(case, min_bound):
    """-> {invalid, this, other}: (C, R) masks of the rows of each z branch (free space: the columns s < n1 of the valid rows)"""
    invalid = case.depth <= min_bound
    state = case.rgbs[..., 3]
    return {"invalid": invalid, "this": ~invalid & (state == 1), "other": ~invalid & (state != 1)}


def expected(case, n1, n2, eps, stop_eps, min_bound, world_frame, dtype):
    """oracle.ref_cpu's origin_dirs_O / origin_dirs_W and sample_3d_points per class, on the case's values in `dtype`; the
    slice maximum is torch.max over the class's rows, as the reference takes it.  eps, stop_eps and min_bound are the float32
    values the kernel receives."""
    eps, stop_eps, min_bound = f32(eps), f32(stop_eps), f32(min_bound)
    keys = ("z", "pts", "origins", "dirs_o", "gt_rgb", "gt_depth", "depth_mask", "labels")
    out = {k: [] for k in keys}
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        for c in range(case.depth.shape[0]):
            T, dirs = case.T[c].to(dtype), case.dirs[c].to(dtype)
            org, dro = (O.origin_dirs_W if world_frame else O.origin_dirs_O)(T, dirs)
            rgb, d, valid, state, pts, z = O.sample_3d_points(case.rgbs[c], case.depth[c].to(dtype), org, dro, case.u[c].to(dtype),
                                                              case.g[c].to(dtype), n1, n2, eps, stop_eps, min_bound)
            for k, v in zip(keys, (z, pts, org, dro, rgb.to(dtype) / 255.0, d, valid.to(torch.uint8), state)):
                out[k].append(v)
    finally:
        torch.set_default_dtype(old)
    return {k: torch.stack(v) for k, v in out.items()}


def groups(case, n1, min_bound):
    """name -> (row mask (C, R), column slice) of the z / pts comparison groups: an easy branch does not borrow a hard one's e_r"""
    b = branches(case, min_bound)
    S = case.u.shape[-1]
    valid = ~b["invalid"]
    return {"invalid": (b["invalid"], slice(0, S)), "free": (valid, slice(0, n1)), "other": (b["other"], slice(n1, S)),
            "this": (b["this"], slice(n1, S))}


def check_groups(got, want64, ref32, case, n1, min_bound, what, only=None, rays=True):
    """modular_cases.check per group on z and pts (and on origins with dirs_o as one group) -> {group: rows}.
    only: the groups to hold (default all four)."""
    rows = {}
    for name, (mask, cols) in groups(case, n1, min_bound).items():
        rows[name] = int(mask.sum())
        if (only is not None and name not in only) or rows[name] == 0 or cols.stop <= cols.start:
            continue
        for k in ("z", "pts"):
            sel = lambda t: t.detach().cpu()[mask][:, cols]
            M.check(sel(got[k]), sel(want64[k]), sel(ref32[k]), f"{what} {name} {k} ({rows[name]} rows)")
    if rays:
        cat = lambda o: torch.cat([o["origins"].detach().cpu().reshape(-1), o["dirs_o"].detach().cpu().reshape(-1)])
        M.check(cat(got), cat(want64), cat(ref32), f"{what} origins+dirs_o")
    print(f"{what}: rows per branch {rows}")
    return rows


# ---- the shapes of tests/test_sampler_gpu.py (a), shared with the host test of the yardstick ---------------------------------------
RECORDED_N = [(0, 1), (1, 9), (3, 33), (1, 63), (0, 64), (1, 64), (8, 65), (16, 112), (64, 128), (130, 126), (130, 128)]
# (C, R, n1, n2, world_frame, min_bound): every (n1, n2) at (3, 67), every (C, R) at (3, 33) and (16, 112); frames and bounds alternate
RECORDED_CASES = [(3, 67, n1, n2, i % 2, 0.25 if i % 3 == 1 else 0.0) for i, (n1, n2) in enumerate(RECORDED_N)]
RECORDED_CASES += [(C, R, n1, n2, (j + k) % 2, 0.25 if (j + k) % 2 else 0.0)
                   for j, (C, R) in enumerate([(1, 1), (2, 5)]) for k, (n1, n2) in enumerate([(3, 33), (16, 112)])]


def recorded_rots(R):
    """R = 1 holds one row: the case is run once per row kind instead"""
    return (0, 1, 2) if R < 5 else (0,)
