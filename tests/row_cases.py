"""Structured rows, the fp64 definitions and the per-element acceptance bars of the DiT row kernels: LayerNorm (+ AdaLN
modulation, or affine), RMSNorm, and RMSNorm(q, k) + 3-axis RoPE + KV-cache write (csrc/ln_row.h, csrc/elementwise.hip; the fp8
quantiser of csrc/fp8_rows.hip shares the LayerNorm row).

Plain torch, CPU or GPU tensors.  tests/test_row_cases_cpu.py checks on the CPU what the builders promise, that an emulation
of the kernels' arithmetic stays inside the WORST CASE of every bar (half the bar) on every family, and that mutants of the
emulation fail; tests/test_row_kernels_gpu.py runs the HIP kernels on the same inputs.

Why structured rows: on iid Gaussian rows under a whole-tensor rel-L2 of 3e-3 a reduction that loses one 8-element chunk of a
5120-wide row (0.08 % of every output element, a fifth of a bf16 unit roundoff), one RoPE pair on the wrong axis or one row
with its neighbour's modulation all pass.  Here one chunk carries the row's sum, the frames' tables differ by a large
constant, the rows' magnitudes differ by 2^24, and every element is held to a bar of a few unit roundoffs of its own size.

What the bars do NOT pin: the intermediate bf16 rounding points.  A kernel that skips round_bf16(x * r) in the RMSNorm, or
rounds n * (1 + s) once instead of three times, stays inside them (it is closer to the fp64 definition, not further).  The
mismatch-fraction caps of tests/test_kernels_gpu.py against the eager chain keep that job.
"""
import math
from dataclasses import dataclass

import torch

U = 2.0 ** -8                # unit roundoff of bf16
U32 = 2.0 ** -24             # ... of fp32
MARGIN = 2.0                 # every bar = MARGIN x the worst case of the arithmetic (attn_cases: 4 against a worst case of 2)
EPS = 1e-6
THETA = 10000.0
THREADS = 256                # EW_THREADS: one workgroup per row
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------ acceptance
def within(out, ref, worst):
    """|out - ref| <= MARGIN * worst elementwise -> (ok, ratio, (row, column)): ratio = the largest |out - ref| / worst - the
    share of the WORST CASE used, so ok means ratio <= MARGIN - and where it is.  worst = 0 asks for out == ref exactly (0 / 0
    counts as ratio 0); a non-finite output element counts as an infinite ratio."""
    err = (out.double() - ref).abs()
    err = torch.where(torch.isfinite(out.double()), err, torch.full_like(err, math.inf))
    ok = bool((err <= MARGIN * worst).all())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / worst)
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    flat = int(ratio.argmax())
    return ok, float(ratio.max()), (flat // ratio.shape[-1], flat % ratio.shape[-1])


def sum_depth(d):
    """The constant c of the LayerNorm bar: the number of fp32 roundings on the longest path from an element of the row to the
    mean.  A thread adds its 8 * ceil(d / 2048) elements one after the other (ln_row.h: chunk threadIdx.x + 256 i, elements in
    order), wave_sum is a 6-step butterfly, block_sum adds the four wave partials in a chain of 3, and the division by d rounds
    once: c = 8 ceil(d / 2048) + 6 + 3 + 1 - 18 up to d = 2048, 42 at d = 8192.  (Higham, Accuracy and Stability, section 4.2:
    whatever the order, a sum errs by at most depth * 2^-24 * sum|x_i| to first order.)"""
    return 8 * ((d + 2047) // 2048) + 10


def frame_index(M, rows_per_frame, row_offset, device="cpu"):
    return (row_offset + torch.arange(M, device=device)) // rows_per_frame


def ln64(x, eps=EPS, weight=None, bias=None, shift=None, scale=None, rows_per_frame=0, row_offset=0):
    """LayerNorm in fp64 on the bf16 row the kernel receives, upcast: n = (x - mu) / sqrt(var + eps) with the two-pass
    (biased) variance; ref = n (plain), n w + b (affine) or n (1 + s_f) + sh_f (modulated: shift / scale are [F, d] tables, row
    r takes f = (row_offset + r) // rows_per_frame).  -> (ref, worst), both [M, d] float64; the bar is

        |out - ref| <= 2 (u cond + t32),     worst = u cond + t32,   u = 2^-8.

    cond: the magnitudes at the bf16 rounding points of ln_row.h.  Plain: |n|, the store.  Affine: |ref|, the store (the affine
    form computes (x - mean) rstd w + b in fp32).  Modulated: bf16(bf16(bf16(n) bf16(1 + s)) + sh) - the roundings of n, of
    1 + s and of their product each move the result by u |n| |1 + s|, the store by u |ref|: 3 |n| |1 + s| + |ref|.

    t32: the fp32 reductions.  The computed mean errs by delta <= c 2^-24 mean|x| <= c 2^-24 max|x|, c = sum_depth(d).  Every
    x - mean moves by delta, every output by delta rstd gain (gain = 1, |w| or |1 + s|) - an ABSOLUTE error that matters
    exactly where |n| is small next to |mu| rstd, the offset and near-constant rows.  The sum of squares has the same depth, so
    rstd errs by (c / 2 + 3) 2^-24 relative (its own rounding, var + eps and v_rsq_f32 included), moving an output by that
    times |n| gain; since max|x| rstd >= 1 on every row whose variance is not below eps this is under c 2^-24 max|x| rstd |n|
    gain, and where the variance is below eps it is under 2^-19 |n|, a 2000th of the u |n| already in cond.  Together

        t32 = c 2^-24 max|x| rstd (1 + |n|) gain.

    The shift of the squares' centre, sum (x - mean - delta)^2 = sum (x - mean)^2 + d delta^2, is second order: (delta rstd)^2
    of the variance, at most 1e-5 on the rows of this file."""
    xd = x.double()
    M, d = xd.shape
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    n = (xd - mu) * rstd
    if weight is not None:
        ref = n * weight.double() + bias.double()
        cond, gain = ref.abs(), weight.double().abs().expand_as(n)
    elif scale is not None:
        f = frame_index(M, rows_per_frame, row_offset, x.device)
        a = 1.0 + scale.double()[f]
        ref = n * a + shift.double()[f]
        cond, gain = 3.0 * n.abs() * a.abs() + ref.abs(), a.abs()
    else:
        ref, cond, gain = n, n.abs(), torch.ones_like(n)
    t32 = sum_depth(d) * U32 * xd.abs().amax(-1, keepdim=True) * rstd * (1.0 + n.abs()) * gain
    return ref, U * cond + t32


def rms64(x, weight, eps=EPS):
    """RMSNorm in fp64 on the bf16 row, upcast: ref = x w / sqrt(mean x^2 + eps).  -> (ref, worst) with worst = 2 u |ref|; the
    bar is |out - ref| <= 4 u |ref|.

    The kernel stores bf16(bf16(x r) w): two roundings, each at most u relative, 2 u |ref| in the worst case.  The sum of
    squares (42 roundings deep at most, all terms positive: 42 * 2^-24 relative, halved by the square root), the division, the
    + eps and v_rsq_f32 (1 ulp) together move r by under 2^-19 relative, a 2000th of u, which the margin takes."""
    xd = x.double()
    ref = xd * weight.double() / torch.sqrt((xd * xd).mean(-1, keepdim=True) + eps)
    return ref, 2.0 * U * ref.abs()


def axis_split(hd):
    """(c0, c1): pairs of a head on the temporal axis and on each of the two spatial axes."""
    c1 = (hd // 2) // 3
    return hd // 2 - 2 * c1, c1


def token_positions(M, grid, start_frame, row_offset, device="cpu"):
    """(frame position, grid row, grid column) of the global tokens row_offset .. row_offset + M on the (F, gh, gw) grid."""
    _, gh, gw = grid
    t = row_offset + torch.arange(M, device=device)
    f, rem = t // (gh * gw), t % (gh * gw)
    return start_frame + f, rem // gw, rem % gw


def rope_angles64(hd, pf, ph, pw):
    """Angles [M, hd / 2] in fp64 from the definition: pair j of an axis of c pairs turns by pos * 10000^(-j / c); the first c0
    pairs take the frame position, the next c1 the grid row, the last c1 the grid column."""
    c0, c1 = axis_split(hd)
    parts = []
    for pos, c in ((pf, c0), (ph, c1), (pw, c1)):
        inv = torch.pow(torch.tensor(THETA, dtype=torch.float64, device=pos.device),
                        -torch.arange(c, dtype=torch.float64, device=pos.device) / c)
        parts.append(pos.double().view(-1, 1) * inv.view(1, -1))
    return torch.cat(parts, 1)


def rope64(x, weight, H, grid, start_frame, row_offset=0, eps=EPS, angles=None):
    """RMSNorm over the full width, then the rotation of every head's pairs (a, b) = (y[2j], y[2j + 1]) by the angle of
    `rope_angles64`, all in fp64.  -> (ref, worst) [M, d]; the bar is

        even element:  |out - (a cos - b sin)| <= 2 u (2 (|a cos| + |b sin|) + |ref|)
        odd element:   |out - (a sin + b cos)| <= 2 u (2 (|a sin| + |b cos|) + |ref|).

    a and b carry the two roundings of the RMSNorm, 2 u each, which the rotation passes on weighted by |cos| and |sin|; the
    rotation is fp32 (contracted or not: 2^-23 of the same magnitudes) and the store rounds once, u |ref|.  The fp32 rounding
    of the (cos, sin) table is 2^-24 relative and sits in the margin with the 2^-19 of the norm (`rms64`)."""
    M, d = x.shape
    hd = d // H
    y, _ = rms64(x, weight, eps)
    if angles is None:
        angles = rope_angles64(hd, *token_positions(M, grid, start_frame, row_offset, x.device))
    cos, sin = torch.cos(angles).view(M, 1, hd // 2), torch.sin(angles).view(M, 1, hd // 2)
    y = y.view(M, H, hd // 2, 2)
    a, b = y[..., 0], y[..., 1]
    re, ro = a * cos - b * sin, a * sin + b * cos
    we = U * (2.0 * ((a * cos).abs() + (b * sin).abs()) + re.abs())
    wo = U * (2.0 * ((a * sin).abs() + (b * cos).abs()) + ro.abs())
    return torch.stack([re, ro], -1).view(M, d), torch.stack([we, wo], -1).view(M, d)


# ------------------------------------------------------------------------------------------------ builders
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def gaussian(M, d, seed=0, sigma=2.0):
    """Family 1 (sigma = 2), 6 (tiny: 1e-3, where var ~ eps, and 1e-10) and 7 (huge: 2^40, squares inside fp32): iid rows."""
    return (torch.randn(M, d, generator=_gen(100 + seed)) * sigma).to(BF16)


SPIKE = 64.0
SPIKE_NOISE = 2.0 ** -5


def spike(d, M=None, positive=False, seed=0):
    """Family 2.  Row i is noise of sigma 2^-5 (its magnitude in the positive variant) plus chunk i % (d / 8), whose elements
    are +-(64 + 4 j), j = 0 .. 7 (all + in the positive variant).  Promise: the chunk carries at least 90 % of the row's sum of
    squares and, in the positive variant, at least half of its sum.  M defaults to d / 8: every chunk index is hit once."""
    nch = d // 8
    M = nch if M is None else M
    x = torch.randn(M, d, generator=_gen(200 + seed)) * SPIKE_NOISE
    if positive:
        x = x.abs()
    sp = SPIKE + 4.0 * torch.arange(8.0)
    if not positive:
        sp = sp * torch.tensor([1.0, -1.0] * 4)
    xv = x.view(M, nch, 8)
    xv[torch.arange(M), torch.arange(M) % nch] = sp
    return x.to(BF16)


def offset(M, d, mean, seed=0):
    """Family 3.  mean + k * spacing, k uniform in -3 .. 3, spacing = the bf16 spacing above `mean` (0.5 at 64, 8 at 1024).
    Promise: exact in bf16; the spread is a 20th of the mean and less."""
    spacing = 2.0 ** (math.floor(math.log2(mean)) - 7)
    k = torch.randint(-3, 4, (M, d), generator=_gen(300 + seed)).float()
    return (mean + k * spacing).to(BF16)


def near_constant(M, d, seed=0):
    """Family 4.  Every element 1024 except one of 1032, at column (131 i + 7 seed) % d of row i.  The variance is 64 (d - 1) /
    d^2; a one-pass E[x^2] - mu^2 in fp32 (2^20 with a spacing of 0.125) cannot hold it."""
    x = torch.full((M, d), 1024.0)
    x[torch.arange(M), (131 * torch.arange(M) + 7 * seed) % d] = 1032.0
    return x.to(BF16)


CONSTANTS = [0.0, 1.0, -3.5, 1024.0, 2.0 ** -20, -(2.0 ** 30), 0.00390625]


def constant(M, d):
    """Family 5.  Row i holds CONSTANTS[i % 7] in every element; row 0 is the zero row.  Promise: exact in bf16.  The sums of a
    constant row are exact in fp32 (k * c, k <= 8192, needs 21 bits), the mean is c, and LayerNorm gives 0, b or sh_f bit for
    bit; RMSNorm and RoPE of the zero row give zeros."""
    c = torch.tensor([CONSTANTS[i % len(CONSTANTS)] for i in range(M)])
    return c.view(M, 1).expand(M, d).contiguous().to(BF16)


def mixed(M, d, seed=0):
    """Family 9.  Gaussian rows of sigma 2, row i scaled by 2^(i % 24 - 12) (exact): nothing may leak between rows."""
    x = torch.randn(M, d, generator=_gen(900 + seed)) * 2.0
    return (x.to(BF16).float() * torch.pow(2.0, (torch.arange(M) % 24 - 12).float()).view(M, 1)).to(BF16)


def frame_tables(F, d, J, seed=0):
    """Family 8.  A modulation table [F, J, d] as the kernel reads it at frame_stride = J d: [:, 0] the shifts, [:, 1] the
    scales.  Frame f's shift is 16 (f + 1) in every column and its scale 0.5 N(0, 1) + f / 2, so the neighbouring frame's row
    of the table is an error of 16, a hundred times the bar."""
    t = (torch.randn(F, J, d, generator=_gen(800 + seed)) * 0.5)
    t[:, 0] = 16.0 * (torch.arange(F).float().view(F, 1) + 1.0)
    t[:, 1] += 0.5 * torch.arange(F).float().view(F, 1)
    return t.to(BF16)


def gains(d, seed=0):
    """A norm weight 1 + 0.1 N(0, 1) and a bias 0.1 N(0, 1)."""
    g = _gen(700 + seed)
    return (1.0 + 0.1 * torch.randn(d, generator=g)).to(BF16), (0.1 * torch.randn(d, generator=g)).to(BF16)


def ln_families(d, M=17):
    """name -> rows [*, d] of every LayerNorm family at width d (the spike sweeps have d / 8 rows)."""
    fam = {"gaussian": gaussian(M, d, 1), "spike": spike(d), "spike_positive": spike(d, positive=True),
           "offset64": offset(M, d, 64.0), "offset1024": offset(M, d, 1024.0), "near_constant": near_constant(M, d),
           "constant": constant(M, d), "tiny1e-3": gaussian(M, d, 2, 1e-3), "tiny1e-10": gaussian(M, d, 3, 1e-10),
           "huge": gaussian(M, d, 4, 2.0 ** 40), "mixed": mixed(40, d)}
    return fam


def rms_families(d, M=17):
    """name -> rows of every RMSNorm / RoPE family at width d (offset and near-constant rows are LayerNorm's business)."""
    return {"gaussian": gaussian(M, d, 5), "spike": spike(d, seed=1), "constant": constant(M, d),
            "tiny1e-3": gaussian(M, d, 6, 1e-3), "tiny1e-10": gaussian(M, d, 7, 1e-10), "huge": gaussian(M, d, 8, 2.0 ** 40),
            "mixed": mixed(40, d, 1)}


def rope_families(d):
    """name -> rows of every RoPE family at width d; every row count is odd, so the wave form's last workgroup is partial."""
    return {"gaussian": gaussian(33, d, 9), "spike": spike(d, M=d // 8 + 1, seed=1), "constant": constant(17, d),
            "tiny1e-3": gaussian(17, d, 6, 1e-3), "tiny1e-10": gaussian(17, d, 7, 1e-10), "huge": gaussian(17, d, 8, 2.0 ** 40),
            "mixed": mixed(41, d, 1)}


def rope_qkv(x):
    """[M, 3 d]: the rows as q, the rows in reverse order as k, the rows as v."""
    return torch.cat([x, x.flip(0), x], 1)


LN_WIDTHS = [8, 256, 1536, 2048, 2056, 5120, 8184, 8192]     # one chunk ... the chunk loop's passes exactly full / one over / one short
FP8_WIDTHS = [256, 1536, 2048, 5120, 8192]                   # the fused quantiser takes multiples of 16
ROPE_SHAPES = [(128, 1), (256, 2), (1024, 8), (1536, 12), (1536, 8), (2048, 16), (5120, 40), (6144, 48), (8192, 64)]   # (d, heads)


# ------------------------------------------------------------------------------------------------ RoPE launch geometry
@dataclass
class RopeGeom:
    """One launch of the RoPE / cache kernel: M rows that are the tokens row_offset .. of an (F, gh, gw) grid, written to the
    logical cache rows cache_row0 + row_offset + r of a cache of `cache_rows` rows (through the ring, if any)."""
    M: int
    grid: tuple
    start_frame: int
    row_offset: int = 0
    cache_row0: int = 0
    cache_rows: int = 0
    ring: tuple = (0, 0, 0)

    def cache_row(self, r):
        lo, size, shift = self.ring
        row = self.cache_row0 + self.row_offset + r
        return lo + (row - lo + shift) % size if size > 0 and row >= lo else row

    def cache_index(self):
        return torch.tensor([self.cache_row(r) for r in range(self.M)], dtype=torch.long)


def rope_geom(M, row_offset=7, cache_row0=3, ring=False):
    """A token shard on a grid of 3 x 5 tokens per frame (gw no power of two) whose last frame position is 1023, the end of
    the table: rows row_offset .. row_offset + M of F = ceil((row_offset + M + 1) / 15) frames, so M < F gh gw and the rows
    include the last token of a grid row and of a frame.  ring: the rows from cache row 6 on live in a ring, shifted by 5."""
    F = (row_offset + M + 1 + 14) // 15
    last = cache_row0 + row_offset + M
    rg = (6, last - 6 + 2, 5) if ring else (0, 0, 0)
    return RopeGeom(M, (F, 3, 5), 1024 - F, row_offset, cache_row0, last + 4, rg)


# ------------------------------------------------------------------------------------------------ emulation (CPU test)
# a .. k: the errors these kernels are most likely to acquire.  l and m are here for the huge and the mixed-magnitude rows, which
# none of a .. k can tell from Gaussian rows: an overflow of the squares, and a statistic that leaks from the neighbouring row.
MUTANTS = {
    "a": "one chunk (the row's last) dropped from the reduction",
    "b": "one wave's partial (red[3], acc4[3]) dropped",
    "c": "one-pass variance E[x^2] - mean^2",
    "d0": "row_offset ignored in the frame index",
    "d1": "frame index of a frame's first row off by one",
    "e": "eps omitted",
    "f": "1 + scale replaced by scale",
    "g": "RoPE grid row and column swapped",
    "h": "RoPE column of the last token of a grid row off by one",
    "i": "the c0 axis boundary moved by one pair",
    "j": "the sign of sin flipped",
    "k": "row_offset ignored in the cache row",
    "l": "squares formed in fp16 (a packed-math rewrite)",
    "m": "rstd taken from the neighbouring row of the workgroup",
}


def _fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in fp64, the sum rounds to 53 bits and then to 24 (a double rounding that
    differs from the hardware in about one case in 2^29)."""
    return (a.double() * b.double() + c.double()).float()


def _layout(x32):
    """[M, d] -> [M, P, 256, 8]: element j of the chunk threadIdx.x + 256 i that thread `threadIdx.x` takes in pass i, zeros
    where the kernels' `c < nchunks` guard skips (adding 0 is exact); and the [P, 256] mask of the chunks that exist."""
    M, d = x32.shape
    nch = d // 8
    P = (nch + THREADS - 1) // THREADS
    v = torch.zeros(M, P * THREADS, 8, dtype=torch.float32)
    v[:, :nch] = x32.view(M, nch, 8)
    valid = (torch.arange(P * THREADS) < nch).view(P, THREADS)
    return v.view(M, P, THREADS, 8), valid


def _butterfly(s):
    """wave_sum: s[..., 64] -> every lane's total after the xor butterfly 32, 16, .. 1 (lane 0's is returned)."""
    idx = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ off]
    return s[..., 0]


def _block_sum(s, mutant):
    """block_sum: per-thread partials [M, 256] -> red[0] + red[1] + red[2] + red[3]."""
    w = _butterfly(s.view(-1, 4, 64))
    t = (w[:, 0] + w[:, 1]) + w[:, 2]
    return t if mutant == "b" else t + w[:, 3]


def _row_sum2(s, mutant):
    """The canonical order of both forms of the RoPE kernel: ((acc0 + acc1) + acc2) + acc3 per lane column, then the butterfly."""
    a = s.view(-1, 4, 64)
    t = (a[:, 0] + a[:, 1]) + a[:, 2]
    return _butterfly(t if mutant == "b" else t + a[:, 3])


def _thread_sums(v, valid, mutant, square=False, center=None):
    """Per-thread accumulation over the passes and the 8 elements of each chunk, in the kernels' order.  square: fused
    multiply-adds of (v - center)^2."""
    M, P = v.shape[:2]
    keep = valid.clone()
    if mutant == "a":
        last = int(valid.sum()) - 1
        keep[last // THREADS, last % THREADS] = False
    s = torch.zeros(M, THREADS, dtype=torch.float32)
    for i in range(P):
        k = keep[i].float().view(1, THREADS)
        for j in range(8):
            t = v[:, i, :, j]
            if center is not None:
                t = t - center
            t = t * k
            if not square:
                s = s + t
            elif mutant == "l":
                s = s + (t.half() * t.half()).float()
            else:
                s = _fma(t, t, s)
    return s


def _neighbour(r):
    idx = torch.arange(r.shape[0]) ^ 1
    return r[idx.clamp(max=r.shape[0] - 1)]


def _rsqrt(v, eps, mutant):
    r = torch.rsqrt(v if mutant == "e" else v + eps)
    return _neighbour(r) if mutant == "m" else r


def _r16(t):
    return t.to(BF16).float()


def emulate_ln(x, eps=EPS, weight=None, bias=None, shift=None, scale=None, rows_per_frame=0, row_offset=0, mutant=None):
    """layernorm_modulate_kernel in fp32 torch: the per-thread / per-wave partials of ln_row.h and its rounding points."""
    x32 = x.float()
    M, d = x32.shape
    v, valid = _layout(x32)
    mean = (_block_sum(_thread_sums(v, valid, mutant), mutant) / d).view(M, 1)
    if mutant == "c":
        var = _block_sum(_thread_sums(v, valid, mutant, square=True), mutant).view(M, 1) / d - mean * mean
    else:
        var = _block_sum(_thread_sums(v, valid, mutant, square=True, center=mean), mutant).view(M, 1) / d
    rstd = _rsqrt(var, eps, mutant)
    o = (x32 - mean) * rstd
    if weight is not None:
        o = o * weight.float() + bias.float()
    elif scale is not None:
        r = torch.arange(M)
        f = (r if mutant == "d0" else row_offset + r) // rows_per_frame
        if mutant == "d1":
            f = ((row_offset + r - 1).clamp(min=0)) // rows_per_frame
        a = scale.float()[f] if mutant == "f" else _r16(1.0 + scale.float()[f])
        o = _r16(_r16(o) * a) + shift.float()[f]
    return o.to(BF16)


def emulate_rms(x, weight, eps=EPS, mutant=None):
    """rmsnorm_kernel in fp32 torch."""
    x32 = x.float()
    M, d = x32.shape
    v, valid = _layout(x32)
    r = _rsqrt(_block_sum(_thread_sums(v, valid, mutant, square=True), mutant).view(M, 1) / d, eps, mutant)
    return (_r16(x32 * r) * weight.float()).to(BF16)


def emulate_rope(qkv, wq, wk, H, geom, table, k_cache, v_cache, eps=EPS, mutant=None):
    """Both forms of the RoPE / cache kernel in fp32 torch (they share the order of the sums): -> q [M, d]; the rows of
    k_cache / v_cache [rows, d] are written in place.  table: rope_cos_sin_table(hd), the project's fp32 (cos, sin) pairs."""
    M, d3 = qkv.shape
    d = d3 // 3
    hd = d // H
    half = hd // 2
    c0, c1 = axis_split(hd)
    if mutant == "i":
        c0 += 1
    pf, ph, pw = token_positions(M, geom.grid, geom.start_frame, geom.row_offset)
    if mutant == "g":
        ph, pw = pw, ph
    if mutant == "h":
        pw = torch.where(pw == geom.grid[2] - 1, pw - 1, pw)
    pj = torch.arange(half)
    pos = torch.where(pj.view(1, -1) < c0, pf.view(-1, 1), torch.where(pj.view(1, -1) < c0 + c1, ph.view(-1, 1), pw.view(-1, 1)))
    cs = table[pos, pj.view(1, -1).expand(M, -1)]                     # [M, half, 2]
    cos, sin = cs[..., 0].view(M, 1, half), cs[..., 1].view(M, 1, half)
    if mutant == "j":
        sin = -sin
    outs = []
    for x, w in ((qkv[:, :d], wq), (qkv[:, d:2 * d], wk)):
        x32 = x.float()
        v, valid = _layout(x32)
        r = _rsqrt(_row_sum2(_thread_sums(v, valid, mutant, square=True), mutant).view(M, 1) / d, eps, mutant)
        y = _r16(_r16(x32 * r) * w.float()).view(M, H, half, 2)
        a, b = y[..., 0], y[..., 1]
        outs.append(torch.stack([a * cos - b * sin, a * sin + b * cos], -1).view(M, d).to(BF16))
    rows = geom.cache_index()
    if mutant == "k":
        rows = rows - geom.row_offset
    k_cache[rows] = outs[1]
    v_cache[rows] = qkv[:, 2 * d:]
    return outs[0]
