"""Inputs, fp64 definitions, acceptance bars and CPU emulations of the five kernels of the text encoder
(realtime_video_amd/csrc/t5_encoder.hip): t5_attn_kernel, t5_rmsnorm_kernel<bool>, t5_geglu_kernel, t5_embed_kernel, t5_add_kernel,
reached through the unit entry points of include/rtv_hip_t5_units.h.

Plain torch, CPU or GPU tensors.  tests/test_t5_cases_cpu.py checks on the CPU what the builders promise, that an emulation of each
kernel's arithmetic passes its bar, and that named mutants of the emulations fail; tests/test_t5_kernels_gpu.py runs the HIP kernels
on the same inputs.

Why these inputs.  The end-to-end test (tests/test_text_encoder_gpu.py) feeds random tokens through random weights: every softmax
is diffuse, one key carries about 1 / L of a row, the relative-position bias is bucketed (bias[d +- 1] == bias[d] for most d) and a
final RMS norm follows - a key masked one position off, a V row from the wrong MFMA slot, an off-by-one in the table index or a head
stride of 2 * max_len all pass rel-L2 1e-2.  Here every answer hangs on one or two known keys, the table is arbitrary floats with
one spike per head, and the row kernels run at the widths where their loops repeat.

ATTENTION.  head_dim 64, no 1 / sqrt(d) scaling, rows % 32 == 0, any valid <= rows.  Reference and bar are those of the DiT attention
tests: attn_cases.attn_ref64(..., bias=..., scale=1.0) and attn_cases.within_bound, |out - ref| <= 4 u P|V| + 1e-6.  The derivation
there carries over because t5_attn_kernel has the same rounding points, checked against its source: scores are fp32 MFMA sums of
exact bf16 products plus an fp32 table entry, times log2(e); P = exp2f(s - m_run) in fp32 with m_run the running maximum itself
(reference point 0 below the maximum, inside the 2^8 the derivation allows); `ps += e0 + e1` sums the UNROUNDED fp32 exponentials
into l; pack_bf16x2 rounds P ONCE for the PV MFMA, which accumulates in fp32; alpha = exp2f(m_old - m_new) rescales l and O in
fp32; O * (1 / l) is rounded ONCE to bf16 by the store.  The reciprocal adds one fp32 rounding, inside the margin.

What the bar cannot see, by its own derivation: l taken from the ROUNDED P.  With w = P / l and P' = P (1 + d_k), |d_k| <= u,
sum w (1 + d) v / sum w (1 + d) differs from sum w v by at most (u P|V| + u |ref|) / (1 - u) <= 2 u P|V| (1 + u); with the store's u |ref|
that is 3 u P|V|, under the bar of 4.  The mutant is kept (INSIDE_THE_BAR) and the CPU test shows it stays inside: it is the one
named error these tests do not pin.

Contract on padding (rows in [valid, rows)): K there is never used - the kernel selects the score away, so NaN is harmless; V^T
columns there must be FINITE, because the PV product multiplies them by P = 0; as queries they give finite, otherwise unspecified
output and never index the table outside [0, 2 max_len - 2].

ROW KERNELS.  The bars follow row_cases.py: MARGIN = 2 times the worst case of the kernel's own rounding points (`rms64`,
`geglu64`); embed and add are exact.  What the bars do NOT pin: intermediate rounding points - a kernel that skipped one would be
closer to the fp64 definition, not further; the end-to-end test keeps that job, as row_cases.py notes for the DiT kernels.
"""
import math
from dataclasses import dataclass, replace

import torch

import attn_cases as ac
import row_cases as rc

HD = 64
LOG2E = 1.4426950408889634
BF16 = torch.bfloat16
U, U32, MARGIN = rc.U, rc.U32, rc.MARGIN
EPS = 1e-6
KB = 32                      # keys per step of t5_attn_kernel
SPIKE = 30.0                 # nats: the table entry of the bias one-hot family
DECOY_V = ac.DECOY_V


def roundup32(n):
    return (n + KB - 1) // KB * KB


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _gauss(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(BF16)


# ================================================================================================ attention
@dataclass
class AttnCase:
    """One launch of rtv_t5_attention.  q, k, v: [rows, H, 64] bf16 (k may hold NaN at rows >= valid); table: [H, 2 max_len - 1]
    float32, entry (key - query) + max_len - 1; targets: [valid, H, T] keys the answer of a query row hangs on, -1 where the builder
    promises nothing for that row (its reference is still the fp64 definition)."""
    name: str
    family: str
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    table: torch.Tensor
    valid: int
    max_len: int
    targets: torch.Tensor = None

    @property
    def rows(self):
        return self.q.shape[0]

    @property
    def H(self):
        return self.q.shape[1]

    def to(self, device):
        return replace(self, q=self.q.to(device), k=self.k.to(device), v=self.v.to(device), table=self.table.to(device))

    def qk(self):
        """[rows, 2 * 64 H]: q columns, then k columns, head h at column 64 h of each half."""
        return torch.cat([self.q.reshape(self.rows, -1), self.k.reshape(self.rows, -1)], 1).contiguous()

    def vt(self):
        """[64 H, rows]: V transposed."""
        return self.v.reshape(self.rows, -1).t().contiguous()

    def bias(self):
        """[1, H, valid, valid] float32: table[h, j - i + max_len - 1]."""
        i = torch.arange(self.valid, device=self.table.device)
        return self.table[:, i.view(1, -1) - i.view(-1, 1) + self.max_len - 1].unsqueeze(0)

    def reference(self):
        n = self.valid
        return ac.attn_ref64(self.q[None, :n], self.k[None, :n], self.v[None, :n], bias=self.bias(), scale=1.0)

    def within(self, out):
        """out [rows, H, 64] -> attn_cases.within_bound on the valid rows."""
        ref, ref_abs = self.reference()
        return ac.within_bound(out[None, :self.valid], ref, ref_abs, BF16)


def _unit_keys(n, H, seed):
    """[n, H, 64]: Gaussian directions of length 8, so k . k = 64 (up to the bf16 rounding) and k . k' is about N(0, 8^2): with
    q = k_t the target scores 64 nats and the best of 512 other keys about 45."""
    k = torch.randn(n, H, HD, generator=_gen(seed))
    return (k / k.norm(dim=-1, keepdim=True) * 8.0).to(BF16)


def _small_table(H, max_len, seed):
    """Arbitrary floats, sigma 0.25 nats: every distance of every head differs, and no lead moves by more than about 2 nats."""
    return torch.randn(H, 2 * max_len - 1, generator=_gen(seed)) * 0.25


def one_hot(valid, H, max_len, rows=None, seed=0, first_target=None):
    """Content one-hot: q_i = k_t with t = perm_h[i], a permutation per head, so every key is some query's target.
    first_target: row 0 of every head targets this key instead (swapped inside the permutation)."""
    rows = rows or roundup32(valid)
    k = _unit_keys(rows, H, 100 + seed)
    v = _gauss((rows, H, HD), 200 + seed)
    g = _gen(300 + seed)
    tg = torch.stack([torch.randperm(valid, generator=g) for _ in range(H)], 1)             # [valid, H]
    if first_target is not None:
        for h in range(H):
            pos = int((tg[:, h] == first_target).nonzero()[0])
            tg[pos, h], tg[0, h] = tg[0, h].clone(), first_target
    q = _gauss((rows, H, HD), 400 + seed, 0.25)
    q[:valid] = torch.gather(k[:valid], 0, tg.view(valid, H, 1).expand(-1, -1, HD))
    return AttnCase(f"one_hot[{valid}/{rows},H{H},L{max_len}]", "one_hot", q, k, v, _small_table(H, max_len, 500 + seed), valid, max_len,
                    tg.unsqueeze(-1))


def bias_one_hot(valid, H, max_len, dists, rows=None, seed=0):
    """q = 0; head h's table is zero except SPIKE at distance dists[h]: query i must return V[i + dists[h]] where that key exists
    (weight >= 1 - valid e^-30); where it does not, the row is the plain mean of the valid V rows."""
    rows = rows or roundup32(valid)
    q = torch.zeros(rows, H, HD, dtype=BF16)
    k = _gauss((rows, H, HD), 600 + seed)
    v = _gauss((rows, H, HD), 700 + seed)
    table = torch.zeros(H, 2 * max_len - 1)
    tg = torch.full((valid, H), -1, dtype=torch.long)
    for h, r in enumerate(dists):
        table[h, r + max_len - 1] = SPIKE
        t = torch.arange(valid) + r
        tg[:, h] = torch.where((t >= 0) & (t < valid), t, torch.full_like(t, -1))
    return AttnCase(f"bias_one_hot[{valid}/{rows},H{H},L{max_len},r{list(dists)}]", "bias_one_hot", q, k, v, table, valid, max_len,
                    tg.unsqueeze(-1))


def bias_sweep(valid, H, max_len):
    """bias_one_hot launches whose heads walk through every distance -(valid - 1) .. valid - 1 (the tail wraps to the front)."""
    dists = list(range(-(valid - 1), valid))
    for c in range((len(dists) + H - 1) // H):
        yield bias_one_hot(valid, H, max_len, [dists[(c * H + h) % len(dists)] for h in range(H)], seed=c)


def _hadamard64():
    h = torch.ones(1, 1)
    while h.shape[0] < HD:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def content_vs_bias(valid, H, max_len, rows=None, seed=0):
    """Two keys at weight 0.5 each, exactly: key j is row j % 64 of the Hadamard matrix of order 64 (+-1: k . k' is 64 or 0), query i
    is the row (i + ra_h) % 64, and the table is -40 except 0 at distance ra_h = h + 1 and 64 at distance rb_h = -(3 + 2 h).  Key
    a = i + ra scores 64 + 0 by content, key b = i + rb scores 0 + 64 by bias, the other keys congruent to a score 64 - 40 and
    everything else -40.  Rows for which a or b falls outside [0, valid) promise nothing."""
    rows = rows or roundup32(valid)
    had = _hadamard64()
    j = torch.arange(rows)
    k = had[j % HD].view(rows, 1, HD).expand(-1, H, -1).contiguous().to(BF16)
    v = _gauss((rows, H, HD), 800 + seed)
    q = torch.empty(rows, H, HD, dtype=BF16)
    table = torch.full((H, 2 * max_len - 1), -40.0)
    tg = torch.full((valid, H, 2), -1, dtype=torch.long)
    for h in range(H):
        ra, rb = h + 1, -(3 + 2 * h)
        q[:, h] = had[(j + ra) % HD].to(BF16)
        i = torch.arange(valid)
        both = (i + ra < valid) & (i + rb >= 0)
        tg[both, h, 0], tg[both, h, 1] = (i + ra)[both], (i + rb)[both]
        if ra <= max_len - 1:
            table[h, ra + max_len - 1] = 0.0
        if -rb <= max_len - 1:
            table[h, rb + max_len - 1] = 64.0
    return AttnCase(f"content_vs_bias[{valid}/{rows},H{H},L{max_len}]", "content_vs_bias", q, k, v, table, valid, max_len, tg)


def mask_edge(valid, H, max_len, rows=None, poison=False, seed=0):
    """one_hot whose row 0 targets key valid - 1 in every head, and whose padding keys valid .. rows - 1 would win if they were read:
    K = 1.5 x the K row of key valid - 1 (poison: NaN), the table holds SPIKE at every distance >= valid (distances only a padding key
    can have), and V = 100.  Needs rows > valid."""
    rows = rows or roundup32(valid)
    if rows <= valid:
        raise ValueError("mask_edge needs padding keys")
    c = one_hot(valid, H, max_len, rows, seed=900 + seed, first_target=valid - 1)
    c.k[valid:] = math.nan if poison else (c.k[valid - 1].float() * 1.5).to(BF16)
    c.v[valid:] = DECOY_V
    c.table[:, valid + max_len - 1:] = SPIKE
    kind = "poison" if poison else "decoy"
    return replace(c, name=f"mask_edge[{valid}/{rows},H{H},L{max_len},{kind}]", family="mask_edge")


def running_max(valid, H, max_len, late, rows=None, seed=0):
    """The target block (the last 32-key block: late; the first: early) holds unit keys kt; every other block b holds g_b kt, gains
    rising 0.25 -> 0.75 towards the target block (late) or falling away from it (early): scores of 16 .. 48 nats that lose to the
    target's 64 by 16.  Late, the running maximum grows in every block and the last block's alpha is about 2^-23."""
    rows = rows or roundup32(valid)
    nb = (valid + KB - 1) // KB
    if nb < 2:
        raise ValueError("running_max needs two key blocks")
    tb = nb - 1 if late else 0
    base = tb * KB
    nt = min(KB, valid - base)
    kt = _unit_keys(nt, H, 1000 + seed)
    k = _gauss((rows, H, HD), 1100 + seed, 0.1)
    others = [b for b in range(nb) if b != tb]
    for rank, b in enumerate(others if late else others[::-1]):
        gain = 0.25 + 0.5 * rank / max(1, len(others) - 1) if len(others) > 1 else 0.75
        n = min(KB, valid - b * KB)
        k[b * KB:b * KB + n] = (kt[torch.arange(n) % nt].float() * gain).to(BF16)
    k[base:base + nt] = kt
    v = _gauss((rows, H, HD), 1200 + seed)
    q = _gauss((rows, H, HD), 1300 + seed, 0.25)
    i = torch.arange(valid)
    q[:valid] = kt[i % nt]
    tg = (base + i % nt).view(valid, 1, 1).expand(-1, H, -1).clone()
    return AttnCase(f"running_max[{valid}/{rows},H{H},L{max_len},{'late' if late else 'early'}]", "running_max", q, k, v,
                    _small_table(H, max_len, 1400 + seed), valid, max_len, tg)


def bucketed_table(H, max_len, seed=0, num_buckets=32):
    """The table text_encoder.WanTextEncoder builds: an embedding [buckets, H] looked up at relative_position_bucket(key - query)."""
    from oracle.t5_oracle import relative_position_bucket
    emb = torch.randn(num_buckets, H, generator=_gen(1500 + seed)) * 0.5
    return emb[relative_position_bucket(torch.arange(-(max_len - 1), max_len), num_buckets)].t().contiguous()


def gaussian(valid, H, max_len, rows=None, seed=0):
    """Diffuse: q = 0.25 N(0, 1), k, v = N(0, 1), the bucketed table of the model."""
    rows = rows or roundup32(valid)
    q, k, v = _gauss((rows, H, HD), 1600 + seed, 0.25), _gauss((rows, H, HD), 1700 + seed), _gauss((rows, H, HD), 1800 + seed)
    return AttnCase(f"gaussian[{valid}/{rows},H{H},L{max_len}]", "gaussian", q, k, v, bucketed_table(H, max_len, seed), valid, max_len)


# (valid, H, max_len): every valid of {1, 31, 32, 33, 63, 64, 65, 300, 512} with max_len = rows and with 512, H from {1, 3, 4}
SHAPES = [(1, 1, 32), (1, 4, 512), (31, 3, 32), (31, 4, 512), (32, 4, 32), (32, 1, 512), (33, 4, 64), (33, 3, 512), (63, 4, 64), (63, 1, 512),
          (64, 1, 64), (64, 3, 512), (65, 4, 96), (65, 3, 512), (300, 4, 320), (300, 3, 512), (512, 4, 512), (512, 1, 512)]
MANY_HEADS = (64, 64, 64)                 # H = 64, the model's head count, once
FINDING = (48, 2, 48)                     # max_len no multiple of 32 and rows = 64 > max_len: the parent kernel's padding queries
#                                           read the table at indices down to -16
WIDE = (64, 3, 512, 128)                  # rows two blocks larger than needed: valid rows bit-identical with the tight launch
SWEEP_SHAPES = [(1, 1, 32), (31, 4, 32), (32, 3, 512), (33, 4, 64), (63, 3, 512), (64, 4, 64), (65, 4, 512), (300, 4, 320), (512, 4, 512),
                (48, 2, 48)]


def attention_cases():
    """Every launch of the GPU file but the distance sweep (`sweep_cases`)."""
    for valid, H, L in SHAPES + [MANY_HEADS, FINDING]:
        yield one_hot(valid, H, L, seed=valid + H)
        yield gaussian(valid, H, L, seed=valid + H)
        if valid >= 31 and H <= 16:           # rb_h - ra_h = -(4 + 3 h) is a multiple of 64 first at h = 20
            yield content_vs_bias(valid, H, L, seed=valid)
        if valid % KB:
            yield mask_edge(valid, H, L, seed=valid)
            yield mask_edge(valid, H, L, poison=True, seed=valid)
        if valid > KB:
            yield running_max(valid, H, L, True, seed=valid)
            yield running_max(valid, H, L, False, seed=valid)
    valid, H, L, rows = WIDE
    yield one_hot(valid, H, L, rows, seed=valid + H)
    yield mask_edge(valid, H, L, rows, seed=valid)
    yield mask_edge(valid, H, L, rows, poison=True, seed=valid)
    yield gaussian(valid, H, L, rows, seed=valid + H)


def sweep_cases(shapes=None):
    for valid, H, L in shapes or SWEEP_SHAPES:
        yield from bias_sweep(valid, H, L)


ATTN_MUTANTS = {
    "index+1": "table index one too far",
    "index-1": "table index one short",
    "sign": "query - key for key - query",
    "head_stride": "head stride 2 max_len for 2 max_len - 1",
    "mask_le": "mask key <= valid for key < valid",
    "no_alpha": "O and l not rescaled when the running maximum grows",
    "scale8": "content scores scaled by 1 / 8 = 1 / sqrt(head_dim)",
    "swap_regs": "P registers 4..7 and 8..11 of a lane swapped: keys 8..15 and 16..23 of a block meet each other's V rows",
}
INSIDE_THE_BAR = {"l_rounded": "l summed from the bf16-rounded P (3 u P|V| at worst: see the module docstring)"}


def emulate_attention(case, mutant=None):
    """t5_attn_kernel in fp32 torch, block of 32 keys by block: fp32 scores + table entry, times log2(e), select, running maximum,
    alpha, l from the unrounded exponentials, P rounded once to bf16 for P V, one rounding of O / l.  -> [rows, H, 64] bf16, padding
    query rows included.  A mutant's table reads that leave the table are clamped to its ends."""
    rows, H, valid, L = case.rows, case.H, case.valid, case.max_len
    q, k, v = case.q.float(), case.k.float(), case.v.float()
    s = torch.einsum("ihc,jhc->hij", q, k)                                         # column j depends on K row j alone
    if mutant == "scale8":
        s = s * 0.125
    i, j = torch.arange(rows).view(-1, 1), torch.arange(rows).view(1, -1)
    dist = j - i.clamp(max=valid - 1)
    if mutant == "sign":
        dist = -dist
    stride = 2 * L if mutant == "head_stride" else 2 * L - 1
    idx = torch.arange(H).view(-1, 1, 1) * stride + (L - 1) + dist + {"index+1": 1, "index-1": -1}.get(mutant, 0)
    flat = case.table.flatten()
    bias = flat[idx.clamp(0, flat.numel() - 1)]
    visible = (j <= valid) if mutant == "mask_le" else (j < valid)
    s = torch.where(visible, (s + bias) * LOG2E, torch.full_like(s, -math.inf))
    m = torch.full((H, rows), -math.inf)
    l = torch.zeros(H, rows)
    o = torch.zeros(H, rows, HD)
    for key0 in range(0, valid, KB):
        sb = s[..., key0:key0 + KB]
        m_new = torch.maximum(m, sb.amax(-1))
        alpha = torch.ones_like(m) if mutant == "no_alpha" else torch.exp2(m - m_new)
        m = m_new
        p = torch.exp2(sb - m.unsqueeze(-1))
        pb = p.to(BF16).float()
        l = l * alpha + (pb if mutant == "l_rounded" else p).sum(-1)
        if mutant == "swap_regs":
            pb = torch.cat([pb[..., :8], pb[..., 16:24], pb[..., 8:16], pb[..., 24:]], -1)
        o = o * alpha.unsqueeze(-1) + torch.einsum("hij,jhc->hic", pb, v[key0:key0 + KB])
    return (o * (1.0 / l).unsqueeze(-1)).permute(1, 0, 2).to(BF16)


# ================================================================================================ RMSNorm
RMS_WIDTHS = [64, 1024, 1088, 4096]       # under one 1024-element pass, exactly one, one and a bit, four
T5_THREADS = 256


def rms_depth(dim):
    """fp32 roundings on the longest path from an element to the row's sum of squares in t5_rmsnorm_kernel: per 1024-element pass a
    thread forms ((x0^2 + x1^2) + x2^2) + x3^2 - the square and three adds - and adds it to its partial: 5; the wave butterfly: 6;
    the chain 0 + red[0] + red[1] + red[2] + red[3]: 4.  (row_cases.sum_depth, for this kernel's structure.)"""
    return 5 * ((dim + 4 * T5_THREADS - 1) // (4 * T5_THREADS)) + 6 + 4


def rms64(x, w, eps=EPS, out_f32=False):
    """T5LayerNorm in fp64 on the fp32 row: ref = w x / sqrt(mean x^2 + eps).  -> (ref, worst), the bar is |out - ref| <= 2 worst,

        worst = (u_store + (c / 2 + 7) 2^-24) |ref|,   c = rms_depth(dim),   u_store = 2^-8 (bf16 output) or 0 (out_f32).

    The sum of squares has only positive terms, so it errs by at most c 2^-24 relative (Higham 4.2), halved by the square root; the
    division by dim and the + eps round once each (halved: 1 together); rsqrtf is good to 2 ulp = 4 * 2^-24; x * r and w * (x r) round
    once each: c / 2 + 1 + 4 + 2.  One bf16 rounding at the store, or none.  Where eps dominates the mean the relative error of the
    sum only matters less."""
    xd = x.double()
    ref = w.double() * xd / torch.sqrt((xd * xd).mean(-1, keepdim=True) + eps)
    rel = (0.0 if out_f32 else U) + (rms_depth(x.shape[-1]) / 2 + 7) * U32
    return ref, rel * ref.abs()


def rms_families(d):
    """name -> float32 rows [*, d]: row_cases' Gaussian, spike (every 8-element chunk of the row carries the sum once), constant,
    tiny, huge (sigma 2^41: squares and their sum stay inside fp32, as in the reference model) and mixed-magnitude rows, plus
    Gaussian rows that are not bf16-representable (the residual stream is float32)."""
    fam = {name: rows.float() for name, rows in rc.rms_families(d).items()}
    fam["gaussian_f32"] = torch.randn(17, d, generator=_gen(1900 + d)) * 2.0
    return fam


RMS_MUTANTS = {"pass": "only the first 1024-element pass enters the sum of squares", "wave": "one wave's partial (red[3]) dropped",
               "eps": "eps omitted"}


def emulate_rms(x, w, eps=EPS, out_f32=False, mutant=None):
    """t5_rmsnorm_kernel in fp32 torch: thread t takes elements 4 t .. 4 t + 3 of every 1024-element pass."""
    M, d = x.shape
    P = (d + 4 * T5_THREADS - 1) // (4 * T5_THREADS)
    xp = torch.zeros(M, P * 4 * T5_THREADS)
    xp[:, :d] = x
    sq = (xp * xp).view(M, P, T5_THREADS, 4)
    s = torch.zeros(M, T5_THREADS)
    for p in range(1 if mutant == "pass" else P):
        s = s + (((sq[:, p, :, 0] + sq[:, p, :, 1]) + sq[:, p, :, 2]) + sq[:, p, :, 3])
    wv = rc._butterfly(s.view(M, 4, 64))
    tot = (wv[:, 0] + wv[:, 1]) + wv[:, 2]
    if mutant != "wave":
        tot = tot + wv[:, 3]
    mean = (tot / d).view(M, 1)
    r = torch.rsqrt(mean if mutant == "eps" else mean + eps)
    out = w.float() * (x * r)
    return out if out_f32 else out.to(BF16)


# ================================================================================================ GEGLU
C0, C1 = 0.7978845608028654, 0.044715
GEGLU_SHAPES = [(13, 64), (3, 10240), (864, 10240)]     # 864 x 10240 / 8 > 4096 x 256: the grid-stride loop's second iteration


def geglu64(gf):
    """fc1 * gelu_tanh(gate) in fp64 on the bf16 inputs gf = [rows][gate (dff) | fc1 (dff)].  -> (ref, worst); the bar is
    |out - ref| <= 2 worst,

        worst = u |ref| + (4 + 10 |a|) 2^-24 |ref| + 2 * 2^-24 |f g tanh(a)|,    a = c0 (g + c1 g^3),  T = 1 + tanh(a).

    The kernel computes f * (0.5 g (1 + tanhf(c0 (g + c1 g g g)))) in fp32 and rounds once to bf16 (u |ref|).  a carries 5
    roundings, 5 * 2^-24 |a|, which tanh passes on as (1 - tanh^2) = T (2 - T) <= 2 T times that: 10 |a| 2^-24 relative to T.  The
    add 1 + tanh, 0.5 g T and f * (.) round once each and 0.5 g is exact: 3, taken as 4.  The ABSOLUTE term: tanhf is good to 2 ulp,
    4 * 2^-24 |tanh a| on the value of T; for negative g, T = 1 + tanh(a) cancels, so relative to T this grows as ulp(1) / T - the
    float32 reference has the same property - and it moves the output by 0.5 |f g| times it.  T itself is evaluated here as
    2 sigmoid(2 a), without the cancellation."""
    dff = gf.shape[1] // 2
    g, f = gf[:, :dff].double(), gf[:, dff:].double()
    a = C0 * (g + C1 * g ** 3)
    T = 2.0 * torch.sigmoid(2.0 * a)
    ref = f * 0.5 * g * T
    worst = U * ref.abs() + (4.0 + 10.0 * a.abs()) * U32 * ref.abs() + 2.0 * U32 * (f * g * (T - 1.0)).abs()
    return ref, worst


def gate_sweep():
    """bf16 gates: 769 steps over [-12, 12], +-0, tiny (2^-40, 1e-3) and the ends again."""
    extra = torch.tensor([0.0, -0.0, 2.0 ** -40, -(2.0 ** -40), 1e-3, -1e-3, 12.0, -12.0, 6.0, -6.0, 3.0, -3.0, 0.5, -0.5])
    return torch.cat([torch.linspace(-12.0, 12.0, 769), extra]).to(BF16)


def geglu_rows(rows, dff, seed=0):
    """gf [rows, 2 dff] bf16: the gates walk the sweep in element order (783 values: every shape here holds all of them); fc1 is N(0, 1) 2^e, e uniform in -20 .. 20, signs mixed."""
    sweep = gate_sweep()
    idx = (torch.arange(rows).view(-1, 1) * dff + torch.arange(dff).view(1, -1)) % sweep.numel()
    g = _gen(2000 + seed)
    f = torch.randn(rows, dff, generator=g) * torch.exp2(torch.randint(-20, 21, (rows, dff), generator=g).float())
    return torch.cat([sweep[idx], f.to(BF16)], 1).contiguous()


GEGLU_MUTANTS = {"erf": "the erf form of GELU for the tanh form", "coef": "0.044 for 0.044715", "swap": "gate and fc1 halves exchanged"}


def emulate_geglu(gf, mutant=None):
    dff = gf.shape[1] // 2
    g, f = gf[:, :dff].float(), gf[:, dff:].float()
    if mutant == "swap":
        g, f = f, g
    if mutant == "erf":
        ge = 0.5 * g * (1.0 + torch.erf(g * (1.0 / math.sqrt(2.0))))
    else:
        c1 = 0.044 if mutant == "coef" else C1
        ge = 0.5 * g * (1.0 + torch.tanh(C0 * (g + c1 * g * g * g)))
    return (f * ge).to(BF16)


# ================================================================================================ embed and add (exact)
EMBED_WIDTHS = [64, 1024, 1088, 4096]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def embed_case(dim, vocab=50, rows=64, valid=41, seed=0):
    """-> (ids int32 [valid], table bf16 [vocab, dim], expected float32 [rows, dim]).  ids: 0, vocab - 1, negatives and values >= vocab
    (the kernel clamps into the table), then random ones; rows >= valid are <pad>, table row 0."""
    g = _gen(2100 + seed + dim)
    table = torch.randn(vocab, dim, generator=g).to(BF16)
    ids = torch.randint(0, vocab, (valid,), generator=g)
    edge = torch.tensor([0, vocab - 1, -1, -7, vocab, vocab + 1000, INT_MAX, INT_MIN, 1, vocab - 2])
    ids[:edge.numel()] = edge
    want = torch.zeros(rows, dim)
    want[:valid] = table[ids.clamp(0, vocab - 1)].float()
    want[valid:] = table[0].float()
    return ids.to(torch.int32), table, want


ADD_SIZES = [8, 8 * 1000, 8 * (4096 * 256 + 4096 + 3)]          # the last: n / 8 > 4096 x 256, the loop's second iteration


def add_case(n, seed=0):
    """-> (x float32 [n], y bf16 [n], expected = the single fp32 addition x + float(y))."""
    g = _gen(2200 + seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-8, 9, (n,), generator=g).float())
    y = torch.randn(n, generator=g).to(BF16)
    return x, y, x + y.float()


# ================================================================================================ the encoder chain
def encoder_chain(w, ids, cfg, dtype=torch.float64, native=False, eps=EPS):
    """T5Encoder.forward on one prompt's tokens `ids` [n] (oracle.t5_oracle.encoder without the batch and the mask), in `dtype`.
    native=True emulates the rounding points of rtv_t5_encode: the input of every linear (the normed rows, the attention output, the
    gated hidden rows) and every linear's output that the native path stores as bf16 (q | k, V^T, the o and fc2 results, gate | fc1)
    are rounded to bf16; the residual stream, norms, softmax and gating stay in `dtype`.  -> [n, dim]."""
    from oracle import t5_oracle as to
    r = (lambda t: t.to(BF16).to(dtype)) if native else (lambda t: t)
    W = lambda name: w[name].to(dtype)
    norm = lambda x, g: g * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps))
    n, H = ids.numel(), cfg["num_heads"]
    x = W("token_embedding.weight")[ids]
    for i in range(cfg["num_layers"]):
        p = f"blocks.{i}"
        xn = r(norm(x, W(p + ".norm1.weight")))
        q, k, v = (r(xn @ W(f"{p}.attn.{m}.weight").t()).view(n, H, -1) for m in "qkv")
        bias = to.relative_bias(W(p + ".pos_embedding.embedding.weight"), n, n, cfg["num_buckets"])[0]
        pm = torch.softmax(torch.einsum("ihc,jhc->hij", q, k) + bias, -1)
        ao = r(torch.einsum("hij,jhc->ihc", pm, v).reshape(n, -1))
        x = x + r(ao @ W(p + ".attn.o.weight").t())
        xn = r(norm(x, W(p + ".norm2.weight")))
        g, f = r(xn @ W(p + ".ffn.gate.0.weight").t()), r(xn @ W(p + ".ffn.fc1.weight").t())
        h = r(f * (0.5 * g * (1.0 + torch.tanh(C0 * (g + C1 * g ** 3)))))
        x = x + r(h @ W(p + ".ffn.fc2.weight").t())
    return norm(x, W("norm.weight"))


def bf16_checkpoint(w):
    """The state dict as the released checkpoint holds it: every tensor bf16-representable.  oracle.t5_oracle.make_t5_weights forms
    its norm weights as 1 + bf16(0.1 N(0, 1)), which is not; the native encoder keeps bf16 weights, so without this a per-element
    bar would measure the rounding of the test's own weights."""
    return {k: v.to(BF16).float() for k, v in w.items()}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


DEEP_T5 = dict(num_layers=24)             # on top of oracle.t5_oracle.TINY_T5: the model's depth at tiny width
DEEP_LENS = (33, 64)
DEEP_TEXT_LEN = 64
