"""Peaked attention inputs, the fp64 definition and the acceptance bound of the attention tests.

Plain torch, CPU or GPU tensors.  tests/test_attention_cases_cpu.py checks on the CPU what the builders promise (a lead of the
target key of at least 12 nats, a weight of at least 1 - 1e-5, no score beyond 80 nats) and that an emulation of the kernels'
arithmetic passes `within_bound` while mutants of it fail; tests/test_attention_peaked_gpu.py runs the HIP kernels on the
same inputs.

Why peaked inputs: on iid Gaussian q / k / v the softmax is diffuse, one key carries a weight of about 1 / Lkv and a row read
from the wrong place moves the output by 1e-3.  Here every query's answer hangs on one or two known keys, so a single wrong key
is an O(1) error.
"""
import math
from dataclasses import dataclass, field, replace

import torch

D = 128
SCALE = 1.0 / math.sqrt(D)
KT = 64                      # keys per tile of every attention kernel
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BOUND_FACTOR = 4.0
DECOY_V = 100.0
CAUSAL_DECOY_V = 16.0        # decoys that other rows see as ordinary keys (spec_causal)


# ------------------------------------------------------------------------------------------------ reference and bound
def scores64(q, k, scale=SCALE, mask=None, bias=None):
    """scale * q k^T + bias in float64 and in nats, [B, H, Lq, Lkv]; masked-out entries are -inf.  mask: True = visible."""
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    if bias is not None:
        s = s + bias.double()
    if mask is not None:
        s = s.masked_fill(~mask, -math.inf)
    return s


def attn_ref64(q, k, v, mask=None, bias=None, scale=SCALE):
    """The fp64 definition on the 16-bit tensors the kernel receives, upcast.  q [B, Lq, H, D], k / v [B, Lkv, H, D]; mask (True =
    visible) and bias (nats) broadcast against [B, H, Lq, Lkv].  -> (ref, ref_abs) = (P @ V, P @ |V|), both [B, Lq, H, D] float64,
    with P = softmax(scale q k^T + bias) over the visible keys."""
    p = torch.softmax(scores64(q, k, scale, mask, bias), dim=-1)
    vd = v.double()
    return torch.einsum("bhqk,bkhd->bqhd", p, vd), torch.einsum("bhqk,bkhd->bqhd", p, vd.abs())


def within_bound(out, ref, ref_abs, dtype):
    """The one acceptance rule:  |out - ref| <= 4 u ref_abs + 1e-6  elementwise, u = the unit roundoff of `dtype`
    (2^-8 bf16, 2^-11 f16).

    Derivation.  The kernels form P = exp2(s - m) in fp32 with a reference point m at most 2^8 below the row maximum, round P
    ONCE to the 16-bit type for the PV product (relative error <= u per key, whatever m is: rounding is relative), accumulate
    P V in fp32, take the row sum l from the UNROUNDED fp32 exponentials, and round O / l ONCE to the 16-bit type.  The rounding
    of P moves an output element by at most u * sum_k P_k |V_kd| / l = u * ref_abs, the rounding of the output by at most
    u * |ref| <= u * ref_abs: 2 u ref_abs in the worst case.  The factor 4 leaves a twofold margin for v_exp_f32 (about 1 ulp
    of fp32 on an argument whose own fp32 rounding error is up to 2^-24 * 80 * log2(e) ~ 7e-6 relative) and the fp32 sums
    (Lkv * 2^-24 at worst), all far below u.  The KV split adds only fp32 operations (partials and their merge are fp32).
    1e-6 is the absolute floor for elements whose ref_abs is 0 (f16 subnormal P of far-away keys).

    -> (ok, ratio, index): ratio = the largest |out - ref| / (u ref_abs + 2.5e-7) - so ok means ratio <= 4 - and index =
    (batch, query row, head, dim) of the element that has it.  A non-finite output element counts as an infinite ratio."""
    u = UNIT_ROUNDOFF[dtype]
    err = (out.double() - ref).abs()
    ok = bool((err <= BOUND_FACTOR * u * ref_abs + 1e-6).all())
    ratio = torch.nan_to_num(err / (u * ref_abs + 2.5e-7), nan=math.inf, posinf=math.inf)
    flat = int(ratio.argmax())
    idx = []
    for n in reversed(ratio.shape):
        idx.append(flat % n)
        flat //= n
    return ok, float(ratio.max()), tuple(reversed(idx))


# ------------------------------------------------------------------------------------------------ builders
@dataclass
class Case:
    """q [B, Lq, H, D], k / v [B, Lkv, H, D] in the 16-bit dtype (CPU tensors; .to(device) moves them) and targets [Lq, H, T]: the
    key or keys of the window that the answer of a query row hangs on (the same in every batch element)."""
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    targets: torch.Tensor
    notes: dict = field(default_factory=dict)

    def to(self, device):
        return Case(self.q.to(device), self.k.to(device), self.v.to(device), self.targets, self.notes)

    def target_of(self, row, head):
        return [int(t) for t in self.targets[row, head]]


def _gauss(shape, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _gather_keys(k, targets):
    """k [B, Lkv, H, D], targets [Lq, H] -> k[b, targets[i, h], h] as [B, Lq, H, D]."""
    B, _, H, Dk = k.shape
    idx = targets.view(1, -1, H, 1).expand(B, -1, -1, Dk)
    return torch.gather(k, 1, idx)


def one_hot(Lq, Lkv, H=2, B=1, dtype=torch.bfloat16, perm_seed=0, offset=0, cover=(), targets=None):
    """K and V are N(0, 1); q[b, i, h] = 4 * k[b, t, h] with t = perm_h[(i + offset) % Lkv], a permutation per head (4 is exact
    in bf16 and f16).  With Lq >= Lkv every key position is some query's target; with Lq < Lkv `cover` names key positions that
    are moved to the front of every head's permutation, and `offset` walks a short launch through the rest.  `targets`
    ([Lq, H] key positions) replaces the permutation, e.g. by each row's last key under a block-causal mask."""
    k = _gauss((B, Lkv, H, D), 1000 + perm_seed, dtype)
    v = _gauss((B, Lkv, H, D), 2000 + perm_seed, dtype)
    if targets is None:
        g = torch.Generator(device="cpu").manual_seed(3000 + perm_seed)
        cols = []
        for _ in range(H):
            perm = torch.randperm(Lkv, generator=g)
            if len(cover):
                front = torch.tensor([c for c in dict.fromkeys(int(c) for c in cover) if 0 <= c < Lkv], dtype=torch.long)
                keep = torch.ones(Lkv, dtype=torch.bool)
                keep[front] = False
                perm = torch.cat([front, perm[keep[perm]]])
            cols.append(perm[(torch.arange(Lq) + offset) % Lkv])
        targets = torch.stack(cols, 1)
    targets = targets.long()
    q = (_gather_keys(k.float(), targets) * 4.0).to(dtype)
    return Case(q, k, v, targets.unsqueeze(-1).clone())


def staircase(Lq, Lkv, H=2, B=1, dtype=torch.bfloat16, seed=0):
    """Each query matches one key in each of four tiles - the first, two middle ones and the last, ragged one - with gains 1, 2,
    3 and 4: q is the combination of the four keys (a 4 x 4 Gram system solved in fp64) whose scaled scores against them are
    16, 32, 48 and 64 nats, exactly up to the 16-bit rounding of q.  Odd rows take the gains in descending order.  The running
    maximum of a row therefore grows by 16 nats = 23 in the log2 domain - more than the 2^8 of the kernels' lazy rescale - at
    each step of an even row (late), and once, in the first tile, in an odd row (early).  The answer hangs on the gain-4 key,
    which leads the gain-3 key by 16 nats; targets[..., 0] is that key, [..., 1:] the other three by falling gain."""
    ntiles = (Lkv + KT - 1) // KT
    if ntiles < 4:
        raise ValueError("staircase needs at least four key tiles")
    k = _gauss((B, Lkv, H, D), 4000 + seed, dtype)
    v = _gauss((B, Lkv, H, D), 5000 + seed, dtype)
    g = torch.Generator(device="cpu").manual_seed(6000 + seed)
    last0 = (ntiles - 1) * KT
    mids = torch.stack([torch.randperm(ntiles - 2, generator=g)[:2].sort().values + 1 for _ in range(Lq * H)]).view(Lq, H, 2)
    within = torch.randint(0, KT, (Lq, H, 4), generator=g)
    tiles = torch.cat([torch.zeros(Lq, H, 1, dtype=torch.long), mids, torch.full((Lq, H, 1), ntiles - 1)], -1)
    keys = tiles * KT + within
    keys[..., 3] = last0 + within[..., 3] % (Lkv - last0)                 # inside the ragged tile
    gains = torch.tensor([1.0, 2.0, 3.0, 4.0]).expand(Lq, H, 4).clone()
    gains[1::2] = gains[1::2].flip(-1)
    kk = torch.stack([_gather_keys(k.double(), keys[..., j]) for j in range(4)], 3)       # [B, Lq, H, 4, D]
    gram = kk @ kk.transpose(-1, -2) * SCALE
    coef = torch.linalg.solve(gram, (16.0 * gains).double().unsqueeze(0).unsqueeze(-1).expand(B, -1, -1, -1, -1))
    q = (coef.transpose(-1, -2) @ kk).squeeze(3).to(dtype)
    order = gains.argsort(-1, descending=True)
    return Case(q, k, v, torch.gather(keys, 2, order), {"gains": gains})


def tie(Lq, Lkv, groups, H=2, B=1, dtype=torch.bfloat16, seed=0):
    """groups: tuples of key positions.  The K rows of a group are bit-identical copies of its first row, the V rows stay
    different, and query i matches group i % len(groups) (q = 4 k): its softmax gives each key of the group the same weight and
    everything else nothing, so the reference is the mean of the group's V rows."""
    k = _gauss((B, Lkv, H, D), 7000 + seed, dtype)
    v = _gauss((B, Lkv, H, D), 8000 + seed, dtype)
    width = max(len(gr) for gr in groups)
    if any(len(gr) != width for gr in groups):
        raise ValueError("tie: groups of one size")
    for gr in groups:
        for pos in gr[1:]:
            k[:, pos] = k[:, gr[0]]
    tg = torch.tensor([list(groups[i % len(groups)]) for i in range(Lq)], dtype=torch.long)      # [Lq, T]
    targets = tg.unsqueeze(1).expand(-1, H, -1).clone()
    q = (_gather_keys(k.float(), targets[..., 0]) * 4.0).to(dtype)
    return Case(q, k, v, targets)


def decoys(k_cache, v_cache, rows, k_window, match, poison=False, value=DECOY_V):
    """Rows of a cache that lie OUTSIDE the key window and would win the softmax if they were ever read: K row rows[j] becomes
    1.5 * k_window[:, match[j]] - ahead of the real key `match[j]` for every query that targets it, by half its score - and the V
    row a row of `value` (100).  poison=True writes +Inf into the K rows and NaN into the V rows instead.  In place; rows outside the
    cache are skipped.  -> [(cache row, matched key)] of the rows written."""
    done = []
    for row, t in zip(rows, match):
        if not 0 <= row < k_cache.shape[1]:
            continue
        if poison:
            k_cache[:, row] = math.inf
            v_cache[:, row] = math.nan
        else:
            k_cache[:, row] = (k_window[:, t].float() * 1.5).to(k_cache.dtype)
            v_cache[:, row] = value
        done.append((row, int(t)))
    return done


def causal_limits(Lq, Lkv, causal_block, q_offset):
    """Block-causal rule of the kernels: query row r sees the keys kv < lim[r] = min(Lkv, ((q_offset + r) // block + 1) * block)."""
    r = torch.arange(Lq)
    return torch.clamp(((q_offset + r) // causal_block + 1) * causal_block, max=Lkv)


def causal_mask(Lq, Lkv, causal_block, q_offset, device="cpu"):
    lim = causal_limits(Lq, Lkv, causal_block, q_offset).to(device)
    return (torch.arange(Lkv, device=device).view(1, -1) < lim.view(-1, 1)).view(1, 1, Lq, Lkv)


# ------------------------------------------------------------------------------------------------ emulation (CPU test)
def emulate_partial(q, k, v, dtype, mask=None, bias=None, slack=8.0, bias_log2=None):
    """One key range in the kernels' arithmetic: fp32 scores in the log2 domain, a reference point m = row maximum - slack
    (RESCALE_SLACK allows up to 8), P = exp2(s - m) in fp32, the row sum l from the unrounded P, P rounded once to `dtype`
    for P V in fp32.  -> (m [B, H, Lq], l [B, H, Lq], O unnormalised [B, Lq, H, D]), all fp32.  A row with no visible key in the
    range leaves (-1e30, 0, 0) as the kernels do.  bias in nats (bias_log2: already in the log2 domain, for the log mutant)."""
    c = SCALE * 1.4426950408889634
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float())
    if bias is not None:
        s = s + (bias.float() / SCALE)                     # the kernels add log2(count) / scale_log2e before the scale
    s = s * c
    if bias_log2 is not None:
        s = s + bias_log2.float()
    if mask is not None:
        s = s.masked_fill(~mask, -math.inf)
    mx = s.amax(-1)
    m = torch.where(torch.isinf(mx), torch.full_like(mx, -1e30), mx - slack)
    p = torch.exp2(s - m.unsqueeze(-1))
    l = p.sum(-1)
    o = torch.einsum("bhqk,bkhd->bqhd", p.to(dtype).float(), v.float())
    return m, l, o


def emulate(q, k, v, dtype, mask=None, bias=None, slack=8.0, ranges=None, swap_maxima=None, bias_log2=None):
    """The whole launch: one range, or the KV split over `ranges` = [(lo, hi), ...] with the combine kernel's merge
    m = max m_s, w_s = 2^(m_s - m), O = sum w_s O_s / sum w_s l_s.  swap_maxima = (a, b): the mutant that weights ranges a and b
    with each other's maximum."""
    Lkv = k.shape[1]
    parts = []
    for lo, hi in (ranges or [(0, Lkv)]):
        mk = None if mask is None else mask.expand(-1, -1, q.shape[1], Lkv)[..., lo:hi]
        bs = None if bias is None else bias.expand(-1, -1, -1, Lkv)[..., lo:hi]
        b2 = None if bias_log2 is None else bias_log2.expand(-1, -1, -1, Lkv)[..., lo:hi]
        parts.append(emulate_partial(q, k[:, lo:hi], v[:, lo:hi], dtype, mk, bs, slack, b2))
    ms = torch.stack([p[0] for p in parts])
    m = ms.amax(0)
    if swap_maxima is not None:
        a, b = swap_maxima
        ms = ms.clone()
        ms[[a, b]] = ms[[b, a]]
    w = torch.exp2(ms - m)
    l = sum(w[i] * parts[i][1] for i in range(len(parts)))
    o = sum(w[i].permute(0, 2, 1).unsqueeze(-1) * parts[i][2] for i in range(len(parts)))
    return (o / l.permute(0, 2, 1).unsqueeze(-1)).to(dtype)


# ------------------------------------------------------------------------------------------------ the cases of the GPU file
# One Spec = one launch configuration of tests/test_attention_peaked_gpu.py: built here, on the CPU, so that
# tests/test_attention_cases_cpu.py checks the builder promises and the emulation on exactly the inputs the kernels get.
@dataclass
class Spec:
    name: str
    q: torch.Tensor                       # [B, Lq, H, D]
    k_base: torch.Tensor                  # the allocation that holds the K cache (an arena may hold V as well)
    v_base: torch.Tensor
    seg0: tuple                           # (first cache row, rows) of the key window's first range
    seg1: tuple = (0, 0)                  # ... and of its second range (n1 = 0: one range)
    targets: torch.Tensor = None          # [Lq, H, T] keys of the WINDOW the answers hang on
    interleaved: bool = False             # k_base is v_base = an arena [B, rows, 2, H, D]: K = [:, :, 0], V = [:, :, 1]
    causal_block: int = 0
    q_offset: int = 0
    dup_key: int = -1
    dup_count: int = 1
    decoy_rows: list = field(default_factory=list)
    answer: int = 0                       # how many leading columns of `targets` carry the answer (0: all of them)

    def to(self, device):
        kb = self.k_base.to(device)
        vb = kb if self.interleaved else self.v_base.to(device)
        return replace(self, q=self.q.to(device), k_base=kb, v_base=vb)

    @property
    def dtype(self):
        return self.q.dtype

    @property
    def Lkv(self):
        return self.seg0[1] + self.seg1[1]

    def caches(self):
        """(k_cache, v_cache) [B, rows, H, D]: strided views when the allocation is an interleaved arena."""
        if self.interleaved:
            return self.k_base[:, :, 0], self.k_base[:, :, 1]
        return self.k_base, self.v_base

    def window(self):
        """(k, v) of the key window as the reference sees it: the rows of the two ranges, concatenated."""
        (r0, n0), (r1, n1) = self.seg0, self.seg1
        kc, vc = self.caches()
        if n1 == 0:
            return kc[:, r0:r0 + n0], vc[:, r0:r0 + n0]
        return torch.cat([kc[:, r0:r0 + n0], kc[:, r1:r1 + n1]], 1), torch.cat([vc[:, r0:r0 + n0], vc[:, r1:r1 + n1]], 1)

    def mask(self, device="cpu"):
        if self.causal_block <= 0:
            return None
        return causal_mask(self.q.shape[1], self.Lkv, self.causal_block, self.q_offset, device)

    def bias(self, device="cpu"):
        if self.dup_key < 0:
            return None
        b = torch.zeros(1, 1, 1, self.Lkv, dtype=torch.float64, device=device)
        b[..., self.dup_key] = math.log(self.dup_count)
        return b

    def reference(self, device="cpu"):
        k, v = self.window()
        return attn_ref64(self.q, k, v, self.mask(device), self.bias(device))


def _cache_around(case, r0, tail):
    """A cache of r0 + Lkv + tail rows that holds the window of `case` at rows [r0, r0 + Lkv) and zeros elsewhere."""
    B, Lkv, H, _ = case.k.shape
    kc = torch.zeros(B, r0 + Lkv + tail, H, D, dtype=case.k.dtype)
    vc = torch.zeros_like(kc)
    kc[:, r0:r0 + Lkv] = case.k
    vc[:, r0:r0 + Lkv] = case.v
    return kc, vc


def spec_every_key(Lq, Lkv, dtype=torch.bfloat16, B=1, offset=0, H=2):
    """Family a: one_hot, dense; K and V are the two planes of an interleaved arena [B, rows, 2, H, D], the window starts at row 5."""
    case = one_hot(Lq, Lkv, H, B, dtype, perm_seed=Lkv, offset=offset)
    arena = torch.zeros(B, 5 + Lkv + 3, 2, H, D, dtype=dtype)
    arena[:, 5:5 + Lkv, 0] = case.k
    arena[:, 5:5 + Lkv, 1] = case.v
    return Spec(f"every_key[{Lq}x{Lkv},B{B},off{offset}]", case.q, arena, arena, (5, Lkv), targets=case.targets, interleaved=True)


def spec_causal(Lq, Lkv, causal_block, q_offset, dtype=torch.bfloat16, far=False, H=2):
    """Family b: every query's target is its last allowed key lim - 1 (far=True: the far end of its own key block instead -
    key 0 for the rows of the first block, lim - block + 1 for the others) and key `lim`, where lim < Lkv, is a decoy for exactly
    these rows: 1.5 x their target's K row, V = 16.  Rows with a larger limit see that decoy as an ordinary key, which it is for
    them: it matches another group's target, not theirs, and the reference counts it.  16 and not 100 because of those rows:
    an f16 P below 2^-14 of the row's reference point is subnormal, with an ABSOLUTE error of up to 2^-25, and 100 x 2^-25 is
    above the 1e-6 floor of `within_bound` (16 x 2^-25 = 4.8e-7 is not).  16 is still 11 away from any N(0, 1) answer."""
    lim = causal_limits(Lq, Lkv, causal_block, q_offset)
    if far:
        tgt = torch.where(lim - causal_block <= 0, torch.zeros_like(lim), lim - causal_block + 1)
        tgt = torch.minimum(tgt, lim - 1)
    else:
        tgt = lim - 1
    case = one_hot(Lq, Lkv, H, 1, dtype, perm_seed=causal_block + q_offset, targets=tgt.view(-1, 1).expand(-1, H))
    pairs = sorted({(int(l), int(t)) for l, t in zip(lim, tgt) if l < Lkv})
    taken = {int(t) for t in tgt}
    assert not any(l in taken for l, _ in pairs), "a decoy would overwrite a target key"
    rows = decoys(case.k, case.v, [l for l, _ in pairs], case.k.clone(), [t for _, t in pairs], value=CAUSAL_DECOY_V)
    return Spec(f"causal[{Lq}x{Lkv},cb{causal_block},off{q_offset},{'far' if far else 'last'}]", case.q, case.k, case.v, (0, Lkv),
                targets=case.targets, causal_block=causal_block, q_offset=q_offset, decoy_rows=rows)


def spec_outside(Lq, Lkv, dtype=torch.bfloat16, poison=False, H=2):
    """Family c: the window is rows [3, 3 + Lkv) of a cache; row 2 and the 64 rows behind the window hold decoys (poison: +Inf in
    K, NaN in V) matched to key 0 and to the last 64 keys, which `cover` makes targets of some query."""
    r0 = 3
    match = [0] + [(Lkv - 1 - j) % Lkv for j in range(KT)]
    case = one_hot(Lq, Lkv, H, 1, dtype, perm_seed=100 + Lkv, cover=match)
    kc, vc = _cache_around(case, r0, KT + 8)
    rows = decoys(kc, vc, [r0 - 1] + [r0 + Lkv + j for j in range(KT)], case.k, match, poison)
    return Spec(f"outside[{Lq}x{Lkv},{'poison' if poison else 'decoy'}]", case.q, kc, vc, (r0, Lkv), targets=case.targets,
                decoy_rows=rows)


TWO_RANGE_WINDOWS = [((64, 64), (0, 64)), ((3, 77), (200, 1003)), ((1000, 1), (10, 130)), ((600, 500), (2, 300)), ((5, 200), (0, 0))]


def spec_two_ranges(seg0, seg1, Lq=300, dtype=torch.bfloat16, H=2):
    """Family d: one_hot over the concatenated window; the cache rows next to each end of each range (those that are not
    themselves part of the window) hold decoys matched to the key at that end."""
    (r0, n0), (r1, n1) = seg0, seg1
    Lkv = n0 + n1
    ends = [(r0 - 1, 0), (r0 + n0, n0 - 1)] + ([(r1 - 1, n0), (r1 + n1, Lkv - 1)] if n1 else [])
    inside = lambda r: r0 <= r < r0 + n0 or (n1 and r1 <= r < r1 + n1)
    ends = [(r, t) for r, t in ends if not inside(r)]
    case = one_hot(Lq, Lkv, H, 1, dtype, perm_seed=200 + Lkv, cover=[0, n0 - 1, min(n0, Lkv - 1), Lkv - 1])
    rows_total = max(r0 + n0, r1 + n1) + KT + 8
    kc = torch.zeros(1, rows_total, H, D, dtype=dtype)
    vc = torch.zeros_like(kc)
    kc[:, r0:r0 + n0], vc[:, r0:r0 + n0] = case.k[:, :n0], case.v[:, :n0]
    if n1:
        kc[:, r1:r1 + n1], vc[:, r1:r1 + n1] = case.k[:, n0:], case.v[:, n0:]
    rows = decoys(kc, vc, [r for r, _ in ends], case.k, [t for _, t in ends])
    return Spec(f"two_ranges[{r0}+{n0},{r1}+{n1}]", case.q, kc, vc, seg0, seg1, targets=case.targets, decoy_rows=rows)


def spec_counted(kind, n_real, dup_key, count, Lq=257, dtype=torch.bfloat16, H=2):
    """Family e: a window of n_real keys plus one key, at position dup_key, that stands for `count` identical ones.
    kind "tie":     the counted key and a real key half a window away are bit-identical K rows; the answer is
                    (v_a + count v_dup) / (count + 1).
    kind "onto":    one_hot whose even rows target the counted key.
    kind "beside":  one_hot whose even rows target a real key t0 while the counted key holds 0.9 x that key's K row: its score
                    is about 4.5 nats below the target's, + log(count); the answer hangs on both and on the bias being applied
                    to that column once, at its size."""
    Lkv = n_real + 1
    a = (dup_key + max(1, Lkv // 2)) % Lkv
    if kind == "tie":
        case = tie(Lq, Lkv, [(dup_key, a)], H, 1, dtype, seed=n_real + dup_key)
    else:
        seed = 300 + n_real + dup_key
        tg = one_hot(Lq, Lkv, H, 1, dtype, perm_seed=seed).targets[..., 0]
        if kind == "beside":                                     # the counted key is nobody's sole target here
            tg[1::2] = torch.where(tg[1::2] == dup_key, torch.full_like(tg[1::2], a), tg[1::2])
        tg[0::2] = dup_key if kind == "onto" else a
        case = one_hot(Lq, Lkv, H, 1, dtype, perm_seed=seed, targets=tg)       # the same K and V, the new targets
        if kind == "beside":
            case.k[:, dup_key] = (case.k[:, a].float() * 0.9).to(dtype)
            case.targets = torch.stack([tg, torch.full_like(tg, dup_key)], -1)
    return Spec(f"counted[{kind},n_real{n_real},key{dup_key},x{count}]", case.q, case.k, case.v, (0, Lkv), targets=case.targets,
                dup_key=dup_key, dup_count=count)


def split_ranges(Lkv, splits):
    """Key ranges of the KV split as the kernels cut them: tiles [ntiles s / S, ntiles (s + 1) / S), never more ranges than tiles."""
    nt = (Lkv + KT - 1) // KT
    S = max(1, min(splits, nt))
    return [(nt * s // S * KT, min(Lkv, nt * (s + 1) // S * KT)) for s in range(S)]


def spec_split(kind, Lkv, splits, Lq=300, dtype=torch.bfloat16, H=2):
    """Family f.  "one_hot": targets spread over all ranges (per row one range's maximum is about 40 log2 units above the others:
    the 2^(m_s - m) underflow side of the merge).  "tie2" / "tie3": bit-identical keys in two / three different ranges (equal
    maxima: equal weights).  "staircase": as family g."""
    if kind == "one_hot":
        case = one_hot(Lq, Lkv, H, 1, dtype, perm_seed=400 + Lkv, cover=[e for lo, hi in split_ranges(Lkv, splits) for e in (lo, hi - 1)])
    elif kind == "staircase":
        case = staircase(Lq, Lkv, H, 1, dtype, seed=Lkv)
    else:
        rg = split_ranges(Lkv, splits)
        n = 3 if kind == "tie3" else 2
        if len(rg) < n:
            raise ValueError("fewer ranges than tied keys")
        pick = [rg[0], rg[len(rg) // 2], rg[-1]] if n == 3 else [rg[0], rg[-1]]
        groups = [tuple(lo + 5 for lo, hi in pick), tuple(hi - 1 for lo, hi in pick)]
        case = tie(Lq, Lkv, groups, H, 1, dtype, seed=Lkv + splits)
    return Spec(f"split[{kind},{Lq}x{Lkv},S{splits}]", case.q, case.k, case.v, (0, Lkv), targets=case.targets,
                answer=1 if kind == "staircase" else 0)


def spec_staircase(Lq, Lkv, dtype=torch.bfloat16, H=2):
    """Family g: the lazy-rescale path."""
    case = staircase(Lq, Lkv, H, 1, dtype, seed=Lkv)
    return Spec(f"staircase[{Lq}x{Lkv}]", case.q, case.k, case.v, (0, Lkv), targets=case.targets, answer=1)


def spec_gaussian(Lq=520, Lkv=1100, dtype=torch.bfloat16, H=2):
    """Family i: iid unit Gaussians, the data of the older attention tests."""
    q, k, v = (_gauss((1, n, H, D), 9000 + i, dtype) for i, n in enumerate((Lq, Lkv, Lkv)))
    return Spec(f"gaussian[{Lq}x{Lkv}]", q, k, v, (0, Lkv), targets=torch.full((Lq, H, 1), -1, dtype=torch.long))


# Shapes: Lq from {1, 257, 300, 520} (ragged 128-, 256- and 64-row tiles), Lkv from {1, 63, 64, 65, 129, 200, 1100} (one key, one
# tile +- 1, a third tile of one key, past the 1024-key threshold of the default dispatch).
EVERY_KEY = [(1, 1, 1, 0), (257, 1, 1, 0), (257, 63, 1, 0), (257, 64, 1, 0), (257, 65, 1, 0), (300, 129, 1, 0), (300, 200, 2, 0),
             (1, 200, 1, 0), (520, 1100, 1, 0), (520, 1100, 1, 520), (520, 1100, 1, 1040)]            # Lq, Lkv, B, offset
CAUSAL = [(Lq, Lkv, cb, off) for Lq, Lkv in ((300, 520), (520, 1100)) for cb in (8, 96, 520) for off in (0, 37, Lkv - Lq)]
OUTSIDE = [(257, 63), (257, 65), (257, 129), (520, 1100)]                                             # Lq, Lkv
COUNTED = ([("tie", n, key, c) for n in (1, 63, 64, 200) for key in sorted({0, n, n // 2}) for c in (2, 3, 7, 448)] +
           [(kind, n, key, c) for kind in ("onto", "beside") for n in (63, 200) for key in (0, n) for c in (7, 448)])
SPLIT = [(kind, Lkv, S) for kind in ("one_hot", "tie2", "tie3", "staircase") for Lkv in (200, 1100) for S in (2, 3, 5, 16)
         if not (kind == "tie3" and S < 3)]
STAIRCASE = [(300, 200), (520, 1100)]


def all_specs(dtype):
    """Every input of the GPU file, for the CPU checks of the builders and of the emulation."""
    for Lq, Lkv, B, off in EVERY_KEY:
        yield spec_every_key(Lq, Lkv, dtype, B, off)
    for Lq, Lkv, cb, off in CAUSAL:
        for far in (False, True):
            yield spec_causal(Lq, Lkv, cb, off, dtype, far)
    for Lq, Lkv in OUTSIDE:
        yield spec_outside(Lq, Lkv, dtype)
    for seg0, seg1 in TWO_RANGE_WINDOWS:
        yield spec_two_ranges(seg0, seg1, dtype=dtype)
    for kind, n, key, c in COUNTED:
        yield spec_counted(kind, n, key, c, dtype=dtype)
    for kind, Lkv, S in SPLIT:
        yield spec_split(kind, Lkv, S, dtype=dtype)
    for Lq, Lkv in STAIRCASE:
        yield spec_staircase(Lq, Lkv, dtype)
