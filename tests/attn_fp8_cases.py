"""Restatements for the fp8 attention tests (include/rtv_hip_attn_fp8.h): the K / V quantiser and the layout of the e4m3 shadow,
the in-kernel Q quantisation, the fp64 reference on the DEQUANTISED operands, the acceptance bound and an emulation of the kernel's
arithmetic.  Plain torch, CPU or GPU tensors.  tests/test_attn_fp8_cpu.py checks the emulation and its mutants here,
tests/test_attn_fp8_gpu.py runs the HIP kernels on the same inputs (the builders of tests/attn_cases.py, imported unchanged).

The bound, per output element.  The reference is fp64 attention on q^ = codes(q) s_q, k^ = codes(k) k_scale, v^ = codes(v) v_scale,
so what the kernel adds is the rounding of P to e4m3, the fp32 sums and the bf16 rounding of the output.  With
P~ = exp(s - max s) over the visible keys and l~ = sum P~:
    e_j = max(2^-4 P~_j, min(P~_j, 2^-10))      half an ulp of e4m3 is 2^-4 relative for normals, 2^-10 absolute below 2^-6, and
                                                never more than P itself when P flushes to zero; the kernel's reference point is
                                                at most the row maximum, which only makes P larger than P~
    E   = sum_j e_j |v^_j| / l~
    accept  |out - ref| <= 2 (E + 2^-8 |ref|) + 1e-6      (2^-8: the bf16 rounding of the output; the factor 2 is the margin
                                                            attn_cases.within_bound grants as well)
"""
import math

import torch

from attn_cases import D, KT, SCALE, causal_limits

FP8_MAX = 448.0
E4M3 = torch.float8_e4m3fn
NAN_CODE = 0x7F
LOG2E = 1.4426950408889634


# ------------------------------------------------------------------------------------------------ layout
def slot(key):
    """Slot of key `key` (physical row & 63) in its storage tile of v8t: key 32 kb + 8 i + 4 g + j -> slot 32 g + 16 kb + 4 i + j."""
    kb, i, g, j = key >> 5, (key >> 3) & 3, (key >> 2) & 1, key & 3
    return 32 * g + 16 * kb + 4 * i + j


SLOT_MAP = torch.tensor([slot(k) for k in range(KT)], dtype=torch.long)


def codes(x, scale):
    """e4m3_rne(clamp(x / scale, +-448)) as uint8 codes; fp32 division, as quantize8 of fp8_quant.h."""
    y = (x.float() / torch.as_tensor(scale, dtype=torch.float32, device=x.device)).clamp(-FP8_MAX, FP8_MAX)
    return y.to(E4M3).view(torch.uint8)


def decode(c):
    """uint8 e4m3 codes -> float64 values (0x7F / 0xFF are NaN)."""
    return c.contiguous().view(E4M3).float().double()


def empty_shadow(cache_rows, H, fill=0, device="cpu"):
    return (torch.full((cache_rows, H, D), fill, dtype=torch.uint8, device=device),
            torch.full(((cache_rows + KT - 1) // KT, H, D, KT), fill, dtype=torch.uint8, device=device))


def quantize_kv(kc, vc, k8, v8t, row0, rows, k_scale=1.0, v_scale=1.0, amax=None, slot_map=SLOT_MAP):
    """Rows [row0, row0 + rows) of the caches kc / vc [cache_rows, H, D] into the shadow, in place; amax (float32 [2]) in place."""
    r = torch.arange(row0, row0 + rows, device=kc.device)
    k8[r] = codes(kc[r], k_scale)
    v8t[r >> 6, :, :, slot_map.to(r.device)[r & 63]] = codes(vc[r], v_scale)      # [rows, H, D] lands as [rows, H, D]
    if amax is not None:
        amax[0] = torch.maximum(amax[0], kc[r].float().abs().max())
        amax[1] = torch.maximum(amax[1], vc[r].float().abs().max())
    return k8, v8t


def gather_v(v8t, rows, slot_map=SLOT_MAP):
    """Codes of V rows `rows` (physical) out of v8t -> [len(rows), H, D]."""
    return v8t[rows >> 6, :, :, slot_map.to(rows.device)[rows & 63]]


def quantize_q(q):
    """The kernel's Q quantisation, q [..., D] bf16: one scale per row and head.  -> (codes uint8, s_q float32 [..., 1])."""
    amax = q.float().abs().amax(-1, keepdim=True)
    s_q = torch.clamp(amax, min=1e-12) * torch.tensor(1.0 / FP8_MAX, dtype=torch.float32, device=q.device)
    return codes(q, s_q), s_q


# ------------------------------------------------------------------------------------------------ a launch
class Launch:
    """One batch element of an attn_cases.Spec as the fp8 kernel sees it: q [Lq, H, D], the caches [rows, H, D], the window."""

    def __init__(self, spec, b=0, k_scale=1.0, v_scale=1.0):
        kc, vc = spec.caches()
        self.q, self.kc, self.vc = spec.q[b], kc[b], vc[b]
        self.seg0, self.seg1 = tuple(spec.seg0), tuple(spec.seg1) if spec.seg1[1] else (0, 0)
        self.causal_block, self.q_offset = spec.causal_block, spec.q_offset
        self.k_scale, self.v_scale = k_scale, v_scale
        self.name = f"{spec.name}[b{b}]"

    @property
    def cache_rows(self):
        return self.kc.shape[0]

    def window_rows(self, device="cpu"):
        (r0, n0), (r1, n1) = self.seg0, self.seg1
        return torch.cat([torch.arange(r0, r0 + n0, device=device), torch.arange(r1, r1 + n1, device=device)])

    def limits(self, delta=0):
        """Keys (of the window) a query row sees: j < lim[row]."""
        Lq, n = self.q.shape[0], self.seg0[1] + self.seg1[1]
        if self.causal_block <= 0:
            return torch.full((Lq,), n, dtype=torch.long)
        return torch.clamp(causal_limits(Lq, n, self.causal_block, self.q_offset) + delta, max=n)

    def shadow(self):
        """The whole cache quantised: (k8, v8t)."""
        k8, v8t = empty_shadow(self.cache_rows, self.kc.shape[1], device=self.kc.device)
        return quantize_kv(self.kc, self.vc, k8, v8t, 0, self.cache_rows, self.k_scale, self.v_scale)


def on_both_grids(spec):
    """A copy of `spec` whose K values are e4m3 numbers at k_scale 2 (hence at 1 as well: twice an e4m3 number below 224 is one) and
    whose V values are e4m3 numbers at v_scale 1 (hence at 0.5).  The shadows at scales (1, 1) and (2, 0.5) then hold the same
    numbers, every power of two moves through the fp32 arithmetic exactly, and the two launches must give the same answer."""
    from dataclasses import replace
    base = spec.k_base.clone()
    out = replace(spec, k_base=base, v_base=base if spec.interleaved else spec.v_base.clone())
    kc, vc = out.caches()
    kc.copy_((decode(codes(kc, 2.0)) * 2.0).to(kc.dtype))
    vc.copy_(decode(codes(vc, 1.0)).to(vc.dtype))
    return out


def reference(launch, k8, v8t):
    """fp64 attention on the dequantised operands -> (ref, E) [Lq, H, D] float64: the definition and the bound's E."""
    dev = k8.device
    rows = launch.window_rows(dev)
    qc, s_q = quantize_q(launch.q.to(dev))
    qh = decode(qc) * s_q.double()
    kh = decode(k8[rows]) * launch.k_scale
    vh = decode(gather_v(v8t, rows)) * launch.v_scale
    s = torch.einsum("qhd,khd->hqk", qh, kh) * SCALE
    lim = launch.limits().to(dev)
    vis = torch.arange(len(rows), device=dev).view(1, 1, -1) < lim.view(1, -1, 1)
    s = s.masked_fill(~vis, -math.inf)
    pt = torch.exp(s - s.amax(-1, keepdim=True))
    lt = pt.sum(-1, keepdim=True)
    e = torch.maximum(pt * 2.0 ** -4, torch.clamp(pt, max=2.0 ** -10))
    ref = torch.einsum("hqk,khd->qhd", pt / lt, vh)
    E = torch.einsum("hqk,khd->qhd", e / lt, vh.abs())
    return ref, E


def bound_ratio(out, ref, E):
    """-> (ok, ratio): ok = |out - ref| <= 2 (E + 2^-8 |ref|) + 1e-6 everywhere, ratio = max err / (E + 2^-8 |ref| + 5e-7); a
    non-finite output element counts as an infinite ratio."""
    err = (out.double() - ref).abs()
    tol = E + 2.0 ** -8 * ref.abs()
    ok = bool((err <= 2 * tol + 1e-6).all())
    ratio = torch.nan_to_num(err / (tol + 5e-7), nan=math.inf, posinf=math.inf)
    return ok, float(ratio.max())


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------ emulation
def emulate(launch, k8, v8t, slack=8.0, slot_map=SLOT_MAP, d_seg0=(0, 0), d_seg1=(0, 0), d_lim=0, apply_k_scale=True,
            apply_v_scale=True, zero_masked_v=True, truncate_p=False):
    """The kernel's arithmetic on the shadow: every 64-row storage tile a range touches is read whole; e4m3 codes of q and k, fp32
    sums, scores times s_q k_scale scale log2(e) in fp32, keys outside the window or beyond the row's limit at -inf (a select: a NaN
    score does not survive), reference point m = row maximum - slack, P = exp2(s - m) in fp32, l from the unrounded P, P rounded
    once to e4m3, the V bytes of keys outside the window replaced by zero, P V in fp32, O v_scale / l rounded once to bf16.
    The keyword arguments are the mutants of tests/test_attn_fp8_cpu.py: another slot map for the V read, window ends moved by
    d_seg = (d_first_row, d_end_row), the causal limit moved by d_lim, a scale not applied, masked V bytes not zeroed, P truncated."""
    dev = k8.device
    (r0, n0), (r1, n1) = launch.seg0, launch.seg1
    a0, b0 = r0 + d_seg0[0], r0 + n0 + d_seg0[1]
    a1, b1 = (r1 + d_seg1[0], r1 + n1 + d_seg1[1]) if n1 else (0, 0)
    phys, inside, key = [], [], []
    base = 0
    for a, b, first in ((a0, b0, r0), (a1, b1, r1)):
        if b <= a:
            continue
        t = torch.arange((a >> 6) * KT, ((b - 1 >> 6) + 1) * KT, device=dev)
        phys.append(t)
        inside.append((t >= a) & (t < b))
        key.append(t - a + base)                       # key index inside the (mutated) window
        base += b - a
    phys, inside, key = torch.cat(phys), torch.cat(inside), torch.cat(key)
    qc, s_q = quantize_q(launch.q.to(dev))
    kcodes = decode(k8[phys.clamp(max=launch.cache_rows - 1)]).float()
    vcodes = decode(gather_v(v8t, phys, slot_map)).float()
    if zero_masked_v:
        vcodes = torch.where(inside.view(-1, 1, 1), vcodes, torch.zeros_like(vcodes))
    c = s_q * torch.tensor(SCALE * LOG2E * (launch.k_scale if apply_k_scale else 1.0), dtype=torch.float32)      # [Lq, H, 1]
    s = torch.einsum("qhd,khd->hqk", decode(qc).float(), kcodes) * c.permute(1, 0, 2)
    lim = (launch.limits(d_lim) if n1 == 0 else torch.full((launch.q.shape[0],), base, dtype=torch.long)).to(dev)
    vis = inside.view(1, 1, -1) & (key.view(1, 1, -1) < lim.view(1, -1, 1))
    s = torch.where(vis, s, torch.full_like(s, -math.inf))
    m = s.amax(-1, keepdim=True) - slack
    p = torch.exp2(s - m)
    l = p.sum(-1)
    p8 = p.to(E4M3)
    if truncate_p:                                      # round towards zero: where RNE went up, the code below (P >= 0)
        p8 = torch.where(p8.float() > p, p8.view(torch.uint8) - 1, p8.view(torch.uint8)).view(E4M3)
    p8 = p8.float()
    o = torch.einsum("hqk,khd->qhd", p8, vcodes)
    vs = launch.v_scale if apply_v_scale else 1.0
    return (o * (torch.tensor(vs, dtype=torch.float32) / l).permute(1, 0).unsqueeze(-1)).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ the oracle's attention function
def restated_attention(q, k, v, limits=None, k_scale=1.0, v_scale=1.0, slack=8.0):
    """The fp8 self-attention as an attention function of oracle/wan_oracle.py (BLHD in, BLHD out, bf16): K and V quantised per
    tensor kind, Q per (row, head), the kernel's arithmetic as in `emulate`, without the storage layout.  limits: per-query key
    prefix (the block-causal pass)."""
    qc, s_q = quantize_q(q)
    c = s_q * torch.tensor(SCALE * LOG2E * k_scale, dtype=torch.float32, device=q.device)                      # [B, Lq, H, 1]
    kf, vf = (decode(codes(t, s)).float() for t, s in ((k, k_scale), (v, v_scale)))
    out = torch.empty_like(q)
    for h in range(q.shape[2]):                         # a head at a time: the score matrix of one head is what fits
        s = torch.einsum("bqd,bkd->bqk", decode(qc[:, :, h]).float(), kf[:, :, h]) * c[:, :, h]
        if limits is not None:
            vis = torch.arange(k.shape[1], device=q.device).view(1, 1, -1) < limits.to(q.device).view(1, -1, 1)
            s = torch.where(vis, s, torch.full_like(s, -math.inf))
        p = torch.exp2(s - (s.amax(-1, keepdim=True) - slack))
        l = p.sum(-1, keepdim=True)
        o = torch.einsum("bqk,bkd->bqd", p.to(E4M3).float(), vf[:, :, h])
        out[:, :, h] = (o * (v_scale / l)).to(q.dtype)
    return out
