"""Restatements for the K smoothing of the fp8 attention shadow (include/rtv_hip_attn_fp8_center.h), on top of
tests/attn_fp8_cases.py: the centred K codes, the centred quantiser, the restated attention on centred keys, and the structured K
that carries per-channel offsets.  Plain torch, CPU or GPU tensors.

Centred codes: t = fp32(k) - c (one fp32 subtraction), then fc.codes(t, k_scale): the fp32 division, the clamp to +-448 and the
e4m3 conversion of the plain quantiser.  Attention on a centred shadow is attention on the keys k - c: every score of a query
moves by q^ . c, the same for every key, and softmax removes it - so fc.reference / fc.emulate / fc.restated_attention run
unchanged on the centred codes, and the fp64 definition on the bf16 operands stays the yardstick of the result."""
import math

import torch

import attn_fp8_cases as fc
from attn_cases import SCALE

BF16 = torch.bfloat16


def centered(k, center):
    """fp32(k) - center, k [..., H, D] bf16, center [H, D] fp32 -> fp32."""
    return k.float() - center.to(device=k.device, dtype=torch.float32)


def centered_codes(k, center, scale):
    """The K codes of a smoothed shadow."""
    return fc.codes(centered(k, center), scale)


def quantize_kv_centered(kc, vc, k8, v8t, row0, rows, center, k_scale=1.0, v_scale=1.0, amax=None):
    """fc.quantize_kv with the K codes of k - center; amax[0] follows |k - center|.  V exactly as fc.quantize_kv."""
    r = torch.arange(row0, row0 + rows, device=kc.device)
    kk = centered(kc[r], center)
    k8[r] = fc.codes(kk, k_scale)
    v8t[r >> 6, :, :, fc.SLOT_MAP.to(r.device)[r & 63]] = fc.codes(vc[r], v_scale)
    if amax is not None:
        amax[0] = torch.maximum(amax[0], kk.abs().max())
        amax[1] = torch.maximum(amax[1], vc[r].float().abs().max())
    return k8, v8t


def column_mean(k):
    """fp32 column means [H, D] of k [rows, H, D], from an fp64 sum."""
    return k.double().mean(0).float()


def restated_attention_centered(q, k, v, center=None, limits=None, k_scale=1.0, v_scale=1.0):
    """fc.restated_attention (BLHD, bf16) with the keys k - center as the quantiser sees them (fp32, not rounded to bf16);
    center None: the fp32 column means of k, per batch element."""
    out = torch.empty_like(q)
    for b in range(q.shape[0]):
        c = column_mean(k[b]) if center is None else center
        out[b:b + 1] = fc.restated_attention(q[b:b + 1], centered(k[b:b + 1], c), v[b:b + 1], limits=limits, k_scale=k_scale,
                                             v_scale=v_scale)
    return out


def definition(q, k, v):
    """fp64 softmax(scale q k^T) v on the bf16 operands, BLHD -> float64."""
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * SCALE
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.double())


def structured_k(rows, H, offset, seed=0, every=8):
    """K [rows, H, 128] bf16: N(0, 1) plus an offset of magnitude `offset`, with a sign drawn per (head, channel), on every
    `every`-th channel - keys as a trained k-norm weight or a slowly rotating RoPE pair leave them."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(rows, H, 128, generator=g)
    sign = torch.where(torch.rand(H, 128 // every, generator=g) < 0.5, -1.0, 1.0)
    k[:, :, ::every] += offset * sign
    return k.to(BF16)


def biased_operands(Lq=96, Lkv=200, H=2, offset=16.0, seed=0):
    """The case the smoothing is measured on: q, v N(0, 1), k = structured_k.  -> q [Lq, H, 128], k, v [Lkv, H, 128], bf16."""
    g = torch.Generator().manual_seed(1000 + seed)
    q = torch.randn(Lq, H, 128, generator=g).to(BF16)
    v = torch.randn(Lkv, H, 128, generator=g).to(BF16)
    return q, structured_k(Lkv, H, offset, seed), v


def rel_l2_pair(q, k, v, center):
    """(rel-L2 of the plain restated attention, of the restated attention on k - center) against the fp64 definition."""
    ref = definition(q[None], k[None], v[None])
    plain = fc.restated_attention(q[None], k[None], v[None])
    smooth = restated_attention_centered(q[None], k[None], v[None], center)
    return fc.rel_l2(plain, ref), fc.rel_l2(smooth, ref)


assert math.isclose(SCALE, 1.0 / math.sqrt(128))
