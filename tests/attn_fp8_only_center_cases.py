"""Restatements for K smoothing on the e4m3-only KV cache (include/rtv_hip_attn_fp8_only_center.h), on top of
tests/attn_fp8_cases.py and tests/attn_fp8_center_cases.py: the centre taken from the codes and the recentring of codes in place.
Plain torch, CPU or GPU tensors.

ARITHMETIC of the recentre, as the header states it, per code:
    1. delta = c_old - c_new               one fp32 subtraction
    2. x = fp32(code) * k_scale            one fp32 multiplication
    3. t = x + delta                       one fp32 addition (torch evaluates 2 and 3 as two kernels: nothing is contracted)
    4. code' = fc.codes(t, k_scale)        the fp32 division, the clamp to +-448 and the e4m3 conversion of the quantisers
A NaN code (0x7F, 0xFF) keeps its byte."""
import torch

import attn_fp8_cases as fc
import attn_fp8_center_cases as cc

F32 = torch.float32


def is_nan_code(codes):
    return (codes & 0x7F) == 0x7F


def dequantized(codes, k_scale):
    """fp32(code) * k_scale, one fp32 multiplication.  codes uint8 [..., H, D] -> fp32."""
    return codes.contiguous().view(fc.E4M3).float() * torch.as_tensor(k_scale, dtype=F32, device=codes.device)


def recentered(codes, c_old, c_new, k_scale):
    """-> (the codes moved from c_old to c_new, t = x + delta): codes uint8 [rows, H, D], the centres fp32 [H, D]."""
    delta = c_old.to(codes.device, F32) - c_new.to(codes.device, F32)
    t = dequantized(codes, k_scale) + delta
    return torch.where(is_nan_code(codes), codes, fc.codes(t, k_scale)), t


def recenter_rows(k8, row0, rows, c_old, c_new, k_scale=1.0, amax=None):
    """rtv_attn_k8_recenter restated: rows [row0, row0 + rows) of k8 in place; amax[0] raised to max |t|, NaNs ignored."""
    new, t = recentered(k8[row0:row0 + rows], c_old, c_new, k_scale)
    k8[row0:row0 + rows] = new
    if amax is not None:
        amax[0] = torch.maximum(amax[0], torch.nan_to_num(t.abs(), nan=0.0).max())
    return k8


def code_mean(codes, k_scale, c_old=None):
    """The centre rtv_attn_k8_center computes, from an fp64 sum: c_old + mean over the rows of code * k_scale -> float64 [H, D]."""
    m = dequantized(codes, k_scale).double().mean(0)
    return m if c_old is None else m + c_old.to(codes.device).double()


def attention_on_codes(q, codes, v, k_scale=1.0):
    """fc.restated_attention with the K operand given as codes (their dequantised values quantise back to themselves)."""
    return fc.restated_attention(q[None], dequantized(codes, k_scale)[None], v[None], k_scale=k_scale)


def rel_l2_triple(q, k, v, k_scale=1.0):
    """On one set of operands, against the fp64 definition on the bf16 operands: rel-L2 of the plain restated attention, of the
    attention on fresh codes centred under the mean of the plain codes, and of the attention on the plain codes recentred in
    place to that mean (two roundings)."""
    ref = cc.definition(q[None], k[None], v[None])
    plain = fc.codes(k, k_scale)
    zero = torch.zeros(k.shape[1:], dtype=F32)
    center = code_mean(plain, k_scale).float()
    fresh = cc.centered_codes(k, center, k_scale)
    moved = recentered(plain, zero, center, k_scale)[0]
    return tuple(fc.rel_l2(attention_on_codes(q, c, v, k_scale), ref) for c in (plain, fresh, moved)) + (center,)
