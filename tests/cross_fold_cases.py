"""Inputs, the fp64 definition and the bound of the folded cross-attention tests (tests/test_cross_fold_gpu.py; also used by
scripts/cross_fold_probs_ratios.py, which measures the factor `C_BOUND` below on today's kernel).

The probabilities kernel writes P[row, h * kh + t] = softmax_t(scale q_h . k_{h,t} + log(count_t)) in bf16.  Reference: the
same softmax in fp64 from the same bf16 q / k.  Bound per element (the form of the peaked attention tests, attn_cases.py):

    |P - P_ref| <= C_BOUND * u * P_ref + TINY,     u = 2^-8.

C_BOUND is NOT taken from the kernel under test: it is twice the largest ratio |P - P_ref| / (u P_ref + TINY) that TODAY's
path (rtv_attn_fwd_dup with V = identity columns, whose output IS its P) reaches on these same inputs, or the peaked tests'
factor 4, whichever is smaller.  Measured (profiles/cross_fold_probs_ratios.txt): today's largest ratio is 1.943 (its P is
rounded twice, before and after the normalisation: up to u each) -> C_BOUND = min(2 x 1.943, 4) = 3.89.  (The new kernel rounds
once and reads 0.996 in the same table.)
TINY = 2^-120: exponentials below the smallest normal fp32 / bf16 number (2^-126) are flushed to zero by the hardware exp2 and by
the bf16 conversion, in the reference they are not; 2^-120 leaves room for the normalisation (1 / l <= 1) and a few flushed terms.
"""
import math

import torch

import attn_cases as ac

U = 2.0 ** -8
TINY = 2.0 ** -120
C_BOUND = 3.89

LQ = (1, 33, 200, 257)            # ragged against the 32-row wave, the 128-row tile, more than one tile
HEADS = (2, 3)
KEYS = (1, 8, 64, 65, 100, 128)   # the whole window (real keys + the counted one): 1 .. 4 key blocks of 32, full and ragged
COUNTS = (1, 448)
FAMILIES = ("gaussian", "peaked")


def round_up(x, m):
    return (x + m - 1) // m * m


def fold_dims(num_heads, text_rows):
    """(kh, k_fold) of the folded layout: the index arithmetic of rtv_cross_fold_dims."""
    kh = round_up(text_rows + 1, 8)
    return kh, round_up(num_heads * kh, 64)


def probs_inputs(family, Lq, H, keys, count):
    """-> (q [Lq, H, 128], k [keys, H, 128], dup_key) bf16 CPU tensors.  The counted key is the LAST key of the window (where
    the cross-attention has it).  gaussian: iid N(0, 1).  peaked: attn_cases.spec_counted("beside"): even rows hang on a real key
    with the counted key 0.9 x that key beside it, odd rows on one key each (scores of ~45 nats)."""
    dup_key = keys - 1
    if family == "gaussian" or keys == 1:
        g = torch.Generator().manual_seed(1000 * keys + 10 * Lq + H + (0 if family == "gaussian" else 5))
        q = torch.randn(Lq, H, ac.D, generator=g).to(torch.bfloat16)
        k = torch.randn(keys, H, ac.D, generator=g).to(torch.bfloat16)
        if family == "peaked":        # one key: nothing to hang on; large scores instead
            q = (q.float() * 4.0).to(torch.bfloat16)
        return q, k, dup_key
    spec = ac.spec_counted("beside", keys - 1, dup_key, max(count, 2), Lq=Lq, H=H)
    k, _ = spec.window()
    return spec.q[0].contiguous(), k[0].contiguous(), dup_key


def probs_ref64(q, k, dup_key, count, scale=ac.SCALE):
    """fp64 softmax [Lq, H, keys] with + log(count) on the counted key."""
    s = torch.einsum("qhd,khd->qhk", q.double(), k.double()) * scale
    s[..., dup_key] += math.log(count)
    return torch.softmax(s, dim=-1)


def probs_ratio(p, ref):
    """Largest |p - ref| / (u ref + TINY); a non-finite element counts as infinite."""
    r = (p.double() - ref).abs() / (U * ref + TINY)
    return float(torch.nan_to_num(r, nan=math.inf, posinf=math.inf).max())
