"""Unit-test support for the Wan VAE mid-block attention and glue kernels (no GPU needed).

This module holds, as plain torch functions that run on any device,
  * the inputs the GPU tests (tests/test_vae_gpu.py, tests/test_taehv_gpu.py) feed to the kernels,
  * the high-precision references and the acceptance of each GPU test, as a `*_violation` function that returns
    max(error / bound) (<= 1 passes; nan / inf and structural faults count as inf),
  * restatements of the native arithmetic written from the comments in csrc/vae_decode.hip and csrc/taehv.hip, with
    NAMED SLIPS: the mistakes a rewrite of that code could make.

The tests here prove, on the CPU, that (a) each restatement without a slip stays inside the acceptance its GPU test
uses - so the acceptance is attainable by correct fp16 arithmetic - and (b) each slip breaks it by at least 10x at the
inputs the GPU test uses (for the bit-exact acceptances: in at least 10 elements), so the GPU test would notice it.
"""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from realtime_video_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "realtime_video_amd", "csrc")
NEW_SYMBOLS = ("rtv_vae_attn_arena_bytes", "rtv_vae_mid_attention", "rtv_vae_prep", "rtv_vae_final", "rtv_vae_upsample_cache_t1",
               "rtv_vae_enc_prep", "rtv_vae_enc_final", "rtv_taehv_prep")
F16_MAX = 65504.0
F16_SUBNORMAL = 2.0 ** -24      # 6e-8, the fp16 subnormal step


def f16r(x):
    """Round to fp16, continue in fp32: a point where the native path stores fp16."""
    return x.half().float()


def f16_ord(t):
    """fp16 tensor -> int32 that is monotone in the value (+0 and -0 both map to 0): differences count ulps."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def f16_ulp_diff(a, b):
    return int((f16_ord(a) - f16_ord(b)).abs().max())


def bits_mismatch(a, b):
    """Number of elements whose bit patterns differ (same dtype, same shape)."""
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert a.dtype == b.dtype and a.shape == b.shape
    return int((a.contiguous().view(iv) != b.contiguous().view(iv)).sum())


def _ratio(err, bound):
    r = err / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


# ====================================================================================================== softmax rows
# (n, ldp, rows): production 60 x 104 first; one exact trip; one trip + one 8-column group; a single group; the old test's
# size; two exact trips; an odd count (77) of 8-column groups
SOFTMAX_SHAPES = [(6240, 6272, 512), (2048, 2048, 64), (2056, 2112, 64), (8, 64, 16), (96, 128, 96), (4096, 4096, 32),
                  (77 * 8, 640, 64)]
SOFTMAX_DISTS = ["gauss3", "peaked", "max_last8", "max_wave3", "constant", "all_min", "mixed_extreme"]
SOFTMAX_LDS_EXTRA = 24      # input row stride lds = n + 24 > n; the columns beyond n hold poison


def wave_of_column(c):
    """softmax_rows_kernel: thread t owns columns 8t .. 8t+7 of every 2048-column trip; wave = t / 64."""
    return (c % 2048) // 512


def softmax_scores(dist, n, rows, seed=0, device="cpu"):
    """fp16 scores [rows][n + SOFTMAX_LDS_EXTRA]; columns >= n hold 65504 (read by mistake, it takes over the row's maximum)."""
    g = torch.Generator().manual_seed(seed * 1000 + n)
    r = torch.arange(rows)
    if dist == "gauss3":
        s = torch.randn(rows, n, generator=g) * 3
    elif dist == "peaked":                       # one column 30 above the rest
        s = torch.randn(rows, n, generator=g)
        col = torch.randint(0, n, (rows,), generator=g)
        s[r, col] = s.max(dim=1).values + 30
    elif dist == "max_last8":                    # the maximum sits in the last 8 columns (the partial trip's last group)
        s = torch.randn(rows, n, generator=g) * 3
        s[r, n - 1 - (r % 8)] = 40.0
    elif dist == "max_wave3":                    # the maximum sits in a column only wave 3 reads, exp(max - other) overflows fp32
        s = torch.randn(rows, n, generator=g) * 3
        cols = torch.tensor([c for c in range(n) if wave_of_column(c) == 3] or [n - 1])
        s[r, cols[(r * 37) % len(cols)]] = 120.0
    elif dist == "constant":
        s = torch.full((rows, n), 1.0) * (r.float()[:, None] - rows / 2) * 7.0
    elif dist == "all_min":
        s = torch.full((rows, n), -F16_MAX)
    elif dist == "mixed_extreme":                # -60000 everywhere, +60000 in a few columns: none of them in wave 0 where n allows
        s = torch.full((rows, n), -60000.0)
        hi = torch.tensor([c for c in range(n) if wave_of_column(c) != 0] or list(range(n)))
        for j in range(3):
            s[r, hi[(r * 13 + j * 101) % len(hi)]] = 60000.0
    else:
        raise ValueError(dist)
    out = torch.full((rows, n + SOFTMAX_LDS_EXTRA), F16_MAX)
    out[:, :n] = s
    return out.half().to(device)


def softmax_reference64(s, n):
    return torch.softmax(s[:, :n].double(), dim=-1)


def softmax_violation(got, s, n):
    """got fp16 [rows][ldp].  Per element |got - ref| <= 1e-3 * ref + 6e-8 (half an fp16 ulp is 4.9e-4 relative, 6e-8 the
    subnormal step); every row sum within n * 2^-12 of 1; pad columns exactly zero."""
    ref = softmax_reference64(s, n)
    g = got[:, :n].double()
    v = _ratio((g - ref).abs(), 1e-3 * ref + F16_SUBNORMAL)
    v = max(v, _ratio((g.sum(dim=1) - 1).abs(), torch.full((g.shape[0],), n * 2.0 ** -12, dtype=torch.float64, device=g.device)))
    if got.shape[1] > n and bool((got[:, n:].view(torch.int16) != 0).any()):
        v = float("inf")
    return v


def softmax_restated(s, n, ldp, slip=None):
    """softmax_rows_kernel in torch: fp32 max, fp32 sum of exp(s - max), exp(s - max) / sum stored fp16, zero pad to ldp."""
    x = s[:, :n].float()
    col = torch.arange(n, device=s.device)
    live = torch.ones(n, dtype=torch.bool, device=s.device)
    if slip == "drop_partial_trip":              # the column loop stops after the last FULL trip of 2048
        live = col < (n // 2048) * 2048
    wave0 = live & (wave_of_column(col) == 0)
    ninf = torch.full_like(x, -float("inf"))
    mx = torch.where(wave0 if slip == "wave0_max" else live, x, ninf).max(dim=1, keepdim=True).values
    e = torch.exp(x - mx)
    sm = torch.where(wave0 if slip == "wave0_sum" else live, e, torch.zeros_like(e)).sum(dim=1, keepdim=True)
    p = torch.where(live, e * (1.0 / sm), torch.zeros_like(e))
    out = torch.zeros(s.shape[0], ldp, dtype=torch.float16, device=s.device)
    if slip == "pad_nonzero":
        out.fill_(7.0)
    out[:, :n] = p.half()
    return out


SOFTMAX_SLIPS = ["wave0_max", "wave0_sum", "drop_partial_trip", "pad_nonzero"]


# ====================================================================================================== RMS norm (+ SiLU)
def rms_ppb(C):
    return 768 // (C // 8)      # pixels per block of rmsnorm_silu_cl_kernel


def rms_npix_cases(C):
    p = rms_ppb(C)
    return [1, p - 1, p, 5 * p, 6240, 480 * 832 // 64]


def rms_inputs(C, npix, scale, seed=0, device="cpu"):
    """x fp16 [npix][C] at `scale`; pixel 0 all zero, the last pixel a single non-zero channel."""
    g = torch.Generator().manual_seed(seed + C + npix)
    x = torch.randn(npix, C, generator=g) * scale
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    if npix >= 3:
        x[0] = 0
        x[-1] = 0
        x[-1, C // 2 + 1] = -3.0 * scale
    return x.half().to(device), gamma.half().to(device)


def rms_reference64(x, gamma, silu):
    x = x.double()
    nrm = x.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)
    y = x / nrm * math.sqrt(x.shape[1]) * gamma.double()
    return y * torch.sigmoid(y) if silu else y


def rms_violation(got, x, gamma, silu):
    """|got - ref| <= 1e-3 * |ref| + 1e-3 * 2^-14 (2^-14 = the smallest normal fp16); an all-zero pixel gives exact zeros."""
    ref = rms_reference64(x, gamma, silu)
    v = _ratio((got.double() - ref).abs(), 1e-3 * ref.abs() + 1e-3 * 2.0 ** -14)
    zero_px = (x == 0).all(dim=1)
    if bool((got[zero_px].view(torch.int16) & 0x7FFF != 0).any()):
        v = float("inf")
    return v


def rms_restated(x, gamma, silu, slip=None):
    xf = x.float()
    ssq = (x * x).float().sum(dim=1, keepdim=True) if slip == "fp16_squares" else (xf * xf).sum(dim=1, keepdim=True)
    nrm = ssq.sqrt()
    if slip != "no_floor":
        nrm = nrm.clamp_min(1e-12)
    y = xf * (math.sqrt(x.shape[1]) / nrm) * gamma.float()
    return (y * torch.sigmoid(y) if silu else y).half()


RMS_SLIPS = ["no_floor", "fp16_squares"]


# ====================================================================================================== mid-block attention
ATTN_C = 384
ATTN_SIZES = [(8, 12), (7, 16), (30, 52), (60, 104)]     # P = 96 (not a multiple of 64), 112, 1560, 6240 (production)
ATTN_REGIMES = ["init", "peaked"]
ATTN_BV_CONST = 4.0


def attn_weights(regime, seed=0, bv_const=None):
    """AttentionBlock weights, fp16-rounded, in the reference's form (un-scaled to_qkv): uniform(-1, 1) / sqrt(384) like
    oracle/vae_oracle.make_vae_weights, gamma 1 + 0.1 * randn.  `peaked` scales the q and k projections (attn_peak_scale)."""
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / math.sqrt(ATTN_C)
    u = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1) * bound
    W = {"gamma": 1 + 0.1 * torch.randn(ATTN_C, generator=g)}
    for n in ("q", "k", "v", "proj"):
        W["w" + n] = u(ATTN_C, ATTN_C)
        W["b" + n] = u(ATTN_C)
    if regime == "peaked":
        for n in ("wq", "bq", "wk", "bk"):
            W[n] = W[n] * ATTN_PEAK_SCALE
    if bv_const is not None:
        W["bv"] = torch.full((ATTN_C,), float(bv_const))
    return {k: v.half() for k, v in W.items()}


# With x ~ N(0, 1) the init-scale scores q.k / sqrt(384) have a standard deviation of 0.34 on the fp64 reference
# (test_attention_regimes below keeps that honest): q and k each scaled by sqrt(6 / 0.34) give about 6
ATTN_PEAK_SCALE = math.sqrt(6.0 / 0.34)


def attn_input(h, w, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(100 + seed + h * w)
    return torch.randn(h * w, ATTN_C, generator=g).half().to(device)


def attn_reference64(x, W):
    """AttentionBlock (wan/modules/vae.py:212-251) in fp64 on the fp16-rounded input and weights: RMS norm with gamma, q / k / v
    1x1 convolutions with bias, softmax(q k^T / sqrt(384)), projection + identity.  Returns (y, scores)."""
    d = {k: v.to(x.device).double() for k, v in W.items()}
    xd = x.double()
    xn = xd / xd.pow(2).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12) * math.sqrt(ATTN_C) * d["gamma"]
    q, k, v = (xn @ d["w" + n].t() + d["b" + n] for n in "qkv")
    s = q @ k.t() / math.sqrt(ATTN_C)
    o = torch.softmax(s, dim=-1) @ v
    return o @ d["wproj"].t() + d["bproj"] + xd, s


def attn_native_weights(W, device="cpu"):
    """What the decoder hands to the library (vae_decoder.py load_state_dict): the softmax scale folded into wq / bq, fp16."""
    sc = 1.0 / math.sqrt(ATTN_C)
    N = dict(W)
    N["wq"], N["bq"] = (W["wq"].float() * sc).half(), (W["bq"].float() * sc).half()
    return {k: v.to(device).contiguous() for k, v in N.items()}


def attn_restated16(x, N, ldp=None, slip=None):
    """mid_attention() in torch: fp32 math with a .half() wherever the native path stores fp16 (xn, q, k, V^T, S, P, o, y).
    N = attn_native_weights(...).  ldp = padded key count (multiple of 64) of the P and V^T buffers."""
    f = {k: v.float() for k, v in N.items()}
    P = x.shape[0]
    ldp = ldp or (P + 63) // 64 * 64
    xf = x.float()
    xn = f16r(xf * (math.sqrt(ATTN_C) / (xf * xf).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-12)) * f["gamma"])
    wq, bq = f["wq"], f["bq"]
    if slip == "q_scale_twice":
        wq, bq = f16r(wq / math.sqrt(ATTN_C)), f16r(bq / math.sqrt(ATTN_C))
    q = f16r(xn @ wq.t() + bq)
    k = f16r(xn @ f["wk"].t() + f["bk"])
    vt = torch.zeros(ATTN_C, ldp, device=x.device)
    v = f["wv"] @ xn.t()
    if slip == "bv_before_softmax":              # bias folded into V^T, in front of the softmax weights
        v = v + f["bv"][:, None]
    vt[:, :P] = f16r(v)
    S = f16r(q @ k.t())
    Pm = torch.zeros(P, ldp, device=x.device)
    Pm[:, :P] = f16r(torch.softmax(S, dim=-1))
    if slip == "pad_counted":                    # stale pad columns: P's left as they were, V^T's not cleared
        Pm[:, P:] = 1.0 / P
        vt[:, P:] = 1.0
    o = Pm @ vt.t()
    if slip not in ("bv_omitted", "bv_before_softmax"):
        o = o + f["bv"] * (2 if slip == "bv_twice" else 1)
    o = f16r(o)
    return f16r(o @ f["wproj"].t() + f["bproj"] + xf).half()


ATTN_SLIPS = ["pad_counted", "bv_omitted", "bv_twice", "q_scale_twice"]


def attn_errors(got, ref):
    d = got.double() - ref
    return float(d.norm() / ref.norm()), float(d.abs().max())


def attn_violation(got, x, W, e16=None):
    """err <= 2 * e16 in rel-L2 and in max-abs, e16 = the error of the fp16 restatement against the fp64 reference.
    Returns (violation, err, e16)."""
    ref, _ = attn_reference64(x, W)
    if e16 is None:
        e16 = attn_errors(attn_restated16(x, attn_native_weights(W, x.device)), ref)
    err = attn_errors(got, ref)
    if not all(math.isfinite(e) for e in err):
        return float("inf"), err, e16
    return max(err[0] / (2 * e16[0]), err[1] / (2 * e16[1])), err, e16


# ====================================================================================================== glue kernels
VAE_MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508,
            0.4134, -0.0715, 0.5517, -0.3632, -0.1922, -0.9497, 0.2503, -0.2921]
VAE_STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743,
           3.2687, 2.1526, 2.8652, 1.5579, 1.6382, 1.1253, 2.8251, 1.9160]
PREP_HW = [96, 77, 6240, 127, 129]


def prep_inputs(hw, identity, T=3, seed=0, device="cpu"):
    """z fp16 [T][16][hw], mean, std, conv2 weight [16][16] + bias (float32).  identity: conv2 = I, bias 0 - the output is then
    the de-normalised latent itself and every rounding point shows bit for bit."""
    g = torch.Generator().manual_seed(seed + hw)
    z = (torch.randn(T, 16, hw, generator=g) * 1.5).half()
    if identity:
        w2, b2 = torch.eye(16), torch.zeros(16)
    else:
        w2 = f16r((torch.rand(16, 16, generator=g) * 2 - 1) * 0.25)
        b2 = f16r((torch.rand(16, generator=g) * 2 - 1) * 0.25)
    return [t.to(device) for t in (z, torch.tensor(VAE_MEAN), torch.tensor(VAE_STD), w2, b2)]


def _inv_std(std):
    return f16r(1.0 / f16r(std))


def prep_denorm(z_t, mean, std, slip=None):
    """fp16 arithmetic of the reference, z / (1 / std) + mean: round(round(z / round(1 / round(std))) + round(mean)); [16][hw] fp32."""
    d = z_t.float() / _inv_std(std)[:, None]
    if slip != "prep_no_round_div":
        d = f16r(d)
    return f16r(d + f16r(mean)[:, None])


def prep_restated(z, t, mean, std, w2, b2, slip=None, matrix_dtype=torch.float32):
    """vae_prep_kernel: de-normalise, then the 16 x 16 matrix in float32 -> fp16 channels-last [hw][32], channels 16..31 zero."""
    zin = prep_denorm(z[0 if slip == "prep_t_ignored" else t], mean, std, slip).to(matrix_dtype)
    y = (w2.to(matrix_dtype) @ zin + b2.to(matrix_dtype)[:, None]).t()
    out = torch.zeros(z.shape[2], 32, dtype=torch.float16, device=z.device)
    out[:, :16] = y.half()
    return out


def ulp16(t):
    """One fp16 ulp at the magnitude of t (the subnormal step below 2^-14)."""
    return torch.clamp_min(2.0 ** (torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -14))) - 10), 2.0 ** -24)


def prep_violation(got, z, t, mean, std, w2, b2, identity):
    """identity conv2: bit-exact (mismatch count, 0 passes).  Random conv2: the kernel's float32 sum of 17 terms differs from the
    exact one by at most 17 * 2^-24 * (|b| + sum |w z|).  Where the result is not a cancellation, |result| >= 2^-7 of that sum,
    this is below a quarter of an fp16 ulp and the output must be within 1 fp16 ulp of the fp64 matrix rounded to fp16; where it
    is, an ulp of the tiny result says nothing about a float32 sum, and the output must be within that float32 bound plus one
    fp16 ulp of the exact result.  Returns the larger of the two (<= 1 passes).  Channels 16..31 are exact zeros."""
    if bool((got[:, 16:].view(torch.int16) != 0).any()):
        return float("inf")
    if identity:
        return bits_mismatch(got, prep_restated(z, t, mean, std, w2, b2))
    zin = prep_denorm(z[t], mean, std).double()
    exact = (w2.double() @ zin + b2.double()[:, None]).t()
    terms = (w2.double().abs() @ zin.abs() + b2.double().abs()[:, None]).t()
    plain = exact.abs() >= 2.0 ** -7 * terms
    d_ulp = (f16_ord(got[:, :16]) - f16_ord(exact.half())).abs()
    v = float(d_ulp[plain].max()) if bool(plain.any()) else 0.0
    if bool((~plain).any()):
        err = (got[:, :16].double() - exact).abs()
        v = max(v, _ratio(err[~plain], (17 * 2.0 ** -24 * terms + ulp16(exact))[~plain]))
    return v


def final_inputs(T, in_hw, seed=0, device="cpu"):
    """Head output fp16 [T][in_hw][8]: channels 0..2 around and beyond +-1 with +-0, +-1, +-65504 and subnormals mixed in;
    channels 3..7 poison (NaN)."""
    g = torch.Generator().manual_seed(seed + T)
    x = torch.randn(T, in_hw, 8, generator=g) * 1.2
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, F16_MAX, -F16_MAX, 6e-8, -6e-8, 1.0009765625, -1.0009765625, 0.99951171875])
    idx = torch.randint(0, len(special), (T, in_hw, 8), generator=g)
    x = torch.where(torch.rand(T, in_hw, 8, generator=g) < 0.1, special[idx], x)
    x[..., 3:] = float("nan")
    return x.half().to(device)


def final_restated(x, hw, skip_px, slip=None):
    """vae_final_kernel: rows skip_px .. skip_px + hw of every frame, channels 0..2, clamp to [-1, 1], float32 [T][3][hw]."""
    s = 0 if slip == "skip_ignored" else skip_px
    y = x[:, s:s + hw, :3].float()
    if slip != "no_clamp":
        y = y.clamp(-1.0, 1.0)
    return y.permute(0, 2, 1).contiguous()


def upsample_inputs(slice_elems, seed=0, device="cpu"):
    """[c0 | c1 | x] fp16 [3][slice]: c1 mixes +0, -0, fp16 subnormals and ordinary values; x is non-zero where c1 is zero and the
    other way round often enough that a `where` keyed on x shows; c0 poison."""
    g = torch.Generator().manual_seed(seed)
    kinds = torch.randint(0, 5, (slice_elems,), generator=g)
    c1 = torch.randn(slice_elems, generator=g)
    c1 = torch.where(kinds == 0, torch.zeros(()), c1)
    c1 = torch.where(kinds == 1, -torch.zeros(()), c1)
    c1 = torch.where(kinds == 2, torch.full((), 6e-8) * torch.randint(1, 1000, (slice_elems,), generator=g), c1)
    c1 = torch.where(kinds == 3, -torch.full((), 6e-8) * torch.randint(1, 1000, (slice_elems,), generator=g), c1)
    x = torch.randn(slice_elems, generator=g)
    x = torch.where(torch.rand(slice_elems, generator=g) < 0.2, torch.zeros(()), x)
    x = torch.where(torch.rand(slice_elems, generator=g) < 0.1, -torch.zeros(()), x)
    buf = torch.stack([torch.full((slice_elems,), float("nan")), c1, x]).half()
    assert int((buf[1].view(torch.int16) == -32768).sum()) > slice_elems // 10      # -0 survives the construction
    return buf.to(device)


def upsample_restated(buf, slip=None):
    """upsample_cache_t1_kernel: cache <- [where(old_cache_last == 0, 0, x), x] on [c0 | c1 | x]; x stays."""
    c1, x = buf[1], buf[2]
    if slip == "where_on_x":
        key = x == 0
    elif slip == "neg_zero_not_zero":
        key = c1.view(torch.int16) == 0
    else:
        key = c1 == 0                        # IEEE comparison: +0 and -0 are zero, subnormals are not
    return torch.stack([torch.where(key, torch.zeros_like(x), x), x, x])


def enc_prep_inputs(Ttot, hw, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed + hw)
    return (torch.rand(3, Ttot, hw, generator=g) * 2 - 1).half().to(device)


def enc_prep_restated(frames, t0, T, slip=None):
    """vae_enc_prep_kernel: frames t0 .. t0 + T of planar [3][Ttot][hw] -> channels-last [T][hw][32], channels 3..31 zero."""
    s = 0 if slip == "t0_ignored" else t0
    out = torch.zeros(T, frames.shape[2], 32, dtype=torch.float16, device=frames.device)
    out[..., :3] = frames[:, s:s + T].permute(1, 2, 0)
    return out


def enc_final_inputs(T, hw, identity, seed=0, device="cpu"):
    """Head output fp16 [T][hw][32], conv1 weight [32][32] + bias [32], mean, std (float32).  identity: conv1 = I, bias 0."""
    g = torch.Generator().manual_seed(seed + hw)
    x = (torch.randn(T, hw, 32, generator=g) * 2).half()
    if identity:
        w1, b1 = torch.eye(32), torch.zeros(32)
    else:
        w1 = f16r((torch.rand(32, 32, generator=g) * 2 - 1) * 0.18)
        b1 = f16r((torch.rand(32, generator=g) * 2 - 1) * 0.18)
    return [t.to(device) for t in (x, w1, b1, torch.tensor(VAE_MEAN), torch.tensor(VAE_STD))]


def enc_final_restated(x, w1, b1, mean, std, mu, tout, slip=None, matrix_dtype=torch.float32):
    """vae_enc_final_kernel: a = conv1(x)[:16] in float32, round(round(round(a) - round(mean)) * round(1 / round(std))) written to
    frames tout .. tout + T of mu fp16 [16][Tout_tot][hw]; the other frames keep what they held.  Returns (mu, a)."""
    a = (x.to(matrix_dtype) @ w1[:16].to(matrix_dtype).t() + b1[:16].to(matrix_dtype)).float()        # [T][hw][16]
    d = f16r(a) - f16r(mean)
    if slip != "final_no_round_sub":
        d = f16r(d)
    v = f16r(d * _inv_std(std))
    out = mu.clone()
    s = 0 if slip == "tout_ignored" else tout
    out[:, s:s + x.shape[0]] = v.permute(2, 0, 1).half()
    return out, a


def enc_final_violation(got, x, w1, b1, mean, std, mu0, tout, identity):
    """identity conv1: bit-exact (mismatch count).  Otherwise the float32 sum of 33 terms differs from the exact a by at most
    da = 33 * 2^-24 * (|b| + sum |w x|), which moves round(a) by at most da + ulp16(a); the difference d = round(a) - round(mean)
    moves by as much and is rounded (one more ulp16(d)); the chain scales that by 1 / std and rounds the result:
    |got - ref| <= (da + ulp16(a) + ulp16(d)) / std + ulp16(ref), ref from the matrix in fp64; frames outside
    tout .. tout + T bit-identical to mu0.  Returns max(err / bound) then."""
    ref, a = enc_final_restated(x, w1, b1, mean, std, mu0, tout, matrix_dtype=torch.float32 if identity else torch.float64)
    if identity:
        return bits_mismatch(got, ref)
    T = x.shape[0]
    keep = torch.ones(mu0.shape[1], dtype=torch.bool, device=mu0.device)
    keep[tout:tout + T] = False
    if bits_mismatch(got[:, keep], mu0[:, keep]):
        return float("inf")
    g, r = got[:, tout:tout + T].float(), ref[:, tout:tout + T].float()
    da = 33 * 2.0 ** -24 * (x.float().abs() @ w1[:16].abs().t() + b1[:16].abs())
    d = f16r(a) - f16r(mean)
    bound = (da + ulp16(a) + ulp16(d)).permute(2, 0, 1) * _inv_std(std)[:, None, None] + ulp16(r)
    return _ratio((g - r).abs(), bound)


def taehv_prep_inputs(T, hw, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed + hw)
    z = torch.randn(T, 16, hw, generator=g) * 4
    z[:, :, :8] = torch.tensor([0.0, -0.0, 60.0, -60.0, F16_MAX, -F16_MAX, 6e-8, 1e-3])
    return z.half().to(device)


def taehv_prep_restated(z, slip=None, dtype=torch.float32):
    """taehv_prep_kernel: z fp16 [T][16][hw] -> tanh(z / 3) * 3 -> channels-last [T][hw][32], channels 16..31 zero."""
    y = z.to(dtype)
    if slip != "no_clamp":
        y = torch.tanh(y / 3) * 3
    out = torch.zeros(z.shape[0], z.shape[2], 32, dtype=torch.float16, device=z.device)
    out[..., :16] = y.permute(0, 2, 1).half()
    return out


def taehv_prep_violation(got, z):
    """<= 1 fp16 ulp from fp16(tanh(z / 3) * 3) evaluated in fp64 (the kernel evaluates tanhf in fp32 and rounds once more);
    channels 16..31 exact zeros."""
    if bool((got[..., 16:].view(torch.int16) != 0).any()) or not bool(torch.isfinite(got.float()).all()):
        return float("inf")
    return f16_ulp_diff(got[..., :16], taehv_prep_restated(z, dtype=torch.float64)[..., :16])


# ====================================================================================================== the CPU tests
@pytest.mark.parametrize("n,ldp,rows", SOFTMAX_SHAPES)
def test_softmax_restatement_and_torch_softmax_stay_inside_the_acceptance(n, ldp, rows):
    for dist in SOFTMAX_DISTS:
        s = softmax_scores(dist, n, min(rows, 64))
        p = torch.zeros(s.shape[0], ldp, dtype=torch.float16)
        p[:, :n] = torch.softmax(s[:, :n].float(), dim=-1).half()
        assert softmax_violation(p, s, n) <= 1, dist
        assert softmax_violation(softmax_restated(s, n, ldp), s, n) <= 1, dist


@pytest.mark.parametrize("slip", SOFTMAX_SLIPS)
def test_softmax_slips_break_the_acceptance(slip):
    worst = {}
    for n, ldp, rows in SOFTMAX_SHAPES:
        for dist in SOFTMAX_DISTS:
            s = softmax_scores(dist, n, min(rows, 32))
            worst[(n, dist)] = softmax_violation(softmax_restated(s, n, ldp, slip), s, n)
    if slip == "wave0_max":                                      # a wrong maximum only shows where exp() overflows
        assert worst[(6240, "max_wave3")] >= 10 and worst[(6240, "mixed_extreme")] >= 10, worst
        return
    assert worst[(6240, "gauss3")] >= 10 and worst[(2056, "gauss3")] >= 10, worst      # the production shape and the 8-column tail
    # today's only shape (n = 96: wave 0 holds everything, one trip) cannot see the reduction and trip slips
    if slip in ("wave0_sum",):
        assert worst[(96, "gauss3")] <= 1, worst


def test_softmax_wave0_max_is_invisible_without_overflow():
    """Why max_wave3 puts its maximum 120 above: softmax is shift-invariant, a wrong maximum only matters through overflow."""
    s = softmax_scores("peaked", 6240, 16)
    assert softmax_violation(softmax_restated(s, 6240, 6272, "wave0_max"), s, 6240) <= 1


@pytest.mark.parametrize("C", [96, 192, 384])
def test_rmsnorm_restatement_inside_and_slips_outside_the_acceptance(C):
    for npix in rms_npix_cases(C)[:5]:
        for scale in (1.0, 1e-3, 200.0):
            x, gamma = rms_inputs(C, npix, scale)
            for silu in (0, 1):
                assert rms_violation(rms_restated(x, gamma, silu), x, gamma, silu) <= 1, (npix, scale, silu)
    x, gamma = rms_inputs(C, 6240, 200.0)
    assert rms_violation(rms_restated(x, gamma, 1, "fp16_squares"), x, gamma, 1) >= 10
    x, gamma = rms_inputs(C, 6240, 1.0)
    assert rms_violation(rms_restated(x, gamma, 0, "no_floor"), x, gamma, 0) >= 10


def test_attention_regimes():
    """The peaked regime is peaked (score standard deviation about 6 on the fp64 reference), the init regime is not."""
    for h, w in ATTN_SIZES[:3]:
        x = attn_input(h, w)
        sd = {r: float(attn_reference64(x, attn_weights(r))[1].std()) for r in ATTN_REGIMES}
        assert sd["init"] < 0.5 and 4.0 <= sd["peaked"] <= 9.0, sd


@pytest.mark.parametrize("h,w", ATTN_SIZES[:3])
@pytest.mark.parametrize("regime", ATTN_REGIMES)
def test_attention_e16_is_not_degenerate(h, w, regime):
    x, W = attn_input(h, w), attn_weights(regime)
    ref, _ = attn_reference64(x, W)
    e16 = attn_errors(attn_restated16(x, attn_native_weights(W)), ref)
    branch = float((ref - x.double()).abs().max())      # size of the attention output itself (y - identity)
    branch_l2 = float((ref - x.double()).norm() / ref.norm())
    print(f"attention {h}x{w} {regime}: e16 rel_l2 {e16[0]:.3e} max_abs {e16[1]:.3e}; attention branch rel_l2 {branch_l2:.3e} max_abs {branch:.3e}")
    assert 0 < e16[0] < branch_l2 / 4 and 0 < e16[1] < branch / 4
    v, _, _ = attn_violation(attn_restated16(x, attn_native_weights(W)), x, W)
    assert v <= 0.5 + 1e-9


@pytest.mark.parametrize("slip", ATTN_SLIPS)
def test_attention_slips_break_the_acceptance(slip):
    """Each slip against the case of the GPU test that is there to catch it: pad columns in both regimes, the bias slips in the
    large-bv run, the scale in the peaked regime (in the init regime the softmax is nearly uniform whatever the scale)."""
    cases = {"pad_counted": [("init", None), ("peaked", None)], "bv_omitted": [("init", ATTN_BV_CONST)],
             "bv_twice": [("init", ATTN_BV_CONST)], "q_scale_twice": [("peaked", None)]}[slip]
    for h, w in ATTN_SIZES[:2]:
        for regime, bv in cases:
            x, W = attn_input(h, w), attn_weights(regime, bv_const=bv)
            v, err, e16 = attn_violation(attn_restated16(x, attn_native_weights(W), slip=slip), x, W)
            print(f"{slip} {h}x{w} {regime} bv={bv}: violation {v:.1f} err {err} e16 {e16}")
            assert v >= 10, (slip, h, w, regime, v)


def test_attention_bias_in_front_of_the_softmax_weights_is_not_observable():
    """`bv` folded into V^T (in front of the softmax weights) instead of behind P V is NOT a fault this suite can or should see:
    the two differ by bv * (sum_j P_ij - 1), and a row of fp16-rounded P sums to 1 within a relative 2^-11, so the difference
    stays below one fp16 ulp of o = P V + bv, which is stored in fp16 either way - for every bv, small or large.  What the
    large-bv run does pin is that bv arrives exactly once (bv_omitted, bv_twice above)."""
    for regime in ATTN_REGIMES:
        for h, w in ATTN_SIZES[:2]:
            x, W = attn_input(h, w), attn_weights(regime, bv_const=ATTN_BV_CONST)
            v, _, _ = attn_violation(attn_restated16(x, attn_native_weights(W), slip="bv_before_softmax"), x, W)
            assert v <= 1, (regime, h, w, v)


@pytest.mark.parametrize("hw", PREP_HW)
def test_prep_restatement_and_slips(hw):
    for identity in (True, False):
        z, mean, std, w2, b2 = prep_inputs(hw, identity)
        assert prep_violation(prep_restated(z, 1, mean, std, w2, b2), z, 1, mean, std, w2, b2, identity) <= (0 if identity else 1)
    z, mean, std, w2, b2 = prep_inputs(hw, True)
    # the fp64 reference of the de-normalisation, unrounded.  The fp16 chain rounds std, 1 / std, the quotient, mean and the sum:
    # at most 4 * 2^-11 of |z * std| + |mean|
    zs, m = z[1].double() * torch.tensor(VAE_STD, dtype=torch.float64)[:, None], torch.tensor(VAE_MEAN, dtype=torch.float64)[:, None]
    got = prep_restated(z, 1, mean, std, w2, b2)[:, :16].t().double()
    assert _ratio((got - (zs + m)).abs(), 2.0 ** -9 * (zs.abs() + m.abs())) <= 1
    for slip in ("prep_no_round_div", "prep_t_ignored"):
        n_bad = prep_violation(prep_restated(z, 1, mean, std, w2, b2, slip), z, 1, mean, std, w2, b2, True)
        assert n_bad >= 10, (slip, n_bad)


def test_final_restatement_and_slips():
    T, in_hw, hw, skip = 4, 24 * 64, 16 * 64, 5 * 64
    x = final_inputs(T, in_hw)
    ref = final_restated(x, hw, skip)
    assert ref.shape == (T, 3, hw) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) == 1.0
    assert torch.equal(ref, x[:, skip:skip + hw, :3].double().clamp(-1, 1).permute(0, 2, 1).float())
    assert int((ref.view(torch.int32) == -2 ** 31).sum()) > 0            # -0 passes through the clamp as -0
    for slip in ("skip_ignored", "no_clamp"):
        assert bits_mismatch(final_restated(x, hw, skip, slip), ref) >= 10, slip


def test_upsample_cache_restatement_and_slips():
    buf = upsample_inputs(4096)
    ref = upsample_restated(buf)
    c1, x = buf[1].double(), buf[2]
    assert bits_mismatch(ref[0], torch.where(c1 == 0, torch.zeros_like(x), x)) == 0 and bits_mismatch(ref[1:], buf[[2, 2]]) == 0
    sub = (c1 != 0) & (c1.abs() < 2.0 ** -14)
    assert int(sub.sum()) > 100 and bits_mismatch(ref[0][sub], x[sub]) == 0       # subnormals are not zero
    for slip in ("where_on_x", "neg_zero_not_zero"):
        assert bits_mismatch(upsample_restated(buf, slip), ref) >= 10, slip


def test_enc_prep_restatement_and_slips():
    frames = enc_prep_inputs(7, 1000)
    ref = enc_prep_restated(frames, 2, 4)
    assert ref.shape == (4, 1000, 32) and float(ref[..., 3:].abs().max()) == 0
    assert torch.equal(ref[1, :, 2], frames[2, 3]) and torch.equal(ref[3, :, 0], frames[0, 5])
    assert bits_mismatch(enc_prep_restated(frames, 2, 4, "t0_ignored"), ref) >= 10


def test_enc_final_restatement_and_slips():
    T, hw, Tout, tout = 2, 500, 5, 2
    for identity in (True, False):
        x, w1, b1, mean, std = enc_final_inputs(T, hw, identity)
        mu0 = torch.full((16, Tout, hw), float("nan")).half()
        got, _ = enc_final_restated(x, w1, b1, mean, std, mu0, tout)
        assert enc_final_violation(got, x, w1, b1, mean, std, mu0, tout, identity) <= (0 if identity else 1)
        if identity:
            exact = (x[..., :16].double() - torch.tensor(VAE_MEAN, dtype=torch.float64)) / torch.tensor(VAE_STD, dtype=torch.float64)
            d = (got[:, tout:tout + T].double().permute(1, 2, 0) - exact).abs()
            assert float(d.max()) <= 4e-3 and bool(torch.isnan(got[:, :tout]).all()) and bool(torch.isnan(got[:, tout + T:]).all())
            for slip in ("final_no_round_sub", "tout_ignored"):
                bad, _ = enc_final_restated(x, w1, b1, mean, std, mu0, tout, slip)
                assert enc_final_violation(bad, x, w1, b1, mean, std, mu0, tout, True) >= 10, slip


def test_taehv_prep_restatement_and_slips():
    z = taehv_prep_inputs(3, 777)
    assert taehv_prep_violation(taehv_prep_restated(z), z) <= 1
    assert float(taehv_prep_restated(z).float().abs().max()) == 3.0
    assert taehv_prep_violation(taehv_prep_restated(z, "no_clamp"), z) >= 10


# ------------------------------------------------------------------------------------------------------ the library
def test_library_exports_vae_unit_symbols():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.declared_symbols(lab=False) and hasattr(lib, s), s
        restype, argtypes = _lib.PROTOTYPES[s]
        assert getattr(lib, s).restype is restype and list(getattr(lib, s).argtypes) == argtypes, s
    P, ldp = 60 * 104, 6272
    need = 2 * (P * P + P * ldp + 4 * P * 384 + 384 * ldp)
    assert need <= lib.rtv_vae_attn_arena_bytes(60, 104) <= need + 16 * 256
    assert lib.rtv_vae_attn_arena_bytes(0, 104) == 0 and lib.rtv_vae_attn_arena_bytes(7, 9) == 0


def test_unit_entries_refuse_bad_arguments_on_the_host():
    """Null pointers and out-of-range sizes are refused before anything is launched (no GPU is touched)."""
    import realtime_video_amd.vae_decoder as vd
    lib = _lib.load()
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)
    attn = vd._Attn()
    bad = [lib.rtv_vae_mid_attention(ctypes.byref(attn), p, ctypes.c_void_p(8192), 8, 12, p, 1 << 30, null),      # null weights
           lib.rtv_vae_mid_attention(None, p, p, 8, 12, p, 1 << 30, null),
           lib.rtv_vae_prep(p, 2, 2, 96, p, p, p, p, p, null),                 # t == T
           lib.rtv_vae_prep(p, 2, 0, 0, p, p, p, p, p, null),
           lib.rtv_vae_prep(p, 2, 0, 96, p, p, p, p, ctypes.c_void_p(4100), null),
           lib.rtv_vae_final(p, p, 1, 64, 96, 40, null),                        # window beyond the frame
           lib.rtv_vae_final(p, p, 1, 64, 96, -1, null),
           lib.rtv_vae_final(null, p, 1, 64, 96, 0, null),
           lib.rtv_vae_upsample_cache_t1(p, 0, null),
           lib.rtv_vae_upsample_cache_t1(null, 64, null),
           lib.rtv_vae_enc_prep(p, 4, 2, 3, 64, p, null),                       # t0 + T > Ttot
           lib.rtv_vae_enc_prep(p, 4, -1, 1, 64, p, null),
           lib.rtv_vae_enc_final(p, 2, 64, p, p, p, p, p, 2, 1, null),          # tout + T > Tout_tot
           lib.rtv_vae_enc_final(p, 1, 64, p, null, p, p, p, 2, 0, null),
           lib.rtv_taehv_prep(p, 0, 64, p, null),
           lib.rtv_taehv_prep(p, 1, 64, null, null)]
    assert all(b != 0 for b in bad), bad
    assert lib.rtv_last_error()


def test_vae_glue_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    r = subprocess.run([hipcc, "--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-O3", "-std=c++17", "-fPIC", "-c",
                        os.path.join(CSRC, "vae_decode.hip"), "-o", str(tmp_path / "vae_decode.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch), r.stderr[-4000:]
    for k in ("rmsnorm_silu_cl_kernel", "softmax_rows_kernel", "upsample_cache_t1_kernel", "vae_prep_kernel", "vae_final_kernel",
              "vae_enc_prep_kernel", "vae_enc_final_kernel"):
        hit = [s for n, s in zip(names, scratch) if k in n]
        assert hit and all(s == 0 for s in hit), (k, list(zip(names, scratch)))
