"""Restatement of the block Hadamard rotation in front of the MXFP4 / MXFP6 quantisers (include/rtv_hip_mx_rotate.h; the arithmetic
of `enable_mxfp4(rotate=True)` / `enable_mxfp6(rotate=True)`) in plain torch:

    per block of 32 consecutive elements of the last dim, index k = 0..31, inputs bf16
    1. the values as fp32
    2. for b = 0, 1, 2, 3, 4 in this order: (u, v) -> (u + v, u - v) on every pair (k, k | 1 << b) with bit b of k clear - fp32
       adds and subtracts (torch's float32 `+` / `-`: IEEE round to nearest even, one operation each, nothing fused)
    3. times 2^-shift (exact): SHIFT_ACT for activations, SHIFT_WEIGHT for weights; 2^-3 * 2^-2 = 1 / 32 undoes H H^T = 32 I
    4. the fp32 results through the format's unchanged floor rule (mx_oracle.Format.mx_quantize evaluates any fp32 input in float64)

`fmt` below is a format's oracle module (mxfp4_oracle or mxfp6_oracle).  The mutants are the errors a kernel can make; the CPU tests
show that the inputs of the GPU tests tell each from the restatement."""
import torch
import torch.nn.functional as F

from mx_oracle import BLOCK, mx_dequantize

SHIFT_ACT, SHIFT_WEIGHT = 3, 2          # RTV_MX_ROT_ACT_SHIFT, RTV_MX_ROT_WEIGHT_SHIFT

MUTANTS = ("index", "shift", "swap")    # (a) k = 4 j + lane for 8 lane + j; (b) the shift off by one; (c) (u - v, u + v) in stage 3
_LANE_MAJOR = torch.tensor([4 * (p & 7) + (p >> 3) for p in range(BLOCK)])     # position p = 8 lane + j -> the mutant's k = 4 j + lane


def rotate32(x, shift, mutant=None):
    """x [..., K] (K % 32 == 0) -> float32 [..., K]: every block through the five butterfly stages, then times 2^-shift."""
    if x.shape[-1] % BLOCK:
        raise ValueError("the last dim must be a multiple of 32")
    assert mutant is None or mutant in MUTANTS
    v = x.detach().float().reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK).clone()
    if mutant == "index":
        w = torch.empty_like(v)
        w[..., _LANE_MAJOR] = v                                        # w[k'] = v[p]: the butterflies then pair what the mutant pairs
        v = w
    for b in range(5):
        lo = torch.tensor([k for k in range(BLOCK) if not (k >> b) & 1])
        hi = lo | (1 << b)
        u, w = v[..., lo], v[..., hi]
        s, d = u + w, u - w                                            # float32, one rounding each
        if mutant == "swap" and b == 3:
            s, d = d, s
        v = torch.empty_like(v)
        v[..., lo], v[..., hi] = s, d
    if mutant == "index":
        v = v[..., _LANE_MAJOR]
    v = v * 2.0 ** -(shift + (mutant == "shift"))                      # exact: a power of two, no fp32 subnormals in the tests' range
    return v.reshape(x.shape)


def mx_quantize_rot(fmt, x, shift, mutant=None):
    """-> fmt.mx_quantize's (code values, block exponents) of the rotated x"""
    return fmt.mx_quantize(rotate32(x, shift, mutant))


def mx_linear_rot(fmt):
    """nn.Linear on rotated operands of the format, for monkeypatch.setattr(wan_oracle, "fp8_linear", ...): activations at
    SHIFT_ACT, weights at SHIFT_WEIGHT, so the product needs no rescaling."""
    def linear(x, weight, bias, shards=1):
        xq = mx_dequantize(*mx_quantize_rot(fmt, x, SHIFT_ACT)).float()
        wq = mx_dequantize(*mx_quantize_rot(fmt, weight, SHIFT_WEIGHT)).float()
        y = F.linear(xq, wq)
        if bias is not None:
            y = y + bias.float()
        return y.to(x.dtype)
    return linear


def product_operands(seed=2024):
    """The operands of the error table (M, N, K = 64, 96, 512): Gaussian activations, weights 0.05 x Gaussian, bf16."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(64, 512, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(96, 512, generator=g)).to(torch.bfloat16)
    return x, w


def outlier_columns(x, factor=32.0):
    """x [M, K] with every 32nd column times `factor` (one outlier channel per block), rounded to bf16"""
    y = x.detach().double().clone()
    y[:, ::BLOCK] *= factor
    return y.to(torch.bfloat16)


def outlier_rows(fmt, M, d, seed=0):
    """bf16 [M, d]: fmt.structured_rows(M, d, seed) with its block scales 2^e compressed from e in [-100, 100] to [-50, 50], and with
    three of every seven blocks (global block index i % 7 = 1, 3, 5) replaced by
      1  Gaussian with one outlier, times 32, whose place moves with the block (every lane and register of a quad gets one)
      3  a block that spans 20 binades: magnitudes m * 2^q, m in [1, 2), q covering -10 .. +10 - fp32 rounds inside the butterflies,
         so the order of the stages shows; every other one of them is a probe of three values on which the pinned order and
         the order of the index mutant round to different codes (see below)
      5  alternately an all-zero block and a block of one non-zero value (its place moves too)
    each scaled by a power of two in 2^-30 .. 2^30.  Every magnitude is zero or within [2^-60, 2^60] (smaller ones of the
    structured rows are set to zero): no butterfly can overflow or reach an fp32 subnormal."""
    g = torch.Generator().manual_seed(seed + 1000)
    nb = d // BLOCK
    total = M * nb
    x = fmt.structured_rows(M, d, seed).double().reshape(total, BLOCK)
    for i in range(total):
        e = -100 + (200 * i) // (total - 1)                            # structured_rows' scale of block i
        x[i] = torch.ldexp(x[i], torch.tensor(e // 2 - e))
        kind = i % 7
        if kind not in (1, 3, 5):
            continue
        n = i // 7
        if kind == 1:
            fill = torch.randn(BLOCK, generator=g)
            fill[n % BLOCK] *= 32
        elif kind == 3 and n % 2:
            # the stage-order probe: a = 1 at k0, b = -(1 - 2^-p) beside it (k0 ^ 1, stage 0), c = 2^-26 at k0 ^ 8 (stage 3).  In the
            # pinned order a + b = 2^-p is exact and c survives: the outputs are 2^-p +- c and about 2.  A kernel that runs stage 3
            # first computes fl(1 +- c) = 1 and loses c: 2^-p exactly.  The block maximum is in [1, 2) x 2^1, so the outputs scale to
            # 4 (2^-p +- c): with p = 4 the tie 0.25 of e2m1, with p = 6 the tie 1/16 of e2m3 - c decides the code.
            fill = torch.zeros(BLOCK, dtype=torch.float64)
            k0 = (3 * n) % BLOCK
            fill[k0], fill[k0 ^ 1], fill[k0 ^ 8] = 1.0, -(1 - 2.0 ** -(4 if n % 4 == 1 else 6)), 2.0 ** -26
        elif kind == 3:
            q = torch.randint(-10, 11, (BLOCK,), generator=g)
            pos = torch.randperm(BLOCK, generator=g)
            q[pos[0]], q[pos[1]] = -10, 10
            m = 1 + torch.randint(0, 128, (BLOCK,), generator=g).double() / 128
            sign = torch.where(torch.rand(BLOCK, generator=g) < 0.5, -1.0, 1.0).double()
            fill = sign * torch.ldexp(m, q)
        else:
            fill = torch.zeros(BLOCK, dtype=torch.float64)
            if n % 2:
                fill[(5 * n) % BLOCK] = (-1.0) ** n * (1 + (n % 8) / 8)
        x[i] = torch.ldexp(fill.double(), torch.tensor(-30 + (60 * i) // (total - 1)))
    x = x.to(torch.bfloat16).double()
    x = torch.where(x.abs() < 2.0 ** -60, torch.zeros_like(x), x)
    return x.reshape(M, d).to(torch.bfloat16)
