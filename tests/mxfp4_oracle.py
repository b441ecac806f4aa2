"""Restatement of the OCP Microscaling Formats (MX) v1.0 conversion to MXFP4 with the floor rule - the arithmetic of
`enable_mxfp4()` (include/rtv_hip_mxfp4.h) - in plain torch, evaluated in float64 by search over the value table (no bit tricks):

    per block of 32 consecutive elements of the last dim
    amax = max |x|                e = clamp(floor(log2 amax) - 2, -127, 127)      (an all-zero block: e = -127, codes 0)
    code = e2m1(x * 2^-e)         nearest of 0, 0.5, 1, 1.5, 2, 3, 4, 6; ties to the even code; saturating at 6
    y[m,n] = bf16(sum_k dq(x)[m, k] dq(w)[n, k] + bias[n])      dq = code value * 2^e

The reference has no FP4 path: this is no reference mode, and the native kernels are pinned to this restatement.  A model-level
test installs it with `monkeypatch.setattr(wan_oracle, "fp8_linear", mx_linear)` and `weights[wan_oracle.FP8_FLAG] = True`, as
tests/fp8_rows_oracle.py is installed.  The packers are the Python twin of the header's storage macros; the structured inputs of the
quantiser tests and the exact GEMM cases live here too, so that the CPU tests vet exactly what the GPU tests run."""
import torch

import mx_oracle
from mx_oracle import BLOCK, mx_dequantize, product_fp64   # (the shared restatement; re-exported)

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)       # magnitude of code c (the nibble is sign << 3 | c)
_FMT = mx_oracle.Format(E2M1, wrap_from=7.0)          # without saturation [7, 8] rounds to 8, whose 3-bit magnitude code wraps to 0
_EVEN_FIRST, _LARGE_FIRST = _FMT.even_first, _FMT.large_first
# mx_quantize -> (code values in {0, +-0.5, ..., +-6} as float64, shape of t; block exponents e as int64 [..., K / 32])
mx_quantize, mx_linear, exact_case = _FMT.mx_quantize, _FMT.mx_linear, _FMT.exact_case


# ------------------------------------------------------------------------------------------ storage (rtv_hip_mxfp4.h)
def scale_pos(b):
    """RTV_MXFP4_SCALE_POS: the byte of block b inside its row of scales."""
    return (b & ~7) | ((b & 1) << 2) | ((b & 7) >> 1)


def scale_bytes(k):
    """RTV_MXFP4_SCALE_BYTES"""
    return ((k // BLOCK) + 7) & ~7


def nibbles(values):
    """code values -> nibbles (sign << 3 | magnitude code) as uint8; -0 and +0 both become 0 (they are the same code for every
    comparison)."""
    a = values.abs()
    mag = torch.zeros(values.shape, dtype=torch.uint8, device=values.device)
    for c, v in enumerate(E2M1):
        mag = torch.where(a == v, torch.full_like(mag, c), mag)
    return torch.where((values < 0), mag | 8, mag)


def pack_codes(values):
    """[M, K] code values -> uint8 [M, K / 2]: element 2j in the low nibble of byte j."""
    n = nibbles(values)
    return (n[..., 0::2] | (n[..., 1::2] << 4)).contiguous()


def unpack_nibbles(codes, canonical=True):
    """uint8 [M, K / 2] -> nibbles [M, K]; canonical: the nibble 8 (-0) reads as 0."""
    n = torch.stack([codes & 15, codes >> 4], dim=-1).reshape(*codes.shape[:-1], codes.shape[-1] * 2)
    return torch.where(n == 8, torch.zeros_like(n), n) if canonical else n


def pack_scales(e):
    """block exponents int64 [M, K / 32] -> uint8 [M, RTV_MXFP4_SCALE_BYTES(K)] in the header's order (unowned bytes 0)."""
    return mx_oracle.pack_scales(e, scale_pos, scale_bytes)


# ------------------------------------------------------------------------------------------ test inputs
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def structured_rows(M, d, seed=0):
    """bf16 [M, d] whose 32-element blocks cycle through four kinds, each scaled by 2^e with e running from -100 to +100 over
    the blocks of the matrix (so the block exponent the format derives is e):
      0  the seven exact ties and their negatives and small multiples of 1/8; every other one without the 5s, its maximum
         exactly 4 (a power of two)
      1  a maximum of 7.5 or -7.25 (amax / 2^e in (6, 8): saturates), values in (6, 8) of both signs, multiples of 1/4
      2  all zeros
      3  normal random values with a maximum in [4, 8)
    """
    g = torch.Generator().manual_seed(seed)
    nb = d // BLOCK
    total = M * nb
    x = torch.zeros(total, BLOCK, dtype=torch.float64)
    for i in range(total):
        kind = 3 if i == total - 1 else i % 4          # (the last block carries e = +100: never the all-zero kind)
        if kind == 0:
            fill = torch.randint(-16, 17, (BLOCK,), generator=g).double() / 8          # |.| <= 2
            fill[:7] = torch.tensor(TIES)
            fill[7:14] = -torch.tensor(TIES)
            if i % 8 == 0:
                fill[6], fill[13], fill[14] = 0.75, -2.5, 4.0      # no 5: the maximum is 4, an exact power of two
            else:
                fill[14] = -4.0                                    # the maximum is the tie at 5
            x[i] = fill[torch.randperm(BLOCK, generator=g)]
        elif kind == 1:
            fill = torch.randint(-24, 25, (BLOCK,), generator=g).double() / 4          # |.| <= 6
            fill[0] = 7.5 if i % 8 == 1 else -7.25
            fill[1], fill[2], fill[3] = 6.5, -7.0, 7.0
            x[i] = fill[torch.randperm(BLOCK, generator=g)]
        elif kind == 3:
            fill = torch.randn(BLOCK, generator=g).clamp(-3.9, 3.9)
            fill[int(torch.randint(0, BLOCK, (1,), generator=g))] = 4.0 + 3.9 * float(torch.rand(1, generator=g))
            x[i] = fill
        e = -100 + (200 * i) // (total - 1)
        x[i] = torch.ldexp(x[i], torch.tensor(e))
    return x.reshape(M, d).to(torch.bfloat16)
