"""Restatement of the OCP Microscaling Formats (MX) v1.0 conversion to MXFP6 (e2m3) with the floor rule - the arithmetic of
`enable_mxfp6()` (include/rtv_hip_mxfp6.h) - in plain torch, evaluated in float64 by search over the value table (no bit tricks):

    per block of 32 consecutive elements of the last dim
    amax = max |x|                e = clamp(floor(log2 amax) - 2, -127, 127)      (an all-zero block: e = -127, codes 0)
    code = e2m3(x * 2^-e)         nearest of the 32 magnitudes k / 8 (k < 8), (1 + m / 8) 2^eps (eps = 0..2); ties to the even
                                  code; saturating at 7.5
    y[m,n] = bf16(sum_k dq(x)[m, k] dq(w)[n, k] + bias[n])      dq = code value * 2^e

The reference has no FP6 path: this is no reference mode, and the native kernels are pinned to this restatement.  A model-level
test installs it with `monkeypatch.setattr(wan_oracle, "fp8_linear", mx_linear)` and `weights[wan_oracle.FP8_FLAG] = True`, as
tests/mxfp4_oracle.py is installed.  The packers are the Python twin of the header's storage macros; the structured inputs of the
quantiser tests and the exact GEMM cases live here too, so that the CPU tests vet exactly what the GPU tests run."""
import torch

import mx_oracle
from mx_oracle import BLOCK, mx_dequantize, product_fp64   # (the shared restatement; re-exported)

BLOCK_BYTES = 24
# magnitude of code c (the 6-bit code is sign << 5 | c; c = exponent field << 3 | mantissa)
E2M3 = tuple(m / 8 if ex == 0 else (1 + m / 8) * 2.0 ** (ex - 1) for ex in range(4) for m in range(8))
_FMT = mx_oracle.Format(E2M3, wrap_from=7.75)         # without saturation [7.75, 8] rounds to 8, whose 5-bit magnitude code wraps to 0
_EVEN_FIRST, _LARGE_FIRST = _FMT.even_first, _FMT.large_first
# mx_quantize -> (code values in {0, +-1/8, ..., +-7.5} as float64, shape of t; block exponents e as int64 [..., K / 32]);
# every term of an exact_case product is a multiple of 2^-8 (two multiples of 1/8, scaled by >= 2^-2)
mx_quantize, mx_linear, exact_case = _FMT.mx_quantize, _FMT.mx_linear, _FMT.exact_case


# ------------------------------------------------------------------------------------------ storage (rtv_hip_mxfp6.h)
def scale_pos(b):
    """RTV_MXFP6_SCALE_POS: the byte of block b inside its row of scales."""
    return (b & ~3) | ((b & 1) << 1) | ((b & 3) >> 1)


def scale_bytes(k):
    """RTV_MXFP6_SCALE_BYTES"""
    return ((k // BLOCK) + 3) & ~3


def code_bytes(k):
    """RTV_MXFP6_CODE_BYTES"""
    return k // 4 * 3


def code_bit(k):
    """RTV_MXFP6_CODE_BIT: the first bit of element k inside its row of codes."""
    return k * 6


def sextets(values):
    """code values -> 6-bit codes (sign << 5 | magnitude code) as uint8; -0 and +0 both become 0 (they are the same code for every
    comparison)."""
    a = values.abs()
    mag = torch.zeros(values.shape, dtype=torch.uint8, device=values.device)
    for c, v in enumerate(E2M3):
        mag = torch.where(a == v, torch.full_like(mag, c), mag)
    return torch.where((values < 0), mag | 32, mag)


def pack_sextets(s):
    """6-bit codes uint8 [M, K] -> uint8 [M, 3 K / 4]: a row is one little-endian bit string, element k at bits [6 k, 6 k + 6) - four
    elements in three bytes.  (A block of 32 is then the 24 bytes [24 b, 24 b + 24), the header's statement.)"""
    q = s.reshape(*s.shape[:-1], s.shape[-1] // 4, 4).to(torch.int32)
    word = q[..., 0] | (q[..., 1] << 6) | (q[..., 2] << 12) | (q[..., 3] << 18)
    out = torch.stack([word & 255, (word >> 8) & 255, (word >> 16) & 255], dim=-1).to(torch.uint8)
    return out.reshape(*s.shape[:-1], s.shape[-1] // 4 * 3).contiguous()


def pack_codes(values):
    """[M, K] code values -> uint8 [M, 3 K / 4] in the header's storage."""
    return pack_sextets(sextets(values))


def unpack_codes(codes, canonical=True):
    """uint8 [M, 3 K / 4] -> 6-bit codes [M, K]; canonical: the code 32 (-0) reads as 0."""
    t = codes.reshape(*codes.shape[:-1], codes.shape[-1] // 3, 3).to(torch.int32)
    word = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)
    s = torch.stack([(word >> (6 * j)) & 63 for j in range(4)], dim=-1).to(torch.uint8)
    s = s.reshape(*codes.shape[:-1], codes.shape[-1] // 3 * 4)
    return torch.where(s == 32, torch.zeros_like(s), s) if canonical else s


def code_values(s):
    """6-bit codes -> their values as float64"""
    val = torch.tensor(E2M3, dtype=torch.float64, device=s.device)[(s & 31).long()]
    return torch.where((s & 32) != 0, -val, val)


def pack_scales(e):
    """block exponents int64 [M, K / 32] -> uint8 [M, RTV_MXFP6_SCALE_BYTES(K)] in the header's order (unowned bytes 0)."""
    return mx_oracle.pack_scales(e, scale_pos, scale_bytes)


# ------------------------------------------------------------------------------------------ test inputs
# the exact ties of e2m3: odd multiples of 1/16 below 1 (between two subnormals, or 15/16 between 7/8 and 1), of 1/16 in [1, 2) as
# well (the first binade shares the subnormals' spacing of 1/8), then of 1/8 in [2, 4) and of 1/4 in [4, 7.5)
TIES = tuple(k / 16 for k in range(1, 32, 2)) + tuple(2 + k / 8 for k in range(1, 16, 2)) + tuple(4 + k / 4 for k in range(1, 14, 2))


def structured_rows(M, d, seed=0):
    """bf16 [M, d] whose 32-element blocks cycle through five kinds, each scaled by 2^e with e running from -100 to +100 over
    the blocks of the matrix (so the block exponent the format derives is e):
      0  exact ties and their negatives (a window of 15 of the 31, moving with the block), small multiples of 1/32, a maximum of
         -7.0 (not a tie)
      1  a maximum in (7.5, 8): 7.75 (the tie with 8, saturates to 7.5) or -7.625 or 7.875, values in (7.5, 8) of both signs
      2  all zeros
      3  normal random values with a maximum in [4, 8)
      4  ties and small values whose maximum is exactly 4, a power of two
    """
    g = torch.Generator().manual_seed(seed)
    nb = d // BLOCK
    total = M * nb
    ties = torch.tensor(TIES, dtype=torch.float64)
    x = torch.zeros(total, BLOCK, dtype=torch.float64)
    for i in range(total):
        kind = 3 if i == total - 1 else i % 5          # (the last block carries e = +100: never the all-zero kind)
        if kind in (0, 4):
            fill = torch.randint(-64, 65, (BLOCK,), generator=g).double() / 32         # |.| <= 2
            lim = len(TIES) if kind == 0 else 24                                       # kind 4: ties below 4 only
            pick = (torch.arange(15) + 7 * (i // 5)) % lim
            sign = torch.where(torch.arange(15) % 2 == (i // 5) % 2, -1.0, 1.0).double()
            fill[:15] = ties[pick] * sign
            fill[15:30] = -fill[:15]
            fill[30] = -7.0 if kind == 0 else 4.0
            x[i] = fill[torch.randperm(BLOCK, generator=g)]
        elif kind == 1:
            fill = torch.randint(-56, 57, (BLOCK,), generator=g).double() / 8          # |.| <= 7
            fill[0] = (7.75, -7.625, 7.875)[(i // 5) % 3]
            fill[1], fill[2], fill[3], fill[4] = 7.5, -7.5625, 7.25, -7.75 if (i // 5) % 3 == 2 else -7.375
            x[i] = fill[torch.randperm(BLOCK, generator=g)]
        elif kind == 3:
            fill = torch.randn(BLOCK, generator=g).clamp(-3.9, 3.9)
            fill[int(torch.randint(0, BLOCK, (1,), generator=g))] = 4.0 + 3.9 * float(torch.rand(1, generator=g))
            x[i] = fill
        e = -100 + (200 * i) // (total - 1)
        x[i] = torch.ldexp(x[i], torch.tensor(e))
    return x.reshape(M, d).to(torch.bfloat16)
