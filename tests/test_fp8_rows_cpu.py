"""CPU-only tests of the fp8 mode with per-row scales (enable_fp8("row"), include/rtv_hip_fp8_rows.h): the restatement the GPU
tests pin the kernels to (tests/fp8_rows_oracle.py) against an element-by-element definition, the generated binding, the
workspace size and the keyword's argument check."""
import ctypes
import math
import struct

import pytest
import torch

from fp8_rows_oracle import fp8_rows_linear, fp8_rows_quantize

# every finite e4m3fn value >= 0 (OCP: 4 exponent bits, bias 7, 3 mantissa bits, no infinities, 448 the largest), by its code
_E4M3 = [(m / 8 * 2.0 ** -6) if e == 0 else (1 + m / 8) * 2.0 ** (e - 7) for e in range(16) for m in range(8)][:127]


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _e4m3_rne(v):
    """Nearest e4m3fn value of a double (ties to the even code), saturating - by search over the table, no bit tricks."""
    a = min(abs(v), 448.0)
    best = min(range(127), key=lambda c: (abs(_E4M3[c] - a), c & 1))
    return math.copysign(_E4M3[best], v)


def test_restatement_matches_the_element_by_element_definition():
    g = torch.Generator().manual_seed(0)
    M, N, K = 5, 8, 64
    x = torch.randn(M, K, generator=g)
    x[1] = 0                                                     # an all-zero row: scale 1e-12 / 448, codes 0
    x[2] = -x[2].abs()
    x[2, 7] = -9.0                                               # a row whose maximum (in magnitude) is negative
    x[3] = torch.randn(K, generator=g) * 2.0 ** -130             # a row of bf16 subnormals (below 2^-126)
    x = x.to(torch.bfloat16)
    assert 0 < float(x[3].float().abs().max()) < 2.0 ** -126
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16)

    inv = _f32(1.0 / 448.0)

    def scale(row):
        return _f32(max(max(abs(float(v)) for v in row), _f32(1e-12)) * inv)

    def quant(row, s):
        return [_e4m3_rne(_f32(float(v) / s)) for v in row]      # the quotient is rounded to fp32 before the e4m3 rounding

    sx, sw = [scale(r) for r in x], [scale(r) for r in w]
    xq, wq = [quant(r, s) for r, s in zip(x, sx)], [quant(r, s) for r, s in zip(w, sw)]
    cq, cs = fp8_rows_quantize(x)
    assert [float(s) for s in cs.reshape(-1)] == sx
    assert cq.float().tolist() == xq
    assert sx[1] == _f32(_f32(1e-12) * inv) and all(v == 0 for v in xq[1])
    assert all(v == 0 for v in xq[3])                            # subnormal inputs under the clamped scale: zeros
    assert xq[2][7] == -448.0

    got = fp8_rows_linear(x, w, bias)
    assert got.dtype == torch.bfloat16 and torch.equal(got, fp8_rows_linear(x, w, bias, shards=2))
    for m in range(M):
        for n in range(N):
            acc = sum(a * b for a, b in zip(xq[m], wq[n]))       # exact in a double: 64 products of two e4m3 values
            y = _f32(_f32(_f32(acc) * sx[m]) * sw[n]) + float(bias[n])
            want = torch.tensor(y, dtype=torch.float32).to(torch.bfloat16)
            # fp32 accumulation order is free: one bf16 ulp of the result
            assert abs(float(got[m, n]) - float(want)) <= 2.0 ** -7 * abs(float(want)) + 1e-5, (m, n)


def test_binding_has_the_row_mode():
    from realtime_video_amd import _lib
    P = _lib.FP8_ROWS_PROTOTYPES
    assert set(P) == {"rtv_quantize_fp8_rows", "rtv_layernorm_modulate_fp8_rows", "rtv_gemm_fp8_rows"}
    assert P["rtv_gemm_fp8_rows"][1][4:6] == [ctypes.c_void_p, ctypes.c_void_p]      # const float* a_row_scales, w_row_scales
    assert P["rtv_quantize_fp8_rows"][1][1] is ctypes.c_int64 and P["rtv_quantize_fp8_rows"][1][5] is ctypes.c_int64
    fields = [n for n, _ in _lib.STRUCTS["rtv_dit_weights"]._fields_]
    assert fields[-2:] == ["fp8_scales", "fp8_row_scales"]                           # appended at the end of the struct
    assert dict(_lib.STRUCTS["rtv_dit_weights"]._fields_)["fp8_row_scales"] is ctypes.POINTER(ctypes.c_void_p)
    assert _lib.ABI_VERSION >= 105
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_workspace_holds_the_row_scales():
    from realtime_video_amd import _lib
    lib = _lib.load()
    Cfg = _lib.STRUCTS["rtv_dit_config"]
    F, gh, gw, text_len = 3, 30, 52, 512
    sizes = {}
    for mode in (0, 1, 2):
        cfg = Cfg(dim=1536, ffn_dim=8960, num_heads=12, num_layers=2, freq_dim=256, text_dim=4096, text_len=text_len, in_dim=16,
                  out_dim=16, eps=1e-6, use_fp8=mode, max_attn_kv_splits=0)
        sizes[mode] = lib.rtv_dit_workspace_bytes(ctypes.byref(cfg), F, gh, gw)
    rows = max(F * gh * gw, text_len)
    assert sizes[0] < sizes[1]
    assert sizes[2] >= sizes[1] + rows * 4


def test_enable_fp8_refuses_an_unknown_granularity():
    from realtime_video_amd.causal_model import CausalWanModel
    model = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=128, device="cpu")
    with pytest.raises(ValueError, match="granularity"):
        model.enable_fp8(granularity="bogus")
