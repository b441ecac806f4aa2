"""Restatement of torchao's Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()) - the arithmetic of
`enable_fp8("row")` - with the conventions oracle/wan_oracle.fp8_linear uses for the per-tensor granularity:

    s_x[m] = max(max_k |x[m, k]|, 1e-12) * fp32(1 / 448)        one scale per activation row
    s_w[n] = the same over row n of W                            one scale per weight row (output channel)
    q(t)   = e4m3fn(clamp(t / s, -448, 448))                     round to nearest even, evaluated in fp32
    y[m,n] = bf16(acc[m, n] * s_x[m] * s_w[n] + bias[n])         products accumulated in fp32

torchao is not part of the reference tree (third-party, unpinned): PARITY WITH torchao ITSELF IS UNPINNED for this granularity as
for the other; the native kernels are pinned to this restatement.  A model-level test installs it with
`monkeypatch.setattr(wan_oracle, "fp8_linear", fp8_rows_linear)` and `weights[wan_oracle.FP8_FLAG] = True`: the oracle's `_linear`
and `_qkv` look `fp8_linear` up as a module global."""
import torch
import torch.nn.functional as F

FP8_MAX = 448.0


def fp8_row_scales(t):
    """fp32 scales [..., 1] of the rows (last dim) of `t`, as torch evaluates `amax / 448.0` on the GPU: a multiplication by the
    fp32 reciprocal (oracle/wan_oracle._fp8_scale does the same for the whole tensor)."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(FP8_MAX, dtype=torch.float32)
    return t.detach().float().abs().amax(dim=-1, keepdim=True).clamp(min=1e-12) * inv.to(t.device)


def fp8_rows_quantize(t):
    """-> (e4m3 codes as a float8_e4m3fn tensor, fp32 scales [..., 1])."""
    s = fp8_row_scales(t)
    return (t.float() / s).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn), s


def fp8_rows_linear(x, weight, bias, shards=1):
    """nn.Linear under per-row fp8 scales.  `shards` (the row sharding of a context-parallel forward) is accepted and ignored:
    the arithmetic of a row needs that row alone, so every sharding computes the same thing."""
    xq, sx = fp8_rows_quantize(x)
    wq, sw = fp8_rows_quantize(weight)
    y = F.linear(xq.float(), wq.float()) * sx * sw.reshape(-1)
    if bias is not None:
        y = y + bias.float()
    return y.to(x.dtype)
