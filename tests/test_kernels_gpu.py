"""Per-kernel parity tests on the MI355X: every call goes through the C ABI (ctypes -> librtv_hip.so).

References: the CPU oracle (oracle/wan_oracle.py, pinned to the upstream reference by
tests/test_oracle_vs_golden.py), golden vectors minted from the reference, and — for these floating
point kernels — a plain torch fp32 restatement of the same op evaluated on the GPU.
Tolerances (bf16): attention atol 2e-2 on unit-variance data; GEMM / elementwise outputs within
2 bf16 ulp of the eager-chain reference (rel-L2 <= 4e-3).

What the attention bars of this file can and cannot see: q, k and v are iid unit Gaussians, so the scores are about N(0, 1),
the softmax is diffuse and a row of the output has a standard deviation of about sqrt(e / Lkv) - 0.017 at 9360 keys, 0.05 at
1000.  One key carries a weight of about 1 / Lkv, so a key masked one position off, a row read from just outside the window or
a counted key counted n +- 1 times moves the output by 1e-3 or less: far inside max_abs <= 2e-2 (which is a whole standard
deviation of the output at 9360 keys).  These cases pin shapes, strides, dispatch and the bit-equalities between the kernels;
the single-key errors are the business of tests/test_attention_peaked_gpu.py, whose inputs make every row's answer hang on one
or two known keys and whose one bar, |out - ref| <= 4 u (P @ |V|) + 1e-6 against the fp64 definition, follows from the kernels'
arithmetic (tests/attn_cases.py; the Gaussian data of this file under that bar: family i there).
"""
import math

import pytest
import torch

from conftest import max_abs, rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


def _randn(*shape, seed=0, dtype=torch.bfloat16, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


# ----------------------------------------------------------------------------------------- probes
def test_probe_mfma_layout():
    import ctypes
    from realtime_video_amd import _lib
    a, b = _randn(32, 16, seed=1), _randn(16, 32, seed=2)
    d = torch.zeros(32, 32, dtype=torch.float32, device=DEV)
    _lib.call("rtv_probe_mfma", ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()),
              ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    ref = a.float() @ b.float()
    assert max_abs(d, ref) <= 1e-4, "MFMA 32x32x16 operand/result lane map differs from the kernels' assumption"


@pytest.mark.parametrize("kbk,s", [(0, 0), (1, 1)])
def test_probe_transpose_read(kbk, s):
    import ctypes
    from realtime_video_amd import _lib
    v = torch.arange(64 * 128, dtype=torch.int16).view(64, 128).to(DEV)
    out = torch.zeros(4, 64, 8, dtype=torch.int16, device=DEV)
    _lib.call("rtv_probe_tr", ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(out.data_ptr()), kbk, s,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    exp = torch.zeros_like(out)
    kbase = kbk * 32 + s * 16
    for db in range(4):
        for lane in range(64):
            g = lane >> 5
            for j in range(8):
                row = kbase + 4 * g + (j if j < 4 else 8 + j - 4)
                exp[db, lane, j] = v[row, db * 32 + (lane & 31)]
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), exp.cpu()), "ds_read_b64_tr_b16 gather differs from the attention kernel's assumption"


# ----------------------------------------------------------------------------------------- GEMM
def _gemm_ref(a, w, bias, act, gate, rows_per_frame, residual):
    """Eager-chain reference with the reference's rounding points, fp32 math on the GPU."""
    dt = a.dtype
    y = a.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    y = y.to(dt)
    if act == 1:
        y = torch.nn.functional.gelu(y.float(), approximate="tanh").to(dt)
    elif act == 2:
        y = torch.nn.functional.silu(y.float()).to(dt)
    if gate is not None:
        f = torch.arange(a.shape[0], device=a.device) // rows_per_frame
        y = (y.float() * gate[f].float()).to(dt)
    if residual is not None:
        y = (residual.float() + y.float()).to(dt)
    return y


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("M,N,K", [(4680, 1536, 1536), (200, 64, 256), (3, 1536, 256), (585, 4608, 1536),
                                   (4680, 256, 64)])
def test_gemm_bias(ops, M, N, K, cfg):
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    out = ops.gemm(a, w, bias=b, tile_cfg=cfg)
    ref = _gemm_ref(a, w, b, 0, None, 0, None)
    assert rel_l2(out, ref) <= 4e-3
    assert max_abs(out, ref) <= 0.05 * float(ref.float().abs().max()) + 1e-3


@pytest.mark.parametrize("act", [1, 2])
def test_gemm_activation(ops, act):
    M, N, K = 1000, 512, 1536
    a, w, b = _randn(M, K, seed=4), _randn(N, K, seed=5, scale=K ** -0.5), _randn(N, seed=6, scale=0.1)
    out = ops.gemm(a, w, bias=b, act=act)
    ref = _gemm_ref(a, w, b, act, None, 0, None)
    assert rel_l2(out, ref) <= 4e-3


def test_gemm_gate_residual_inplace(ops):
    """self-attention output projection epilogue: x += (y + b) * e[2][frame] (causal_model.py:476)."""
    M, N, K, fs = 3 * 520, 256, 256, 520
    a, w, b = _randn(M, K, seed=7), _randn(N, K, seed=8, scale=K ** -0.5), _randn(N, seed=9, scale=0.1)
    emod = _randn(3, 6, N, seed=10)            # [F, 6, d]; gate = chunk 2
    x = _randn(M, N, seed=11)
    ref = _gemm_ref(a, w, b, 0, emod[:, 2], fs, x)
    xin = x.clone()
    out = ops.gemm(a, w, bias=b, gate=emod[0, 2], gate_stride=6 * N, rows_per_frame=fs, residual=xin, out=xin)
    assert out.data_ptr() == xin.data_ptr()
    assert rel_l2(out, ref) <= 4e-3
    # residual only (cross-attention output projection, causal_model.py:480)
    ref2 = _gemm_ref(a, w, b, 0, None, 0, x)
    out2 = ops.gemm(a, w, bias=b, residual=x)
    assert rel_l2(out2, ref2) <= 4e-3


def test_gemm_fp16(ops):
    M, N, K = 777, 384, 384
    a, w = _randn(M, K, seed=1, dtype=torch.float16), _randn(N, K, seed=2, dtype=torch.float16, scale=K ** -0.5)
    out = ops.gemm(a, w)
    ref = (a.float() @ w.float().t()).half()
    assert rel_l2(out, ref) <= 1e-3


@pytest.mark.parametrize("cfg", [0, 5, 7])
@pytest.mark.parametrize("M,N,K", [(4680, 5120, 1024), (4680, 13824, 512), (2400, 7680, 2048), (585, 5120, 5120)])
def test_gemm_split_k_tail_round(ops, M, N, K, cfg):
    """tile_cfg 5: the tiles of the last partial round are split along K over several workgroups and reduced in-launch
    (agent-scope release/acquire + arrival counter).  Repeated launches reuse the workspace."""
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    ref = _gemm_ref(a, w, b, 1, None, 0, None)
    for _ in range(8):   # repeated launches: race screen of the DMA / barrier schedule and of the split-K hand-off
        out = ops.gemm(a, w, bias=b, act=1, tile_cfg=cfg)
        assert rel_l2(out, ref) <= 4e-3
        assert max_abs(out, ref) <= 0.05 * float(ref.float().abs().max()) + 1e-3


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("M,N,K", [(4680, 1536, 512), (777, 264, 64), (130, 5128, 128), (1560, 512, 192), (585, 1536, 320)])
def test_gemm_epilogue_through_lds_all_fusions(ops, M, N, K, cfg):
    """Every fused epilogue (bias / GELU / SiLU / per-frame gate + residual in place / residual only) through the LDS-staged
    coalesced store path of every tile config, ragged M and N edges, K of 1..3 K-tiles (pipeline prologue / tail), and the
    narrow fallback (output rows not 16-byte aligned: a column slice of a wider buffer).  Repeated launches must be
    bit-identical (race screen of the DMA / barrier schedule)."""
    fs = (M + 2) // 3
    a, w, b = _randn(M, K, seed=7), _randn(N, K, seed=8, scale=K ** -0.5), _randn(N, seed=9, scale=0.1)
    emod = _randn(3, 6, N, seed=10)
    x = _randn(M, N, seed=11)
    for act, gate, res in [(0, False, False), (1, False, False), (2, False, True), (0, True, True)]:
        ref = _gemm_ref(a, w, b, act, emod[:, 2] if gate else None, fs, x if res else None)
        outs = []
        for rep in range(3):
            xin = x.clone()
            out = ops.gemm(a, w, bias=b, act=act, gate=emod[0, 2] if gate else None, gate_stride=6 * N,
                           rows_per_frame=fs if gate else 0, residual=xin if res else None, out=xin if res else None,
                           tile_cfg=cfg)
            outs.append(out.clone())
        assert rel_l2(outs[0], ref) <= 4e-3, (act, gate, res)
        assert max_abs(outs[0], ref) <= 0.05 * float(ref.float().abs().max()) + 1e-3
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        # narrow path: ldc = N + 4 keeps 8-byte but not 16-byte row alignment -> same values through the direct store
        wide = torch.zeros(M, N + 4, dtype=torch.bfloat16, device=DEV)
        narrow = ops.gemm(a, w, bias=b, act=act, gate=emod[0, 2] if gate else None, gate_stride=6 * N,
                          rows_per_frame=fs if gate else 0, residual=x if res else None, out=wide[:, :N], tile_cfg=cfg)
        assert torch.equal(narrow, outs[0]) and float(wide[:, N:].abs().max()) == 0


def test_gemm_fp16_epilogue_large_tile(ops):
    """fp16 operands through the 256x256 kernel (tile_cfg 4) and its LDS epilogue with a fused residual (VAE usage)."""
    M, N, K = 1000, 384, 384
    a, w = _randn(M, K, seed=1, dtype=torch.float16), _randn(N, K, seed=2, dtype=torch.float16, scale=K ** -0.5)
    b, r = _randn(N, seed=3, dtype=torch.float16, scale=0.1), _randn(M, N, seed=4, dtype=torch.float16)
    ref = ((a.float() @ w.float().t() + b.float()).half().float() + r.float()).half()
    for cfg in (1, 4):
        assert rel_l2(ops.gemm(a, w, bias=b, residual=r, tile_cfg=cfg), ref) <= 1e-3


def test_gemm_rejects_bad_arguments(ops):
    a, w = _randn(64, 100), _randn(64, 100)
    with pytest.raises(RuntimeError):
        ops.gemm(a, w)  # K not a multiple of 64
    with pytest.raises(RuntimeError):
        ops.gemm(torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16))  # CPU tensors


# ----------------------------------------------------------------------------------------- attention
def _attn_ref(q, k, v, kv_limit=None):
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if kv_limit is not None:
        idx = torch.arange(k.shape[1], device=q.device).view(1, 1, 1, -1)
        s = s.masked_fill(idx >= kv_limit.view(1, 1, -1, 1), float("-inf"))
    return (torch.softmax(s, -1) @ vf).transpose(1, 2).contiguous()


def test_attention_golden_vs_reference(ops, golden):
    g = golden("ops.pt")
    out = ops.attn_fwd(g["attn_q"].to(DEV), g["attn_k"].to(DEV), g["attn_v"].to(DEV))
    assert out.shape == g["attn_out"].shape and out.dtype == torch.bfloat16 and out.is_contiguous()
    assert max_abs(out.cpu(), g["attn_out"]) <= 2e-2   # upstream SDPA-fallback output
    from oracle import wan_oracle as wo
    gold = wo.attention_math(g["attn_q"], g["attn_k"], g["attn_v"])
    err_ours, err_ref = max_abs(out.cpu(), gold), max_abs(g["attn_out"], gold)
    assert err_ours <= max(2 * err_ref, 1e-2)


@pytest.mark.parametrize("Lq,Lkv,H", [(4680, 9360, 4), (585, 9360, 3), (4680, 512, 2), (4680, 4680, 1),
                                      (256, 64, 8), (1, 1, 1), (257, 65, 1), (100, 1000, 16)])
def test_attention_shapes_strided_cache(ops, Lq, Lkv, H):
    """K/V are strided views of a larger cache (causal_model.py:386-390)."""
    q = _randn(1, Lq, H, 128, seed=1)
    cache_k = _randn(1, Lkv + 77, H, 128, seed=2)
    cache_v = _randn(1, Lkv + 77, H, 128, seed=3)
    k, v = cache_k[:, 5:5 + Lkv], cache_v[:, 5:5 + Lkv]
    out = ops.attn_fwd(q, k, v)
    ref = _attn_ref(q, k, v)
    assert max_abs(out, ref) <= 2e-2
    assert rel_l2(out, ref) <= 1e-2


def test_attention_batch_and_fp16(ops):
    q = _randn(2, 300, 2, 128, seed=1, dtype=torch.float16)
    k = _randn(2, 333, 2, 128, seed=2, dtype=torch.float16)
    v = _randn(2, 333, 2, 128, seed=3, dtype=torch.float16)
    out = ops.attn_fwd(q, k, v)
    assert max_abs(out, _attn_ref(q, k, v)) <= 4e-3


@pytest.mark.parametrize("S,block,q_offset", [(1040, 520, 0), (1560, 520, 0), (700, 256, 0), (300, 128, 128)])
def test_attention_block_causal(ops, S, block, q_offset):
    """KV-recompute mask kv < ends[q] (causal_model.py:108-141, :339-348)."""
    Lkv = S + q_offset
    q = _randn(1, S, 2, 128, seed=1)
    k, v = _randn(1, Lkv, 2, 128, seed=2), _randn(1, Lkv, 2, 128, seed=3)
    lim = torch.clamp(((torch.arange(S, device=DEV) + q_offset) // block + 1) * block, max=Lkv)
    out = ops.attn_fwd(q, k, v, causal_block=block, q_offset=q_offset)
    assert max_abs(out, _attn_ref(q, k, v, lim)) <= 2e-2


def test_attention_outlier_keys_rescale_path(ops):
    """Forces large running-max jumps at late tiles (online-softmax rescale correctness)."""
    Lq, Lkv = 256, 640
    q, k, v = _randn(1, Lq, 1, 128, seed=1), _randn(1, Lkv, 1, 128, seed=2), _randn(1, Lkv, 1, 128, seed=3)
    k[0, 300, 0] = q[0, 17, 0] * 6.0      # huge logit for row 17 in tile 4
    k[0, 639, 0] = q[0, 200, 0] * 9.0     # and for row 200 in the last tile
    out = ops.attn_fwd(q, k, v)
    assert max_abs(out, _attn_ref(q, k, v)) <= 3e-2
    assert torch.isfinite(out.float()).all()


def test_attention_rejects_bad_arguments(ops):
    q = _randn(1, 8, 2, 64)
    with pytest.raises(RuntimeError):
        ops.attn_fwd(q, q, q)  # head_dim != 128


# ----------------------------------------------------------------------------------------- elementwise
# What the row-kernel bars of this section can and cannot see: the rows are iid Gaussians and the bar is a whole-tensor
# rel-L2 <= 3e-3 against the bf16 eager chain (plus a cap on the fraction of elements that differ at all).  That pins the
# bf16 ROUNDING POINTS - a kernel that skips round_bf16(x * r) differs in a fifth of its elements - and the shapes the forward
# uses.  It cannot see a reduction that loses a chunk, a lane column or a wave's partial (at d = 5120 one 8-element chunk is
# 0.16 % of sum x^2, 0.08 % of every output, a fifth of a bf16 unit roundoff), one RoPE pair on the wrong axis, one row with its
# neighbouring frame's modulation (a few wrong elements add less than 3e-3 to the rel-L2), a one-pass variance (zero-mean rows
# are well conditioned) or a misplaced eps (var = 4); and it never sets row_offset > 0, ldx != ldo != d, a head_dim that does not
# divide 512, or a width at a boundary of the chunk loops.  Those are the business of tests/test_row_kernels_gpu.py: rows in
# which each chunk in turn carries the sum, offset, near-constant, constant, tiny, huge and mixed-magnitude rows, per-frame
# tables that tell frames apart, every element against the fp64 definition under a bar derived from the kernel's rounding
# points (tests/row_cases.py; the Gaussian data of this section under that bar: family `gaussian` there).
def test_layernorm_modulate_matches_eager_chain(ops):
    """(norm1(x).unflatten(F, fs) * (1 + e[1]) + e[0]).flatten(1, 2), causal_model.py:471."""
    F_, fs, d = 3, 520, 1536
    x = _randn(F_ * fs, d, seed=1, scale=2.0)
    emod = _randn(F_, 6, d, seed=2, scale=0.5)
    out = ops.layernorm_modulate(x, 1e-6, shift=emod[0, 0], scale=emod[0, 1], frame_stride=6 * d, rows_per_frame=fs)
    n = torch.nn.functional.layer_norm(x, (d,), None, None, 1e-6)
    ref = (n.view(F_, fs, d) * (1 + emod[:, 1:2]) + emod[:, 0:1]).view(F_ * fs, d)
    assert ref.dtype == torch.bfloat16
    assert rel_l2(out, ref) <= 3e-3
    # plain and affine LayerNorm (norm3, causal_model.py:424-426)
    wgt, b = _randn(d, seed=3) * 0.1 + 1, _randn(d, seed=4) * 0.1
    assert rel_l2(ops.layernorm_modulate(x, 1e-6), n) <= 3e-3
    ref3 = torch.nn.functional.layer_norm(x, (d,), wgt, b, 1e-6)
    assert rel_l2(ops.layernorm_modulate(x, 1e-6, weight=wgt, bias=b), ref3) <= 3e-3


@pytest.mark.parametrize("d", [256, 1536, 5120])
def test_rmsnorm_matches_oracle(ops, d):
    from oracle import wan_oracle as wo
    x, wgt = _randn(37, d, seed=1, scale=3.0), (_randn(d, seed=2) * 0.1 + 1)
    out = ops.rmsnorm(x, wgt, 1e-6)
    ref = wo.rms_norm(x.cpu(), wgt.cpu(), 1e-6)
    assert rel_l2(out.cpu(), ref) <= 3e-3
    assert (out.cpu() != ref).float().mean() <= 0.02  # bit-identical except rare rounding ties


def _rope_cs(hd):
    from realtime_video_amd.rope import rope_cos_sin_table
    return rope_cos_sin_table(hd).to(DEV)


@pytest.mark.parametrize("d,H,grid,start,row0", [(256, 2, (2, 6, 8), 3, 10), (1536, 12, (1, 30, 52), 5, 0),
                                               (5120, 40, (1, 6, 8), 0, 7), (8192, 64, (1, 3, 5), 2, 1)])
@pytest.mark.parametrize("form", [0, 1])
def test_qk_norm_rope_cache_matches_oracle(ops, d, H, grid, start, row0, form):
    """RMSNorm(q,k) -> RoPE -> KV-cache write, causal_model.py:243-256, :143-171, :380-385 - both forms of the kernel (one 256-thread
    workgroup per row: launches of few rows; two waves per row, r04: the full-size launches - chosen by row count in production,
    forced here through include/rtv_hip_lab.h)."""
    from oracle import wan_oracle as wo
    from realtime_video_amd import _lib
    M = grid[0] * grid[1] * grid[2]
    hd = d // H
    qkv = _randn(M, 3 * d, seed=1, scale=2.0)
    wq, wk = _randn(d, seed=2) * 0.1 + 1, _randn(d, seed=3) * 0.1 + 1
    kc = torch.zeros(M + 20, H, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    _lib.load().rtv_rope_set_wave(form)
    try:
        q = ops.qk_norm_rope_cache(qkv, kc, vc, row0, H, wq, wk, _rope_cs(hd), grid, start)
    finally:
        _lib.load().rtv_rope_set_wave(-1)
    c = qkv.cpu()
    freqs = wo.rope_table(hd)
    rq = wo.rope_apply(wo.rms_norm(c[:, :d], wq.cpu()).view(1, M, H, hd), grid, freqs, start)
    rk = wo.rope_apply(wo.rms_norm(c[:, d:2 * d], wk.cpu()).view(1, M, H, hd), grid, freqs, start)
    assert rel_l2(q.cpu().view(1, M, H, hd), rq) <= 3e-3
    assert rel_l2(kc[row0:row0 + M].cpu(), rk[0]) <= 3e-3
    assert torch.equal(vc[row0:row0 + M].cpu().view(M, d), c[:, 2 * d:])
    # rows outside the written window stay untouched
    assert float(kc[:row0].abs().sum()) == 0 and float(kc[row0 + M:].abs().sum()) == 0
    assert (q.cpu().view(1, M, H, hd) != rq).float().mean() <= 0.03


def test_qk_norm_rope_cache_forms_are_bit_identical(ops):
    """The RoPE / cache kernel has two forms chosen by the launch's row count (one workgroup per row for the few rows of a
    context-parallel token shard, two waves per row for full-size launches).  They sum a row's squares in ONE canonical order, so the
    form never shows in the bits - a sharded forward stays bit-identical with the unsharded one.  d = 256 ... 8192, ragged widths."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    try:
        for d, H, grid in ((5120, 40, (1, 9, 13)), (1536, 12, (2, 5, 7)), (256, 2, (1, 4, 5)), (8192, 64, (1, 2, 3)), (1024, 8, (1, 6, 6))):
            M, hd = grid[0] * grid[1] * grid[2], d // H
            qkv = _randn(M, 3 * d, seed=d, scale=3.0)
            wq, wk = _randn(d, seed=2) * 0.1 + 1, _randn(d, seed=3) * 0.1 + 1
            outs = []
            for form in (0, 1):
                lib.rtv_rope_set_wave(form)
                kc = torch.zeros(M + 4, H, hd, dtype=torch.bfloat16, device=DEV)
                vc = torch.zeros_like(kc)
                q = ops.qk_norm_rope_cache(qkv, kc, vc, 2, H, wq, wk, _rope_cs(hd), grid, 1)
                outs.append((q.clone(), kc, vc))
            for a, b in zip(*outs):
                assert torch.equal(a, b), (d, H)
    finally:
        lib.rtv_rope_set_wave(-1)


def test_modulation_table_and_sinusoid(ops):
    from oracle import wan_oracle as wo
    mod, e0 = _randn(4, 6, 256, seed=1), _randn(3, 6, 256, seed=2)
    out = ops.modulation_table(mod, e0)
    ref = mod.unsqueeze(1) + e0.unsqueeze(0)
    assert torch.equal(out, ref)
    hm, e = _randn(1, 2, 256, seed=3), _randn(3, 1, 256, seed=4)
    assert torch.equal(ops.modulation_table(hm, e), hm.unsqueeze(1) + e.unsqueeze(0))
    t = torch.tensor([1000.0, 908.8427, 713.9794, 0.0], device=DEV)
    sin = ops.sinusoidal_embedding(t, 256)
    ref = wo.sinusoidal_embedding_1d(256, t.cpu()).to(torch.bfloat16)
    assert max_abs(sin.cpu(), ref) <= 2 ** -7


def test_patchify_unpatchify(ops):
    from oracle import wan_oracle as wo
    C, F_, gh, gw = 16, 3, 6, 8
    x = _randn(C, F_, 2 * gh, 2 * gw, seed=1)
    rows = ops.patchify(x, gh, gw)
    wgt = _randn(32, C, 1, 2, 2, seed=2)
    ref = torch.nn.functional.conv3d(x.float().unsqueeze(0), wgt.float(), stride=(1, 2, 2))
    got = rows.float() @ wgt.float().flatten(1).t()
    assert max_abs(got.t().reshape(ref.shape), ref) <= 1e-3
    tok = _randn(F_ * gh * gw, 64, seed=3)
    out = ops.unpatchify(tok, 16, F_, gh, gw)
    assert torch.equal(out.cpu(), wo.unpatchify(tok.cpu(), (F_, gh, gw)))


def test_attention_rows_independent_of_wave_grouping(ops):
    """Token sharding changes which query rows share a wave.  A row's result must not depend on it (context-parallel ==
    unsharded, bit for bit): the lazy softmax rescale is decided per row.  Keys grow in magnitude along the sequence so
    that rescales do fire after the first tiles."""
    g = torch.Generator().manual_seed(11)
    Lq, Lkv, H = 600, 1024, 2
    q = (torch.randn(1, Lq, H, 128, generator=g) * 2).to(torch.bfloat16).to(DEV)
    ramp = torch.linspace(0.2, 6.0, Lkv).view(1, Lkv, 1, 1)
    k = (torch.randn(1, Lkv, H, 128, generator=g) * ramp).to(torch.bfloat16).to(DEV)
    v = torch.randn(1, Lkv, H, 128, generator=g).to(torch.bfloat16).to(DEV)
    full = ops.attn_fwd(q, k, v)
    for off in (4, 37, 300):
        part = ops.attn_fwd(q[:, off:].contiguous(), k, v)
        assert torch.equal(part, full[:, off:]), off


@pytest.mark.parametrize("causal_block", [0, 96])
def test_attention_128_row_workgroups_equal_256_row_ones(ops, causal_block):
    """The 4-wave build (chosen when the 256-row grid cannot fill the CUs: head-sharded attention under context
    parallelism) computes every row exactly like the 8-wave one; ragged Lq / Lkv and the block-causal prefix included."""
    g = torch.Generator().manual_seed(12)
    Lq, Lkv, H = 333, 1000, 3
    q = (torch.randn(1, Lq, H, 128, generator=g) * 2).to(torch.bfloat16).to(DEV)
    k = (torch.randn(1, Lkv, H, 128, generator=g) * torch.linspace(0.2, 5.0, Lkv).view(1, Lkv, 1, 1)).to(torch.bfloat16).to(DEV)
    v = torch.randn(1, Lkv, H, 128, generator=g).to(torch.bfloat16).to(DEV)
    outs = []
    try:
        for waves in (8, 4, 0):
            ops.attn_set_waves(waves)
            outs.append(ops.attn_fwd(q, k, v, causal_block=causal_block, q_offset=Lkv - Lq if causal_block else 0))
    finally:
        ops.attn_set_waves(0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ----------------------------------------------------------------------------------------- fp8 path
def _fp8_linear_ref(x, w, bias):
    """torchao Float8DynamicActivationFloat8WeightConfig(PerTensor) restated: per-tensor scales max|t|/448, e4m3 operands,
    fp32 products/accumulation, bias added before the bf16 rounding."""
    sx = x.float().abs().max().clamp(min=1e-12) / 448.0
    sw = w.float().abs().max().clamp(min=1e-12) / 448.0
    xq = (x.float() / sx).clamp(-448, 448).to(torch.float8_e4m3fn)
    wq = (w.float() / sw).clamp(-448, 448).to(torch.float8_e4m3fn)
    y = (xq.float() @ wq.float().t()) * (sx * sw)
    if bias is not None:
        y = y + bias.float()
    return y, xq, wq, sx, sw


def test_quantize_fp8_matches_torch_e4m3(ops):
    x = (_randn(1000, 512, seed=5) * 3).contiguous()
    q, s = ops.quantize_fp8(x)
    _, xq, _, sx, _ = _fp8_linear_ref(x, x[:8], None)
    inv448 = torch.tensor(1.0) / torch.tensor(448.0)                         # the restatement's scale, evaluated on the host
    rs = x.cpu().float().abs().max().clamp(min=1e-12) * inv448
    assert float(sx) == float(rs) and torch.equal(s.cpu().view(torch.int32), rs.reshape(1).view(torch.int32))
    assert torch.equal(q.view(torch.uint8), xq.view(torch.uint8))          # same rounding (RNE), same saturation
    z, sz = ops.quantize_fp8(torch.zeros(16, 128, dtype=torch.bfloat16, device=DEV))
    assert float(z.float().abs().max()) == 0 and float(sz) > 0


@pytest.mark.parametrize("M,N,K", [(4680, 5120, 1024), (300, 1536, 256), (2340, 13824, 512), (4680, 2560, 5120)])
def test_gemm_fp8_matches_scaled_mm_restatement(ops, M, N, K):
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    ref, _, wq, _, sw = _fp8_linear_ref(a, w, b)
    for _ in range(3):
        aq, sa = ops.quantize_fp8(a)
        out = ops.gemm_fp8(aq, sa, wq, float(sw), bias=b)
        assert rel_l2(out, ref.to(torch.bfloat16)) <= 4e-3
    # and the fp8 result is close to the bf16 GEMM (quantisation noise of two e4m3 operands)
    assert rel_l2(out, (a.float() @ w.float().t() + b.float())) <= 6e-2


@pytest.mark.parametrize("M,N,K", [(4680, 5120, 5120), (585, 15360, 5120), (300, 1536, 256)])
def test_gemm_fp8_matches_torch_scaled_mm(ops, M, N, K):
    """Independent pin of the fp8 weight path (release_server.py:179-182): torchao's Float8DynamicActivationFloat8WeightConfig
    (PerTensor) quantises with scale = amax / 448, casts to e4m3 and calls `torch._scaled_mm(x_q, w_q.t(), scale_a, scale_b,
    bias, out_dtype=x.dtype)`.  torchao itself is not in the image, but `torch._scaled_mm` - the third-party arithmetic at the
    bottom of that path (hipBLASLt's e4m3 GEMM on gfx950) - is: the same e4m3 bytes and scales go through it and through
    rtv_gemm_fp8.  Products of two e4m3 numbers are exact in fp32, so the two differ only by the fp32 accumulation order and
    the final bf16 rounding: rel-L2 <= 2e-3, max-abs within one bf16 ulp of the largest output."""
    if not hasattr(torch, "_scaled_mm"):
        pytest.skip("torch._scaled_mm not available")
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    aq, sa = ops.quantize_fp8(a)
    sw = (w.float().abs().max().clamp(min=1e-12) * (torch.tensor(1.0) / torch.tensor(448.0)).to(DEV)).reshape(1)
    wq = (w.float() / sw).clamp(-448, 448).to(torch.float8_e4m3fn)
    try:
        ref = torch._scaled_mm(aq, wq.t(), scale_a=sa.reshape(()), scale_b=sw.reshape(()), bias=b, out_dtype=torch.bfloat16)
    except (RuntimeError, TypeError) as e:                  # a build without fp8 GEMM support for this device
        pytest.skip(f"torch._scaled_mm unavailable here: {str(e)[:120]}")
    out = ops.gemm_fp8(aq, sa, wq, float(sw), bias=b)
    assert rel_l2(out, ref) <= 2e-3
    assert max_abs(out, ref) <= 2 ** -7 * float(ref.float().abs().max())


def test_gemm_fp8_fused_epilogue(ops):
    M, N, K, F = 4680, 1536, 1536, 3
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    gate, res = _randn(F, N, seed=4), _randn(M, N, seed=5)
    y, _, wq, _, sw = _fp8_linear_ref(a, w, b)
    yb = y.to(torch.bfloat16)
    g = gate.repeat_interleave(M // F, dim=0)
    ref = res + (yb * g)                                     # bf16(acc+bias) -> * gate -> + residual, as rtv_gemm
    aq, sa = ops.quantize_fp8(a)
    out = ops.gemm_fp8(aq, sa, wq, float(sw), bias=b, gate=gate, gate_stride=N, rows_per_frame=M // F, residual=res)
    assert rel_l2(out, ref) <= 4e-3
    out = ops.gemm_fp8(aq, sa, wq, float(sw), bias=b, act=1)
    assert rel_l2(out, torch.nn.functional.gelu(yb, approximate="tanh")) <= 4e-3


# ----------------------------------------------------------------------------------------- BASELINE config 3 sizes
@pytest.mark.parametrize("name,N,K,act", [("qkv", 15360, 5120, 0), ("o", 5120, 5120, 0), ("ffn0", 13824, 5120, 1),
                                          ("ffn2", 5120, 13824, 0)])
def test_gemm_full_14b_shapes(ops, name, N, K, act):
    """The four projection shapes of the 14B layer at the full token count (M = 4680) against the fp32 eager chain, default
    tile config with split-K workspace attached (the bench's configuration)."""
    ops.ensure_gemm_workspace(torch.device(DEV))
    a, w, b = _randn(4680, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    out = ops.gemm(a, w, bias=b, act=act)
    ref = _gemm_ref(a, w, b, act, None, 0, None)
    assert rel_l2(out, ref) <= 4e-3
    assert max_abs(out, ref) <= 0.05 * float(ref.float().abs().max()) + 1e-3
    # linearity in the activations (size-independent property): (2a) W^T + b - (a W^T + b) == a W^T up to bf16 rounding
    if act == 0:
        out2 = ops.gemm((a.float() * 2).to(a.dtype), w, bias=b)
        lin = (out2.float() - out.float())
        assert rel_l2(lin, (ref.float() - b.float())) <= 1e-2


@pytest.mark.parametrize("Lq,n_real,total,H", [(4680, 64, 512, 4), (300, 1, 512, 2), (257, 200, 512, 3), (100, 63, 70, 1), (585, 64, 65, 2)])
def test_attention_duplicate_key_equals_repeated_keys(ops, Lq, n_real, total, H):
    """rtv_attn_fwd_dup (the text cross-attention without its redundant work, model.py:171-228): a window of n_real keys plus ONE
    key counted (total - n_real) times equals dense attention over the window with that key repeated - mathematically; in floating
    point the two differ by summation order and the bf16 rounding of P: both within the attention tolerance of the fp32 definition,
    and within 4e-3 of each other.  count == 1 is plain attention (bit-identical)."""
    q = _randn(1, Lq, H, 128, seed=1)
    k = _randn(1, n_real + 1, H, 128, seed=2)
    v = _randn(1, n_real + 1, H, 128, seed=3)
    count = total - n_real
    kk = torch.cat([k[:, :n_real], k[:, n_real:].expand(-1, count, -1, -1)], 1).contiguous()
    vv = torch.cat([v[:, :n_real], v[:, n_real:].expand(-1, count, -1, -1)], 1).contiguous()
    full = ops.attn_fwd(q, kk, vv)
    fold = ops.attn_fwd_dup(q, k, v, n_real, count)
    ref = _attn_ref(q, kk, vv)
    assert max_abs(full, ref) <= 2e-2 and max_abs(fold, ref) <= 2e-2
    assert max_abs(fold, full) <= 4e-3 + 1e-2 * float(ref.abs().max()) and rel_l2(fold, full) <= 5e-3
    if count == 1:
        assert torch.equal(fold, full)
    with pytest.raises(RuntimeError):
        ops.attn_fwd_dup(q, k, v, n_real + 1, 3)             # dup_key outside the window


@pytest.mark.parametrize("Lq,Lkv,H,splits,waves", [(4680, 2048, 5, 2, 0), (1100, 3000, 16, 2, 0), (585, 9360, 8, 3, 0), (300, 1000, 5, 4, 4),
                                                   (257, 700, 3, 16, 8), (33, 100, 1, 5, 0), (600, 1500, 2, 2, 82),
                                                   (600, 1500, 2, 2, 840 + 600), (4680, 2048, 5, 2, 840 + 600), (300, 1300, 3, 4, 840 + 200)])
def test_attention_kv_split_matches_unsplit(ops, Lq, Lkv, H, splits, waves):
    """rtv_attn_fwd_split (the self-attention launch of a context-parallel rank, xdit_context_parallel.py:179 in the reference):
    key window cut into `splits` ranges of 64-key tiles, one workgroup per (head, query tile, range), unnormalised fp32 partials
    merged by a second kernel.  Same mathematics as one launch, other fp32 summation order: both within the attention tolerance
    of the fp32 definition and within 2 bf16 ulps of each other; through both kernels (4-wave / 8-wave lockstep, four-phase),
    with a two-range ring window, more splits than key tiles, and splits = 1 (bit-identical with the plain launch)."""
    q = _randn(1, Lq, H, 128, seed=1)
    kc = _randn(1, Lkv + 200, H, 128, seed=2)
    vc = _randn(1, Lkv + 200, H, 128, seed=3)
    ops.attn_set_waves(waves)
    try:
        for seg0, seg1 in (((7, Lkv), (0, 0)), ((150, Lkv - 90), (20, 90))):
            whole = ops.attn_fwd_win(q, kc, vc, seg0, seg1)
            split = ops.attn_fwd_split(q, kc, vc, seg0, seg1, kv_splits=splits)
            one = ops.attn_fwd_split(q, kc, vc, seg0, seg1, kv_splits=1)
            kk = torch.cat([kc[:, seg0[0]:seg0[0] + seg0[1]], kc[:, seg1[0]:seg1[0] + seg1[1]]], 1).contiguous()
            vv = torch.cat([vc[:, seg0[0]:seg0[0] + seg0[1]], vc[:, seg1[0]:seg1[0] + seg1[1]]], 1).contiguous()
            ref = _attn_ref(q, kk, vv)
            assert torch.equal(one, whole)
            assert torch.isfinite(split.float()).all()
            assert max_abs(whole, ref) <= 2e-2 and max_abs(split, ref) <= 2e-2
            assert rel_l2(split, whole) <= 3e-3
            assert max_abs(split, whole) <= 2 ** -7 * float(ref.abs().max())       # 2 ulps of bf16 at the largest magnitude
        # block-causal window (the recompute pass): every workgroup splits its own tile count; rows whose keys inside a range
        # are all masked contribute (m, l, O) = (-1e30, 0, 0)
        Lc = min(Lq, Lkv)
        cb = max(64, (Lc + 2) // 3)
        qc, kq, vq = q[:, :Lc].contiguous(), kc[:, :Lc].contiguous(), vc[:, :Lc].contiguous()
        whole = ops.attn_fwd(qc, kq, vq, causal_block=cb, q_offset=0)
        split = ops.attn_fwd_split(qc, kq, vq, (0, Lc), kv_splits=splits, causal_block=cb, q_offset=0)
        assert torch.isfinite(split.float()).all()
        assert rel_l2(split, whole) <= 3e-3 and max_abs(split, whole) <= 2 ** -7 * float(whole.float().abs().max())
    finally:
        ops.attn_set_waves(0)
    with pytest.raises(RuntimeError):
        ops.attn_fwd_split(q, kc, vc, (0, Lkv), kv_splits=2, workspace=torch.empty(16, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("M,N,K", [(585, 5120, 1024), (585, 15360, 512), (160, 256, 128), (161, 512, 256), (1, 264, 192), (700, 1536, 1536),
                                   (1170, 13824, 256), (37, 200, 320)])
def test_gemm_160_row_one_wave_per_simd_kernel_is_bit_identical(ops, M, N, K):
    """gemm5.hip (r05: 160 x 256 tiles, four waves = one per SIMD, accumulators and fragments in asm-owned accumulation
    registers - the kernel of the context-parallel token shards): tile config 19 (no split-K) accumulates K in the order of the
    256 x 256 ping-pong kernel without split-K (tile config 4) and shares its epilogue - bit-identical for every epilogue kind,
    ragged rows / columns, one-row problems; tile config 9 (K segments where the tiles cannot fill the chip) differs by fp32
    re-association only and is repeatable (fixed summation order)."""
    ops.ensure_gemm_workspace(torch.device(DEV))
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    r = _randn(M, N, seed=4)
    gate = _randn(3, N, seed=5)
    for kw in (dict(bias=b), dict(bias=b, act=1), dict(bias=b, gate=gate, gate_stride=N, rows_per_frame=(M + 2) // 3, residual=r), dict()):
        ref = ops.gemm(a, w, tile_cfg=4, **kw).clone()
        outs = [ops.gemm(a, w, tile_cfg=19, **kw).clone() for _ in range(3)]
        assert torch.equal(outs[0], ref) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        sp = [ops.gemm(a, w, tile_cfg=9, **kw).clone() for _ in range(2)]
        assert torch.equal(sp[0], sp[1]) and rel_l2(sp[0], ref) <= 2e-3


def test_gemm_default_dispatch_takes_the_160_row_kernel_for_token_shards(ops):
    """The default dispatch (tile config 0) at the row counts of 8- and 4-way context parallelism on the 14B's wide projections
    (QKV 15360, ffn-in 13824 columns): one round of 160 x 256 tiles, unsplit - i.e. the bits of tile config 4 - where the
    256- / 128-row kernels would split a tail along K."""
    ops.ensure_gemm_workspace(torch.device(DEV))
    for M, N in ((585, 15360), (585, 13824), (1170, 15360)):
        a, w, b = _randn(M, 1024, seed=1), _randn(N, 1024, seed=2, scale=1024 ** -0.5), _randn(N, seed=3, scale=0.1)
        assert torch.equal(ops.gemm(a, w, bias=b, tile_cfg=0), ops.gemm(a, w, bias=b, tile_cfg=4))


def test_gemm_one_wave_per_simd_config_is_bit_identical(ops):
    """Tile config 8 (gemm4.hip: four waves, 128 x 128 per wave, A by LDS DMA, W through registers) against the production
    ping-pong kernel (config 4) on the layer shapes and ragged ones: same K order per accumulator, same epilogue - bit-identical;
    K must be a multiple of 128 (the K loop runs in pairs of tiles).  An experimental kernel: present in the lab build only
    (make LAB=1, RTV_LIB_PATH=.../librtv_hip_lab.so); the product library must REJECT the configuration (a mistyped
    tile config must not return numbers from a timing experiment)."""
    from realtime_video_amd import _lib
    if not _lib.load().rtv_lab_build():
        for cfg in (8, 81, 86, 91):
            with pytest.raises(RuntimeError):
                ops.gemm(_randn(256, 256, seed=1), _randn(256, 256, seed=2), tile_cfg=cfg)
        return
    for M, N, K, act in ((4680, 5120, 1024, 1), (585, 1536, 5120, 0), (300, 520, 256, 2), (257, 264, 128, 0), (1000, 2048, 1664, 1)):
        a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
        r = _randn(M, N, seed=4)
        assert torch.equal(ops.gemm(a, w, bias=b, act=act, tile_cfg=8), ops.gemm(a, w, bias=b, act=act, tile_cfg=4)), (M, N, K)
        assert torch.equal(ops.gemm(a, w, bias=b, residual=r, tile_cfg=8), ops.gemm(a, w, bias=b, residual=r, tile_cfg=4)), (M, N, K)
    with pytest.raises(RuntimeError):
        ops.gemm(_randn(64, 192, seed=1), _randn(64, 192, seed=2), tile_cfg=8)


def test_gemm_split_k_sum_order_is_fixed(ops):
    """Split-K with more than two K segments per tile (few tiles on 256 CUs: S = 8): the reducer sums the published slabs in index
    order whichever unit arrived last, so repeated launches - and the same GEMM on another rank / GPU - give the same bits.
    40 launches each of three such problems (with an unrelated kernel in between to shuffle the arrival order)."""
    ops.ensure_gemm_workspace(torch.device(DEV))
    for M, N, K, cfg in ((300, 520, 2048, 5), (585, 1536, 5120, 7), (4680, 512, 5120, 5)):
        a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
        first = ops.gemm(a, w, bias=b, tile_cfg=cfg).clone()
        noise = torch.empty(1 << 22, device=DEV)
        for i in range(40):
            if i % 3 == 0:
                noise.normal_()
            assert torch.equal(ops.gemm(a, w, bias=b, tile_cfg=cfg), first), (M, N, K, i)
        ref = (a.float() @ w.float().t() + b.float())
        assert rel_l2(first, ref) <= 1e-2


def test_gemm_half_tile_tail_is_bit_identical_with_the_plain_launch(ops):
    """gemm8's tail round as 128 x 256 half tiles (a tail that split-K would cut in two, K <= 8192: 380 and 1140 tiles on 256 CUs)
    through the 128-row body inside the same kernel: full K per unit, the unsplit summation order - the same bits as the launch
    without it (rtv_gemm_set_half_tail(0), tile config 4 = no split-K either), for both epilogue families and a ragged M."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    try:
        for M, N, K in ((4680, 5120, 1024), (4680, 15360, 512), (4500, 5120, 2048)):
            a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
            r = _randn(M, N, seed=4)
            outs = []
            for on in (1, 0):
                lib.rtv_gemm_set_half_tail(on)
                outs.append((ops.gemm(a, w, bias=b, act=1, tile_cfg=4).clone(), ops.gemm(a, w, bias=b, residual=r, tile_cfg=4).clone()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (M, N, K)
            lib.rtv_gemm_set_half_tail(1)
            assert rel_l2(ops.gemm(a, w, bias=b, tile_cfg=0), a.float() @ w.float().t() + b.float()) <= 1e-2
    finally:
        lib.rtv_gemm_set_half_tail(1)


def test_sampled_event_brackets_count_every_launch(ops):
    """bench.py's roofline block brackets kernel launches with hipEvents (rtv_prof_*).  An event pair costs the launch stream a few
    microseconds, so a class can be bracketed every n-th launch only (rtv_prof_set_stride): the sampled launches carry time and
    work, ALL launches of the class are counted, and the class time is the sampled time scaled by work."""
    a, w = _randn(512, 256, seed=1), _randn(384, 256, seed=2, scale=0.06)
    try:
        ops.prof_reset()
        ops.prof_set_stride("gemm", 3)
        ops.prof_enable(True, ["gemm"])
        for _ in range(10):
            ops.gemm(a, w)
        ops.layernorm_modulate(_randn(64, 256, seed=3))            # another class: not enabled, not counted
        torch.cuda.synchronize()
        r = ops.prof_read("gemm")
        assert r["launches"] == 4 and r["seen_launches"] == 10      # launches 0, 3, 6, 9
        flops = 2.0 * 512 * 384 * 256
        assert abs(r["work"] - 4 * flops) < 1 and abs(r["seen_work"] - 10 * flops) < 1
        assert r["ms"] > 0 and abs(r["ms_class"] - r["ms"] * 2.5) <= 1e-9 * r["ms_class"]
        assert ops.prof_read("layernorm")["seen_launches"] == 0
        ops.prof_reset()
        assert ops.prof_read("gemm")["seen_launches"] == 0
    finally:
        ops.prof_enable(False)
        ops.prof_set_stride("gemm", 1)
        ops.prof_reset()


def test_gemm_ragged_row_strips_are_bit_identical_with_the_plain_launch(ops):
    """r04: where it removes the tail round, a ragged last row of 256-row tiles (M = 4680: 72 real rows) runs as 128 x 512 strips in
    front of the tile grid - two half tiles through the 128-row body, full K (ffn-in: 19 x 54 = 1026 tiles = 4 rounds + 2 split-K
    tiles -> 972 tiles + 27 strips = four rounds, no split).  Same bits as tile config 4 (no strips, no split-K) for both epilogue
    families, an odd column-tile count (a strip of one half tile), 1 / 72 / 128 rows in the last tile; shapes where the rule does
    not apply are unchanged; with the switch off the launch goes back to the round-3 form (split-K tail: fp32 re-association)."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    ops.ensure_gemm_workspace(torch.device(DEV))
    try:
        # 256 CUs: strips apply to 1026 = 4 x 256 + 2 tiles (54 columns), 19 x 27 = 513 = 2 x 256 + 1 (27 columns, odd), not to 380
        for M, N, K in ((4680, 13824, 1024), (4609, 13824, 256), (4736, 13824, 512), (4680, 6912, 1024), (4680, 5120, 1024),
                        (4680, 15360, 512)):
            a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
            r = _randn(M, N, seed=4)
            gate = _randn(3, N, seed=5)
            lib.rtv_gemm_set_ragged_strips(1)
            got = (ops.gemm(a, w, bias=b, act=1, tile_cfg=5).clone(),
                   ops.gemm(a, w, bias=b, gate=gate, gate_stride=N, rows_per_frame=(M + 2) // 3, residual=r, tile_cfg=5).clone())
            ref = (ops.gemm(a, w, bias=b, act=1, tile_cfg=4),
                   ops.gemm(a, w, bias=b, gate=gate, gate_stride=N, rows_per_frame=(M + 2) // 3, residual=r, tile_cfg=4))
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (M, N, K)
            lib.rtv_gemm_set_ragged_strips(0)
            off = ops.gemm(a, w, bias=b, act=1, tile_cfg=5)
            assert rel_l2(off, ref[0]) <= 2e-3, (M, N, K)
    finally:
        lib.rtv_gemm_set_ragged_strips(1)


def test_idle_wave_loops_change_nothing_but_the_time(ops):
    """Waves whose rows lie beyond M (gemm8_kernel) / beyond Lq (four-phase attention) run an idle loop - barriers and DMA duty
    only.  With the switch off they compute on clamped rows and the epilogue masks the result: the outputs must be bit-identical,
    with and without the split-K tail, for row counts that leave one to seven idle waves."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    ops.ensure_gemm_workspace(torch.device(DEV))
    try:
        for M, N, K, cfg in ((4680, 5120, 1024, 5), (4680, 15360, 512, 4), (585, 2560, 640, 5), (300, 1536, 256, 4), (3, 512, 192, 4)):
            a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
            outs = []
            for on in (1, 0):
                lib.rtv_gemm_set_skip_idle(on)
                outs.append(ops.gemm(a, w, bias=b, act=1, tile_cfg=cfg).clone())
            assert torch.equal(outs[0], outs[1]), (M, N, K, cfg)
        for Lq, Lkv, H in ((4680, 2048, 4), (300, 1500, 2), (33, 1100, 3), (1000, 1024, 1)):
            q, k, v = _randn(1, Lq, H, 128, seed=4), _randn(1, Lkv, H, 128, seed=5), _randn(1, Lkv, H, 128, seed=6)
            outs = []
            for kern in (82, W4):                       # the four-phase / the one-wave-per-SIMD kernel whatever the grid size
                ops.attn_set_waves(kern)
                for on in (1, 0):
                    lib.rtv_attn_set_skip_idle(on)
                    outs.append(ops.attn_fwd(q, k, v).clone())
            assert all(torch.equal(outs[0], o) for o in outs[1:]), (Lq, Lkv, H)
            assert max_abs(outs[0], _attn_ref(q, k, v)) <= 2.5e-2
    finally:
        lib.rtv_gemm_set_skip_idle(1)
        lib.rtv_attn_set_skip_idle(1)
        ops.attn_set_waves(0)


def test_attention_full_size_properties(ops):
    """Self-attention at the benchmarked size (4680 queries x 9360 cached keys x 40 heads, the 14B denoise step): (1) against
    the fp32 definition on a sample of heads; (2) invariance under a permutation of the keys (softmax-weighted sums do not
    depend on key order; the online softmax then meets the tile maxima in another order, so this exercises the rescale
    path); (3) duplicating every key/value pair leaves the output unchanged."""
    H, Lq, Lkv = 40, 4680, 9360
    q = _randn(1, Lq, H, 128, seed=1)
    k = _randn(1, Lkv, H, 128, seed=2)
    v = _randn(1, Lkv, H, 128, seed=3)
    out = ops.attn_fwd(q, k, v)
    for h in (0, 17, 39):
        ref = _attn_ref(q[:, :, h:h + 1], k[:, :, h:h + 1], v[:, :, h:h + 1])
        assert max_abs(out[:, :, h:h + 1], ref) <= 2e-2
    perm = torch.randperm(Lkv, generator=torch.Generator().manual_seed(4)).to(DEV)
    out_p = ops.attn_fwd(q, k[:, perm].contiguous(), v[:, perm].contiguous())
    assert rel_l2(out_p, out) <= 5e-3
    hs = slice(0, 8)                                            # duplication on 8 heads (memory)
    k2 = torch.cat([k[:, :, hs], k[:, :, hs]], 1).contiguous()
    v2 = torch.cat([v[:, :, hs], v[:, :, hs]], 1).contiguous()
    out_d = ops.attn_fwd(q[:, :, hs].contiguous(), k2, v2)
    assert rel_l2(out_d, out[:, :, hs]) <= 5e-3


# ----------------------------------------------------------------------------------------- randomized shape sweeps
def test_gemm_random_shape_sweep(ops):
    """40 random problems (ragged M incl. 1, N multiple of 8, K multiple of 64, every epilogue combination, default tile
    config with the split-K workspace attached) against the fp32 eager chain."""
    import random
    ops.ensure_gemm_workspace(torch.device(DEV))
    rng = random.Random(1234)
    for case in range(40):
        M = rng.choice([1, 2, 3, 31, 255, 257, 585, 1170, rng.randint(1, 5000)])
        N = 8 * rng.randint(1, 700)
        K = 64 * rng.randint(1, 40)
        act = rng.choice([0, 0, 1, 2])
        a, w = _randn(M, K, seed=case), _randn(N, K, seed=100 + case, scale=K ** -0.5)
        b = _randn(N, seed=200 + case, scale=0.1) if rng.random() < 0.7 else None
        rpf = rng.choice([1, 7, 1560])
        use_gate = rng.random() < 0.4
        gate = _randn((M + rpf - 1) // rpf, N, seed=300 + case) if use_gate else None
        res = _randn(M, N, seed=400 + case) if rng.random() < 0.4 else None
        out = ops.gemm(a, w, bias=b, act=act, gate=gate, gate_stride=N if use_gate else 0,
                       rows_per_frame=rpf if use_gate else 0, residual=res)
        ref = _gemm_ref(a, w, b, act, gate, rpf, res)
        assert rel_l2(out, ref) <= 5e-3, (case, M, N, K, act, use_gate, res is not None)
        assert max_abs(out, ref) <= 0.05 * float(ref.float().abs().max()) + 1e-2, (case, M, N, K)


def test_attention_random_shape_sweep(ops):
    """30 random problems: ragged Lq / Lkv (incl. 1), 1..5 heads, strided cache views, dense and block-causal with random
    block size / query offset, against the fp32 definition."""
    import random
    rng = random.Random(4321)
    for case in range(30):
        H = rng.randint(1, 5)
        Lq = rng.choice([1, 31, 32, 33, 255, 256, 257, rng.randint(1, 1500)])
        Lkv = rng.choice([1, 63, 64, 65, rng.randint(1, 3000)])
        q = _randn(1, Lq, H, 128, seed=case)
        cache_k, cache_v = _randn(1, Lkv + 9, H, 128, seed=50 + case), _randn(1, Lkv + 9, H, 128, seed=90 + case)
        off = rng.randint(0, 9)
        k, v = cache_k[:, off:off + Lkv], cache_v[:, off:off + Lkv]
        if rng.random() < 0.4 and Lkv >= Lq:
            cb = rng.choice([8, 96, 128, 520])
            q_off = rng.randint(0, Lkv - Lq)
            lim = ((q_off + torch.arange(Lq, device=DEV)) // cb + 1) * cb
            out = ops.attn_fwd(q, k, v, causal_block=cb, q_offset=q_off)
            ref = _attn_ref(q, k, v, kv_limit=lim.clamp(max=Lkv))
        else:
            out = ops.attn_fwd(q, k, v)
            ref = _attn_ref(q, k, v)
        assert max_abs(out, ref) <= 2.5e-2, (case, Lq, Lkv, H)
        assert rel_l2(out, ref) <= 1.2e-2, (case, Lq, Lkv, H)


# ----------------------------------------------------------------------------------------- the plug-in entry points
def test_attention_plugin_entries_run_on_device(ops, golden):
    """The drop-in boundary itself executed on the GPU: `attention(...)` (wan/modules/attention.py:150-212
    contract), the `sageattn_func` stand-in (wan/modules/sage.py:12-19, BHLD) and the registered custom op
    `torch.ops.rtv.attn_fwd`, with K/V as strided views of a K/V-interleaved cache arena (how causal_model.py:386-390
    hands the cache window to the backend), against the reference's own `attention()` output (ops.pt)."""
    from realtime_video_amd import attention as plug
    g = golden("ops.pt")
    q, k, v = (g[n].to(DEV) for n in ("attn_q", "attn_k", "attn_v"))
    Lkv, H = k.shape[1], k.shape[2]
    arena = torch.zeros(1, Lkv + 9, 2, H, 128, dtype=torch.bfloat16, device=DEV)
    arena[:, 4:4 + Lkv, 0], arena[:, 4:4 + Lkv, 1] = k, v
    kc, vc = arena[:, 4:4 + Lkv, 0], arena[:, 4:4 + Lkv, 1]
    assert not kc.is_contiguous()
    before = arena.clone()
    o_attn = plug.attention(q, kc, vc)
    o_op = torch.ops.rtv.attn_fwd(q, kc, vc)
    o_sage = plug.sageattn_func(q.transpose(1, 2), kc.transpose(1, 2), vc.transpose(1, 2)).transpose(1, 2)
    assert torch.equal(arena, before)                       # the backend must not write the cache it reads
    for o in (o_attn, o_op, o_sage):
        assert o.shape == g["attn_out"].shape and o.dtype == torch.bfloat16
        assert max_abs(o.cpu(), g["attn_out"]) <= 2e-2
    assert o_attn.is_contiguous() and torch.equal(o_attn, o_op) and torch.equal(o_attn, o_sage)
    assert torch.equal(o_attn, ops.attn_fwd(q, kc, vc))     # == the raw C-ABI call
    # dtype contract (attention.py:166-178): non-half inputs are computed in `dtype` and returned in the input dtype
    o32 = plug.attention(q.float(), kc.float(), vc.float())
    assert o32.dtype == torch.float32 and torch.equal(o32, o_attn.float())
    # softmax_scale / q_scale
    ref = _attn_ref(q * 0.5, kc, vc)
    assert max_abs(plug.attention(q, kc, vc, q_scale=0.5), ref) <= 2e-2
    assert max_abs(plug.attention(q, kc, vc, softmax_scale=0.5 / math.sqrt(128)), ref) <= 2e-2
    # block-causal recompute mask through the op
    S = min(q.shape[1], Lkv)
    lim = torch.clamp((torch.arange(S, device=DEV) // 128 + 1) * 128, max=S)
    o_bc = torch.ops.rtv.attn_fwd(q[:, :S], kc[:, :S], vc[:, :S], -1.0, 128, 0)
    assert max_abs(o_bc, _attn_ref(q[:, :S], kc[:, :S], vc[:, :S], lim)) <= 2e-2
    with pytest.raises(NotImplementedError):
        plug.attention(q, kc, vc, causal=True)


def test_attention_plugin_honours_key_lengths_or_refuses(ops):
    """`k_lens` of the plug-in contract (wan/modules/attention.py:91-99, :119-147: the FlashAttention branch drops the keys at
    positions >= k_lens[b]; the cross-attention of the non-causal model passes it, model.py:215): honoured exactly as a per-batch
    key prefix, full lengths are the plain call bit for bit, and what cannot be honoured raises - nothing is silently ignored."""
    from realtime_video_amd import attention as plug
    q, k, v = _randn(2, 300, 3, 128, seed=1), _randn(2, 512, 3, 128, seed=2), _randn(2, 512, 3, 128, seed=3)
    lens = torch.tensor([77, 512])
    out = plug.attention(q, k, v, k_lens=lens)
    for b, n in enumerate(lens.tolist()):
        assert max_abs(out[b:b + 1], _attn_ref(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n])) <= 2e-2
    assert rel_l2(out[0], plug.attention(q, k, v)[0]) > 1e-2                      # the mask matters for the short element
    full = plug.attention(q, k, v, q_lens=torch.tensor([300, 300]), k_lens=torch.tensor([512, 512]))
    assert torch.equal(full, plug.attention(q, k, v))
    with pytest.raises(NotImplementedError):
        plug.attention(q, k, v, q_lens=torch.tensor([300, 200]))
    with pytest.raises(ValueError):
        plug.attention(q, k, v, k_lens=torch.tensor([600, 512]))


def test_attention_custom_op_opcheck():
    """torch.library.opcheck on `rtv::attn_fwd` (schema, fake-tensor propagation, AOT dispatch) - the registration the
    reference does for sageattention (sage.py:12-19) so that traced graphs survive."""
    import realtime_video_amd.attention  # noqa: F401  (registers the op)
    q = _randn(1, 200, 2, 128, seed=1)
    cache = _randn(1, 333, 2, 2, 128, seed=2)
    k, v = cache[:, 10:310, 0], cache[:, 10:310, 1]
    torch.library.opcheck(torch.ops.rtv.attn_fwd.default, (q, k, v), {"softmax_scale": -1.0, "causal_block": 0, "q_offset": 0})
    torch.library.opcheck(torch.ops.rtv.attn_fwd.default, (q, k[:, :256], v[:, :256]),
                          {"softmax_scale": 0.05, "causal_block": 64, "q_offset": 56})
    fake = torch.library.opcheck   # noqa: F841
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fq = torch.empty(1, 200, 2, 128, dtype=torch.bfloat16, device=DEV)
        fk = torch.empty(1, 300, 2, 128, dtype=torch.bfloat16, device=DEV)
        out = torch.ops.rtv.attn_fwd(fq, fk, fk)
        assert out.shape == (1, 200, 2, 128) and out.dtype == torch.bfloat16


# ----------------------------------------------------------------------------------------- ring-indexed rolling cache (K8)
@pytest.mark.parametrize("seg0,seg1", [((1560, 3000), (7000, 2360)), ((0, 64), (100, 64)), ((5, 1), (900, 1)),
                                       ((4680, 4680), (0, 4680)), ((10, 100), (0, 0)), ((3, 77), (200, 1003))])
def test_attention_two_segment_window_equals_concatenated_keys(ops, seg0, seg1):
    """rtv_attn_fwd_win walks two row ranges of the cache in place; the result is bit-identical to the one-segment kernel
    on a contiguous copy of the same keys (same virtual tiling) and within tolerance of the fp32 definition."""
    (r0, n0), (r1, n1) = seg0, seg1
    H, Lq = 2, 300
    q = _randn(1, Lq, H, 128, seed=1)
    arena = _randn(1, 9400, 2, H, 128, seed=2)
    kc, vc = arena[:, :, 0], arena[:, :, 1]
    out = ops.attn_fwd_win(q, kc, vc, seg0, seg1)
    k = torch.cat([kc[:, r0:r0 + n0], kc[:, r1:r1 + n1]], 1).contiguous()
    v = torch.cat([vc[:, r0:r0 + n0], vc[:, r1:r1 + n1]], 1).contiguous()
    assert torch.equal(out, ops.attn_fwd(q, k, v))
    assert max_abs(out, _attn_ref(q, k, v)) <= 2e-2


@pytest.mark.parametrize("form", [0, 1])
def test_qk_norm_rope_cache_ring_write(ops, form):
    """rtv_qk_norm_rope_cache_ring stores logical cache row r >= ring_lo at ring_lo + (r - ring_lo + shift) % size: the rows it
    writes are the plain kernel's rows, permuted; everything else in the cache is untouched.  Both forms of the kernel."""
    from realtime_video_amd import _lib
    from realtime_video_amd.rope import rope_cos_sin_table
    _lib.load().rtv_rope_set_wave(form)
    try:
        _ring_write_case(ops)
    finally:
        _lib.load().rtv_rope_set_wave(-1)      # the switch is process-wide: never leave it forced for the tests that follow


def _ring_write_case(ops):
    from realtime_video_amd.rope import rope_cos_sin_table
    F_, gh, gw, H = 2, 6, 10, 2
    M, d = F_ * gh * gw, 256
    qkv = _randn(M, 3 * d, seed=1)
    wq, wk = _randn(d, seed=2), _randn(d, seed=3)
    cs = rope_cos_sin_table(128).to(DEV)
    rows = 400
    base = _randn(rows, 2, H, 128, seed=4)
    plain, ring = base.clone(), base.clone()
    row0, lo, size, shift = 150, 40, 300, 100        # rows [150, 270): 40 + ((110 .. 229) + 100) % 300 wraps after 90 rows
    q0 = ops.qk_norm_rope_cache(qkv, plain[:, 0], plain[:, 1], row0, H, wq, wk, cs, (F_, gh, gw), 5)
    q1 = ops.qk_norm_rope_cache(qkv, ring[:, 0], ring[:, 1], row0, H, wq, wk, cs, (F_, gh, gw), 5, ring=(lo, size, shift))
    assert torch.equal(q0, q1)
    r = torch.arange(row0, row0 + M)
    phys = lo + (r - lo + shift) % size
    assert phys.min() >= lo and phys.max() < lo + size and (phys[1:] < phys[:-1]).any()      # really wraps
    assert torch.equal(ring[phys.to(DEV)], plain[row0:row0 + M])
    mask = torch.ones(rows, dtype=torch.bool)
    mask[phys] = False
    assert torch.equal(ring[mask.to(DEV)], base[mask.to(DEV)])
    with pytest.raises(RuntimeError):
        ops.qk_norm_rope_cache(qkv, ring[:, 0], ring[:, 1], row0, H, wq, wk, cs, (F_, gh, gw), 5, ring=(lo, 100, 3))


# ----------------------------------------------------------------------------------------- scheduler step (one launch)
def _eager_x0(sch, flow, xt, t):
    """The reference's eager chain (utils/wan_wrapper.py:181-205) evaluated with torch ops."""
    fp, x, sig, ts = flow.double(), xt.double(), sch.sigmas.double(), sch.timesteps.double()
    idx = torch.argmin((ts.unsqueeze(0) - t.unsqueeze(1)).abs(), dim=1)
    return (x - sig[idx].reshape(-1, 1, 1, 1) * fp).to(flow.dtype)


def _eager_add_noise(sch, x0, noise, t):
    """utils/scheduler.py:159-176 with torch ops."""
    idx = torch.argmin((sch.timesteps.unsqueeze(0) - t.unsqueeze(1)).abs(), dim=1)
    sigma = sch.sigmas[idx].reshape(-1, 1, 1, 1)
    return ((1 - sigma) * x0 + sigma * noise).type_as(noise)


def test_scheduler_step_is_bit_exact_with_the_reference_golden(golden, ops):
    """x0 and add_noise minted from the reference (oracle/make_golden.py) - integer-exact comparison."""
    from realtime_video_amd.scheduler import FlowMatchScheduler
    from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
    g = golden("ops.pt")
    sch = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(1000, training=True)
    sch.to(DEV)
    a, b, t = g["an_x0"].to(DEV), g["an_noise"].to(DEV), g["an_t"].to(DEV)
    assert torch.equal(sch.add_noise(a, b, t).cpu(), g["an_out"])                 # kernel path (GPU bf16 4-D)
    assert torch.equal(sch.add_noise(a, b, t.long()).cpu(), sch.add_noise(a.cpu(), b.cpu(), t.long().cpu()))
    wr = WanDiffusionWrapper.__new__(WanDiffusionWrapper)
    wr.scheduler = sch
    assert torch.equal(wr._convert_flow_pred_to_x0(a, b, t).cpu(), g["x0_out"])
    x0, noisy = ops.scheduler_step(sch.timesteps, sch.sigmas, flow=a, xt=b, t=t, noise=a, t_next=t)
    assert torch.equal(x0.cpu(), g["x0_out"])
    assert torch.equal(noisy, _eager_add_noise(sch, x0, a, t))


@pytest.mark.parametrize("tdtype", [torch.float32, torch.int64, torch.float64])
def test_scheduler_step_matches_the_eager_chain_bitwise_at_full_size(ops, tdtype):
    """3 x 16 x 60 x 104 latents, the model's [C, F, h, w] output read through strides, per-frame timesteps that differ,
    ties of the nearest-timestep search included (t halfway between two table entries)."""
    from realtime_video_amd.scheduler import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=8.0, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(1000, training=True)
    sch.to(DEV)
    F, C, h, w = 3, 16, 60, 104
    out_cf = _randn(C, F, h, w, seed=3)                       # what the DiT returns
    flow = out_cf.permute(1, 0, 2, 3)                         # [F, C, h, w] view, channel stride F*h*w
    big = _randn(7, C, h, w, seed=4)
    xt = big[2:5]                                             # a slice of the session's noise buffer
    noise = _randn(F, C, h, w, seed=5)
    tab = sch.timesteps
    mid = ((tab[10].double() + tab[11].double()) / 2).item()
    for t_list, tn_list in [([1000.0, 750.0, 500.0], [750.0, 500.0, 250.0]), ([mid, 0.0, 999.0], [3.0, mid, 1000.0]),
                            ([tab[500].item()] * 3, [tab[999].item()] * 3)]:
        t = torch.tensor(t_list, dtype=torch.float64).to(tdtype).to(DEV)
        tn = torch.tensor(tn_list, dtype=torch.float64).to(tdtype).to(DEV)
        x0, noisy = ops.scheduler_step(sch.timesteps, sch.sigmas, flow=flow, xt=xt, t=t, noise=noise, t_next=tn)
        ref_x0 = _eager_x0(sch, flow, xt, t)
        assert torch.equal(x0, ref_x0)
        assert torch.equal(noisy, _eager_add_noise(sch, ref_x0, noise, tn))
        x0_only, none = ops.scheduler_step(sch.timesteps, sch.sigmas, flow=flow, xt=xt, t=t)
        assert none is None and torch.equal(x0_only, ref_x0)
        _, noisy_only = ops.scheduler_step(sch.timesteps, sch.sigmas, x0=ref_x0, noise=noise, t_next=tn)
        assert torch.equal(noisy_only, noisy)


def test_scheduler_step_refuses_what_it_does_not_cover(ops):
    from realtime_video_amd.scheduler import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=8.0, sigma_min=0.0, extra_one_step=True).to(DEV)
    a = _randn(3, 16, 8, 12)
    t = torch.full((3,), 500.0, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.scheduler_step(sch.timesteps, sch.sigmas, flow=a.float(), xt=a.float(), t=t)
    with pytest.raises(ValueError):
        ops.scheduler_step(sch.timesteps, sch.sigmas, flow=a, xt=a, t=t[:2])
    with pytest.raises(RuntimeError):
        ops.scheduler_step(sch.timesteps.cpu(), sch.sigmas.cpu(), flow=a.cpu(), xt=a.cpu(), t=t.cpu())
    # float32 latents keep the eager chain (still on the GPU)
    out = sch.add_noise(a.float(), a.float(), t)
    assert out.dtype == torch.float32


# ----------------------------------------------------------------------------------------- attention: four-phase kernel
W4 = 840 + 600     # rtv_attn_set_waves: the one-wave-per-SIMD kernel (attn_w4.hip), product variant


def _both_schedules(ops, fn):
    """lockstep, four-phase, and - folded into the second result after an equality check - the one-wave-per-SIMD kernel (r05: where it
    does not apply - f16, two-range windows - the launcher falls back to the four-phase kernel, which makes the check trivial)."""
    outs = []
    try:
        for w in (81, 82, W4):
            ops.attn_set_waves(w)
            outs.append(fn())
    finally:
        ops.attn_set_waves(0)
    assert torch.equal(outs[1], outs[2]), "one-wave-per-SIMD kernel != four-phase kernel"
    return outs[:2]


@pytest.mark.parametrize("B,Lq,Lkv,H,cb,dt", [
    (1, 600, 1024, 2, 0, torch.bfloat16), (1, 333, 1000, 3, 96, torch.bfloat16), (2, 300, 333, 2, 0, torch.float16),
    (1, 256, 64, 1, 0, torch.bfloat16), (1, 100, 70, 2, 0, torch.bfloat16), (1, 257, 129, 2, 0, torch.bfloat16),
    (1, 1040, 1040, 2, 520, torch.bfloat16), (1, 512, 191, 8, 0, torch.bfloat16), (1, 1560, 3000, 8, 0, torch.bfloat16),
    (1, 4680, 4680, 8, 4680, torch.bfloat16), (2, 700, 2100, 3, 0, torch.bfloat16), (1, 64, 4100, 1, 0, torch.bfloat16)])
def test_attention_four_phase_kernel_equals_lockstep_and_reference(ops, B, Lq, Lkv, H, cb, dt):
    """The four-phase kernel (LDS-DMA staging, fragments read a phase ahead) and the one-wave-per-SIMD kernel (r05: 4 waves x 64
    rows, softmax pipelined across the matrix phases, asm-owned accumulation registers) accumulate in the same order as the lockstep
    one: outputs are bit-identical, on ragged windows, one-tile windows, the block-causal prefix and fp16 alike; both are
    within the stated tolerance of the fp32 reference.  Keys grow along the sequence so that rescales fire late."""
    q = _randn(B, Lq, H, 128, seed=1, dtype=dt)
    k = (_randn(B, Lkv, H, 128, seed=2, dtype=torch.float32) * torch.linspace(0.3, 3.0, Lkv, device=DEV).view(1, Lkv, 1, 1)).to(dt)
    v = _randn(B, Lkv, H, 128, seed=3, dtype=dt)
    q_off = Lkv - Lq if cb and Lkv > Lq else 0
    a, b = _both_schedules(ops, lambda: ops.attn_fwd(q, k, v, causal_block=cb, q_offset=q_off))
    assert torch.equal(a, b)
    lim = None
    if cb:
        lim = torch.clamp(((torch.arange(Lq, device=DEV) + q_off) // cb + 1) * cb, max=Lkv)
    assert max_abs(b, _attn_ref(q, k, v, lim)) <= (4e-3 if dt == torch.float16 else 3e-2)


@pytest.mark.parametrize("seg0,seg1", [((2000, 700), (100, 333)), ((100, 333), (2000, 700)), ((64, 64), (0, 64)),
                                       ((1000, 1), (10, 130)), ((500, 1000), (0, 0)), ((2900, 100), (0, 1500))])
def test_attention_four_phase_kernel_two_range_windows(ops, seg0, seg1):
    """Ring windows: the second range below the first one (a wrapped ring - the DMA base moves to the lowest row), above it,
    tile-straddling boundaries; equal to the lockstep kernel and to attention over the concatenated keys."""
    kc, vc = _randn(1, 3000, 4, 128, seed=5), _randn(1, 3000, 4, 128, seed=6)
    q = _randn(1, 520, 4, 128, seed=7)
    a, b = _both_schedules(ops, lambda: ops.attn_fwd_win(q, kc, vc, seg0, seg1))
    kk = torch.cat([kc[:, seg0[0]:seg0[0] + seg0[1]], kc[:, seg1[0]:seg1[0] + seg1[1]]], 1).contiguous()
    vv = torch.cat([vc[:, seg0[0]:seg0[0] + seg0[1]], vc[:, seg1[0]:seg1[0] + seg1[1]]], 1).contiguous()
    ref, ref_pp = _both_schedules(ops, lambda: ops.attn_fwd(q, kk, vv))
    assert torch.equal(a, b) and torch.equal(b, ref) and torch.equal(ref, ref_pp)


def test_attention_four_phase_kernel_strided_cache_views_full_size(ops):
    """14B layer geometry: 4680 query rows, 40 heads, keys in place in a [rows, H, 128] cache whose row stride is the whole
    model width, window of 9360 rows starting mid-cache; default dispatch (four-phase) == lockstep, bit for bit."""
    H = 40
    kc = _randn(1, 9360 + 700, H, 128, seed=2)
    vc = _randn(1, 9360 + 700, H, 128, seed=3)
    q = _randn(1, 4680, H, 128, seed=1)
    k, v = kc[:, 333:333 + 9360], vc[:, 333:333 + 9360]
    a, b = _both_schedules(ops, lambda: ops.attn_fwd(q, k, v))
    assert torch.equal(a, b) and torch.equal(ops.attn_fwd(q, k, v), b)


# ----------------------------------------------------------------------------------------- r06: the whole 32760-row cache at 40 heads
def test_attention_full_cache_window_32760_rows_at_14b_width(ops):
    """north_star's "~25 GB KV cache" operating point at the kernel: the largest window the reference ever attends -
    `max_attention_size` = 32760 rows (wan/modules/causal_model.py:192, :388-389), the size pipeline/causal_inference.py:284-289
    allocates - at the 14B's 40 heads, 4680 query rows, K and V read IN PLACE from one layer's slice of the cache arena
    ([rows, 2, H, 128]: K and V of a row side by side, row stride 2 x the model width, pipeline._initialize_kv_cache).
    (1) against the fp32 definition on sampled heads, stated tolerance 2e-2 max-abs / 1e-2 rel-L2 on unit-variance data;
    (2) the one-wave-per-SIMD kernel (the default for this shape) == the four-phase kernel == the lockstep kernel, bit for bit;
    (3) the window as two physical ranges of the same rows (a ring that wrapped at row 20000) == the single range."""
    H, Lq, Lkv = 40, 4680, 32760
    arena = _randn(1, Lkv, 2, H, 128, seed=2)
    k, v = arena[:, :, 0], arena[:, :, 1]
    assert k.stride(1) == 2 * H * 128 and not k.is_contiguous()
    q = _randn(1, Lq, H, 128, seed=1)
    a, b = _both_schedules(ops, lambda: ops.attn_fwd(q, k, v))
    out = ops.attn_fwd(q, k, v)
    assert torch.equal(a, b) and torch.equal(out, b)
    for h in (0, 23, 39):
        ref = _attn_ref(q[:, :, h:h + 1], k[:, :, h:h + 1], v[:, :, h:h + 1])
        assert max_abs(out[:, :, h:h + 1], ref) <= 2e-2
        assert rel_l2(out[:, :, h:h + 1], ref) <= 1e-2
    two = ops.attn_fwd_win(q, k, v, (0, 20000), (20000, Lkv - 20000))
    assert torch.equal(two, out)
