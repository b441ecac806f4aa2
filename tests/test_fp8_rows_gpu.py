"""The fp8 mode with per-row scales on the GPU (enable_fp8("row"); include/rtv_hip_fp8_rows.h): the row quantiser, the
LayerNorm-fused quantiser and the row-scale GEMM against the restatement in tests/fp8_rows_oracle.py, then the model, its
context-parallel sharding and the LoRA re-quantisation.  Parity with torchao itself is unpinned (see the oracle file)."""
import pytest
import torch

from conftest import max_abs, rel_l2
from fp8_rows_oracle import fp8_rows_linear, fp8_rows_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def _codes(t):
    return t.view(torch.uint8)


# ----------------------------------------------------------------------------------------- row quantiser
@pytest.mark.parametrize("M,d,ld", [(5, 128, 128),        # a wave per row, a workgroup of 4 rows with one row to spare
                                    (300, 1536, 1536),    # wave form, 3 of a lane's 4 chunks
                                    (37, 13824, 13824),   # the widest row: 7 chunks per thread, the last one partial (1728 = 6.75 x 256)
                                    (64, 5120, 5120 + 64)])   # workgroup form (3 chunks, the last partial), strided input
def test_row_quantiser_matches_restatement_bit_for_bit(ops, M, d, ld):
    g = torch.Generator().manual_seed(M + d)
    mag = 2.0 ** torch.linspace(-20, 20, M).reshape(M, 1)              # row magnitudes from 2^-20 to 2^20
    xf = torch.randn(M, ld, generator=g) * mag
    xf[1] = 0                                                          # a zero row
    big = xf.to(BF).to(DEV)
    x = big[:, :d]
    assert x.stride(0) == ld
    q, s = ops.quantize_fp8_rows(x)
    torch.cuda.synchronize()
    rq, rs = fp8_rows_quantize(x.cpu())                                # the restatement, evaluated on the host
    assert s.dtype == torch.float32 and s.shape == (M,)
    assert torch.equal(s.cpu().view(torch.int32), rs.reshape(M).view(torch.int32))
    assert torch.equal(_codes(q).cpu(), _codes(rq))
    inv448 = torch.tensor(1.0) / torch.tensor(448.0)
    assert float(s[1]) == float(torch.tensor(1e-12) * inv448) and int(_codes(q)[1].max()) == 0
    # into a strided output: the bytes between the rows are not written
    wide = torch.full((M, d + 64), 0x55, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    q2, _ = ops.quantize_fp8_rows(x, out=wide[:, :d])
    assert torch.equal(_codes(q2), _codes(q)) and bool((_codes(wide)[:, d:] == 0x55).all())


# ----------------------------------------------------------------------------------------- LayerNorm + modulate + quantise
@pytest.mark.parametrize("d", [1536, 5120])
@pytest.mark.parametrize("form", ["modulated", "affine"])
def test_fused_layernorm_quantiser_equals_the_two_kernels_bit_for_bit(ops, d, form):
    F_, fs = 3, 96
    x = _randn(F_ * fs, d, seed=1, scale=2.0)
    if form == "modulated":
        emod = _randn(F_, 6, d, seed=2, scale=0.5)
        kw = dict(shift=emod[0, 0], scale=emod[0, 1], frame_stride=6 * d, rows_per_frame=fs)
    else:
        kw = dict(weight=_randn(d, seed=3) * 0.1 + 1, bias=_randn(d, seed=4) * 0.1)
    q_ref, s_ref = ops.quantize_fp8_rows(ops.layernorm_modulate(x, 1e-6, **kw))
    q, s = ops.layernorm_modulate_fp8_rows(x, 1e-6, **kw)
    assert torch.equal(s.view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(_codes(q), _codes(q_ref))
    assert int((_codes(q) & 0x7F).max()) == 0x7E                       # every row reaches +-448: the scales are live
    if form == "modulated":                                           # a row offset into the frames, as a token shard passes it
        q_ref2, s_ref2 = ops.quantize_fp8_rows(ops.layernorm_modulate(x[:fs], 1e-6, row_offset=2 * fs, **kw))
        q2, s2 = ops.layernorm_modulate_fp8_rows(x[:fs], 1e-6, row_offset=2 * fs, **kw)
        assert torch.equal(_codes(q2), _codes(q_ref2)) and torch.equal(s2, s_ref2) and not torch.equal(_codes(q2), _codes(q[:fs]))


# ----------------------------------------------------------------------------------------- GEMM
def test_gemm_rows_exact_case(ops):
    """Small integer operands (exact in e4m3), power-of-two scales that change with every row and every column - with different
    periods, so a row / column swap or a scale index shifted by one shows - K = 128: every partial sum is an integer below 2^24
    and the scaled result is exact in fp32, so the output must be bf16(RNE(exact)) bit for bit.  (M, N) = (257, 264): an M tail of
    one row, an N tail that is a multiple of 8 only."""
    M, N, K = 257, 264, 128
    g = torch.Generator().manual_seed(7)
    a = torch.randint(-8, 9, (M, K), generator=g).float()
    w = torch.randint(-8, 9, (N, K), generator=g).float()
    sa = 2.0 ** ((torch.arange(M) % 31) - 15).float()
    sw = 2.0 ** (-(torch.arange(N) % 23)).float()
    aq, wq = a.to(torch.float8_e4m3fn).to(DEV), w.to(torch.float8_e4m3fn).to(DEV)
    assert torch.equal(aq.float().cpu(), a) and torch.equal(wq.float().cpu(), w)
    exact = (a.double() @ w.double().t()) * sa.double().reshape(M, 1) * sw.double().reshape(1, N)
    assert float((a.double().abs() @ w.double().abs().t()).max()) < 2 ** 24
    assert torch.equal(exact.float().double(), exact)                 # representable in fp32: one rounding, fp32 -> bf16
    ref = exact.float().to(BF)
    out = ops.gemm_fp8_rows(aq, sa.to(DEV), wq, sw.to(DEV))
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))
    bias = _randn(N, seed=8)                                          # through the narrow store path too (ldc no multiple of 8)
    pad = torch.zeros(M, N + 4, dtype=BF, device=DEV)
    ops.gemm_fp8_rows(aq, sa.to(DEV), wq, sw.to(DEV), bias=bias, out=pad[:, :N])
    ref_b = (exact.float() + bias.float().cpu()).to(BF)
    assert torch.equal(pad[:, :N].cpu().view(torch.int16), ref_b.view(torch.int16)) and float(pad[:, N:].abs().max()) == 0


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N,K", [(257, 264, 128), (4680, 5120, 1024)])
def test_gemm_rows_equals_the_per_tensor_gemm_under_constant_power_of_two_scales(ops, M, N, K, with_bias):
    """The two fp8 GEMM kernels are one body (csrc/gemm_fp8_body.h) around two de-quantise steps.  With power-of-two scales that
    are constant over rows and columns both steps are exact - sum * 2^-8 against sum * 2^-3 * 2^-5 - so on any e4m3 codes the
    kernels must agree bit for bit.  (257, 264, 128): M and N tails; (4680, 5120, 1024): the last round split along K, whose
    partial sums are added in index order, so the arrival order cannot show."""
    g = torch.Generator().manual_seed(M + K)

    def codes(rows):                                                  # every e4m3 code but the two NaNs
        c = torch.randint(0, 256, (rows, K), generator=g, dtype=torch.uint8)
        return c.masked_fill((c & 0x7F) == 0x7F, 0).to(DEV).view(torch.float8_e4m3fn)

    aq, wq = codes(M), codes(N)
    s_x, s_w = 2.0 ** -3, 2.0 ** -5
    bias = _randn(N, seed=5) if with_bias else None
    rows = ops.gemm_fp8_rows(aq, torch.full((M,), s_x, device=DEV), wq, torch.full((N,), s_w, device=DEV), bias=bias)
    tensor = ops.gemm_fp8(aq, torch.full((1,), s_x, device=DEV), wq, s_w, bias=bias)
    assert bool(torch.isfinite(tensor).all()) and float(tensor.float().abs().max()) > 0
    assert torch.equal(rows.view(torch.int16), tensor.view(torch.int16))


def _quantised_pair(ops, M, N, K):
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    aq, sa = ops.quantize_fp8_rows(a)
    wq, sw = fp8_rows_quantize(w)
    return a, w, b, aq, sa, wq, sw.reshape(N).contiguous()


@pytest.mark.parametrize("M,N,K", [(300, 1536, 256), (585, 2560, 5120), (4680, 5120, 1024)])
def test_gemm_rows_matches_fp64_on_the_dequantised_operands(ops, M, N, K):
    """(4680, 5120, 1024): 380 tiles, the last round split along K (the workspace is attached by ops.gemm_fp8_rows)."""
    _, _, b, aq, sa, wq, sw = _quantised_pair(ops, M, N, K)
    ref = (aq.float().double() * sa.double().reshape(M, 1)) @ (wq.float().double() * sw.double().reshape(N, 1)).t() + b.double()
    for _ in range(2):                                                # (the split-K arrival counters must come back to zero)
        out = ops.gemm_fp8_rows(aq, sa, wq, sw, bias=b)
        assert rel_l2(out, ref) <= 4e-3


@pytest.mark.parametrize("M,N,K", [(300, 1536, 256), (585, 2560, 5120)])
def test_gemm_rows_matches_torch_scaled_mm_rowwise(ops, M, N, K):
    """The same e4m3 bytes and scales through `torch._scaled_mm` with scale_a [M, 1] and scale_b [1, N] - what torchao's PerRow
    linear calls at the bottom - and through rtv_gemm_fp8_rows: they differ by the fp32 accumulation order, the order of the two
    scale multiplications and the final bf16 rounding.  Bounds of the per-tensor pin."""
    if not hasattr(torch, "_scaled_mm"):
        pytest.skip("torch._scaled_mm not available")
    _, _, b, aq, sa, wq, sw = _quantised_pair(ops, M, N, K)
    def scaled_mm(bias):
        y = torch._scaled_mm(aq, wq.t(), scale_a=sa.reshape(M, 1), scale_b=sw.reshape(1, N), bias=bias, out_dtype=BF)
        torch.cuda.synchronize()
        return y

    try:
        try:
            ref = scaled_mm(b)
        except (RuntimeError, TypeError, ValueError, NotImplementedError):      # row-wise scales without the fused bias, then
            ref, b = scaled_mm(None), None
    except (RuntimeError, TypeError, ValueError, NotImplementedError) as e:      # a build that refuses row-wise scales here
        pytest.skip(f"torch._scaled_mm refuses row-wise scales in this build: {str(e)[:160]}")
    out = ops.gemm_fp8_rows(aq, sa, wq, sw, bias=b)
    print(f"rows vs _scaled_mm ({M}, {N}, {K}): rel-L2 {rel_l2(out, ref):.3e} max-abs {max_abs(out, ref):.3e}")
    assert rel_l2(out, ref) <= 2e-3
    assert max_abs(out, ref) <= 2 ** -7 * float(ref.float().abs().max())


def test_gemm_rows_fused_epilogue(ops):
    M, N, K, F = 4680, 1536, 1536, 3
    a, w, b, aq, sa, wq, sw = _quantised_pair(ops, M, N, K)
    gate, res = _randn(F, N, seed=4), _randn(M, N, seed=5)
    xq, sx = fp8_rows_quantize(a)
    assert torch.equal(_codes(xq), _codes(aq))
    y = (xq.float() @ wq.float().t()) * sx * sw + b.float()
    yb = y.to(BF)
    g = gate.repeat_interleave(M // F, dim=0)
    ref = res + (yb * g)                                               # bf16(acc+bias) -> * gate -> + residual, as rtv_gemm
    out = ops.gemm_fp8_rows(aq, sa, wq, sw, bias=b, gate=gate, gate_stride=N, rows_per_frame=M // F, residual=res)
    assert rel_l2(out, ref) <= 4e-3
    out = ops.gemm_fp8_rows(aq, sa, wq, sw, bias=b, act=1)
    assert rel_l2(out, torch.nn.functional.gelu(yb, approximate="tanh")) <= 4e-3


def test_rows_far_below_the_tensor_maximum_keep_their_precision(ops):
    """The case the mode exists for: activation rows whose magnitudes run from 2^0 down to 2^-16.  Per row, the relative error
    against fp64 on the UNQUANTISED operands; the worst row of the native result may exceed the worst row of the restatement on
    the same data by 4e-3 (the bound of the GEMM tests above) and no more.  The per-tensor path's worst row is printed beside it:
    its small rows sit in e4m3's subnormals or flush to zero."""
    M, N, K = 512, 384, 1024
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(M, K, generator=g) * 2.0 ** torch.linspace(0, -16, M).reshape(M, 1)).to(BF).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF).to(DEV)
    exact = x.double() @ w.double().t()

    def worst_row(y):
        return float(((y.double() - exact).norm(dim=1) / exact.norm(dim=1)).max())

    xq, sx = ops.quantize_fp8_rows(x)
    wq, sw = fp8_rows_quantize(w)
    native = worst_row(ops.gemm_fp8_rows(xq, sx, wq, sw.reshape(N).contiguous()))
    restated = worst_row(fp8_rows_linear(x, w, None))
    tq, ts = ops.quantize_fp8(x)
    s_w = w.float().abs().max().clamp(min=1e-12) / 448.0
    tensor = worst_row(ops.gemm_fp8(tq, ts, (w.float() / s_w).clamp(-448, 448).to(torch.float8_e4m3fn), float(s_w)))
    print(f"worst row, rel. error vs fp64: per-row native {native:.4f}, restatement {restated:.4f}; per-tensor native {tensor:.4f}")
    assert native <= restated + 4e-3


# ----------------------------------------------------------------------------------------- model
def _on_dev(w):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in w.items()}


def _tiny():
    from oracle.make_golden import TEXT_DIM, TINY, tiny_inputs
    return dict(TINY), TEXT_DIM, tiny_inputs


def _build(cfg, text_dim, weights):
    from realtime_video_amd.causal_model import CausalWanModel
    from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
    m = CausalWanModel(dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"],
                       text_dim=text_dim, freq_dim=cfg.get("freq_dim", 256), local_attn_size=cfg.get("local_attn_size", -1),
                       sink_size=cfg.get("sink_size", 0))
    m.load_state_dict(weights)
    return m, WanDiffusionWrapper(m, timestep_shift=5.0)


def _caches(cfg, kv_size):
    hd, L, H = cfg["dim"] // cfg["num_heads"], cfg["num_layers"], cfg["num_heads"]
    kv = [{"k": torch.zeros(1, kv_size, H, hd, dtype=BF, device=DEV), "v": torch.zeros(1, kv_size, H, hd, dtype=BF, device=DEV),
           "global_end_index": 0, "local_end_index": 0} for _ in range(L)]
    ca = [{"k": torch.zeros(1, 512, H, hd, dtype=BF, device=DEV), "v": torch.zeros(1, 512, H, hd, dtype=BF, device=DEV),
           "is_init": False} for _ in range(L)]
    return kv, ca


def _three_forwards(model, wr, lat, ctx, t, t0):
    """Denoise at cache offset 0, block-causal recompute, second-block denoise (tests/test_dit_gpu.py's fp8 sequence)."""
    kv, ca = _caches(dict(num_layers=model.num_layers, num_heads=model.num_heads, dim=model.dim), 9360)
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    a, _ = wr(lat[0].to(DEV), cond, t.to(DEV), kv, ca, current_start=0)
    for c in kv:
        c["global_end_index"] = 0
        c["local_end_index"] = 0
    model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3)
    rc, _ = wr(lat[2].to(DEV), cond, t0.to(DEV), kv, ca, current_start=4680)
    model.block_mask = None
    b, _ = wr(lat[3].to(DEV), cond, t.to(DEV), kv, ca, current_start=4680)
    return [x.cpu() for x in (a, rc, b)]


def test_row_mode_forward_matches_the_row_oracle(monkeypatch):
    """enable_fp8("row") against the oracle graph with its fp8 Linear replaced by the per-row restatement, on the three forwards of
    the per-tensor test and with its bounds: rel-L2 <= 3e-2 against the oracle, 0 < rel-L2 <= 0.1 against the bf16 model."""
    from oracle import wan_oracle as wo
    monkeypatch.setattr(wo, "fp8_linear", fp8_rows_linear)
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    w8 = dict(w)
    w8[wo.FP8_FLAG] = True
    lat, ctx = tiny_inputs()
    sched = wo.FlowMatchScheduler()
    kvc = wo.initialize_kv_cache(cfg["num_layers"], 1, 9360, cfg["num_heads"], 128, BF, DEV)
    cac = wo.initialize_crossattn_cache(cfg["num_layers"], 1, cfg["num_heads"], 128, BF, device=DEV)
    w8, ctx_d, lat_d = _on_dev(w8), ctx.to(DEV), [x.to(DEV) for x in lat]
    t = torch.ones([1, 3], dtype=torch.int64) * 700
    t0 = torch.zeros([1, 3], dtype=torch.int64)
    ref_a, _ = wo.wrapper_forward(w8, cfg, sched, lat_d[0], [ctx_d], t.to(DEV), kvc, cac, 0)
    wo.reset_kv_cache(kvc)
    ref_rc, _ = wo.wrapper_forward(w8, cfg, sched, lat_d[2], [ctx_d], t0.to(DEV), kvc, cac, 4680, recompute=True)
    ref_b, _ = wo.wrapper_forward(w8, cfg, sched, lat_d[3], [ctx_d], t.to(DEV), kvc, cac, 4680)
    outs = {}
    for mode in ("bf16", "row"):
        model, wr = _build(cfg, text_dim, w)
        if mode == "row":
            assert model.enable_fp8("row") is model and model._cfg.use_fp8 == 2
            with pytest.raises(RuntimeError, match="other granularity"):
                model.enable_fp8()
        outs[mode] = _three_forwards(model, wr, lat, ctx, t, t0)
    vs_oracle = [rel_l2(ours, ref) for ours, ref in zip(outs["row"], (ref_a, ref_rc, ref_b))]
    vs_bf16 = [rel_l2(f8, bf) for f8, bf in zip(outs["row"], outs["bf16"])]
    print("row mode vs row oracle:", " ".join(f"{v:.3e}" for v in vs_oracle), "| vs bf16:", " ".join(f"{v:.3e}" for v in vs_bf16))
    assert all(v <= 3e-2 for v in vs_oracle)
    assert all(0 < v <= 0.1 for v in vs_bf16)


@pytest.mark.parametrize("exchange", ["heads", "rows"])
def test_row_mode_context_parallel_matches_the_unsharded_row_mode(exchange):
    """Two shards in lockstep on this GPU (the rig of the per-tensor context-parallel test) against the unsharded forward, both in
    row mode: every row is quantised alone, so the shards take the unsharded forward's quantisation decisions and what remains is
    the accumulation order of GEMMs and attention over other tile grids.  <= 3e-2; the per-tensor mode measures 2.5e-2 / 3.2e-2.
    Measured here: 0 for both exchanges - e4m3 products are exact and an output element is accumulated over K in the same order
    whatever the tile grid, so the sharded forward is bit-identical; the bound stays, split-K plans may differ with other shapes."""
    from oracle import wan_oracle as wo
    from realtime_video_amd.parallel import SimulatedContextParallel
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    t = torch.ones([1, 3], dtype=torch.int64) * 700
    t0 = torch.zeros([1, 3], dtype=torch.int64)
    outs = []
    for cp in (SimulatedContextParallel(2, exchange), None):
        model, wr = _build(cfg, text_dim, w)
        model.context_parallel = cp
        model.enable_fp8("row")
        kv, ca = _caches(cfg, 9360)
        cond = {"prompt_embeds": [ctx.to(DEV)]}
        model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3)
        rc, _ = wr(lat[2].to(DEV), cond, t0.to(DEV), kv, ca, current_start=4680)
        model.block_mask = None
        b, _ = wr(lat[3].to(DEV), cond, t.to(DEV), kv, ca, current_start=4680)
        outs.append((rc.cpu(), b.cpu()))
    errs = [rel_l2(sharded, whole) for sharded, whole in zip(*outs)]
    print(f"row mode, 2 shards ({exchange}) vs unsharded:", " ".join(f"{v:.3e}" for v in errs))
    assert all(v <= 3e-2 for v in errs)


# ----------------------------------------------------------------------------------------- LoRA
def test_lora_requantises_rows_in_place():
    """Adapter loaded, enable_fp8("row"), set_lora_scale, unload: the merged matrices are re-quantised into the existing e4m3
    buffers and row-scale tensors (same addresses, graphs dropped), and after the unload codes and row scales are those of a
    fresh enable_fp8("row")."""
    from oracle import wan_oracle as wo
    from realtime_video_amd.causal_model import CausalWanModel
    cfg = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=2, freq_dim=256, text_len=512, eps=1e-6)
    sd = wo.make_weights(cfg, seed=5, text_dim=128)
    g = torch.Generator().manual_seed(9)
    lsd = {}
    for name, (o, k) in {"self_attn.q": (256, 256), "self_attn.v": (256, 256), "cross_attn.k": (256, 256), "ffn.0": (512, 256),
                         "ffn.2": (256, 512)}.items():
        lsd[f"blocks.1.{name}.lora_A.weight"] = (0.05 * torch.randn(8, k, generator=g)).to(BF)
        lsd[f"blocks.1.{name}.lora_B.weight"] = (0.05 * torch.randn(o, 8, generator=g)).to(BF)

    def model():
        m = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=128, device=DEV)
        m.load_state_dict(sd)
        return m

    def state(m):
        return ({k: _codes(v).clone() for k, v in m._tensors.items() if v.dtype == torch.float8_e4m3fn},
                {k: v.clone() for k, v in m._fp8_row_scales.items()})

    def same(a, b):
        return all(x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))

    fresh = model().enable_fp8("row")
    assert len(fresh._fp8_row_scales) == 6 + 8 * 2 and fresh._fp8_row_scales["L0.qkv_w"].shape == (768,)
    m = model()
    m.load_lora(lsd, scale=0.0, name="style")
    m.enable_fp8("row")
    assert same(state(m), state(fresh))                                 # strength 0: the bases
    ptrs = {k: v.data_ptr() for k, v in list(m._tensors.items()) + [("s." + k, v) for k, v in m._fp8_row_scales.items()]}
    table, version = list(m._fp8_row_table), m._weights_version
    m.set_lora_scale("style", 1.0)
    merged = model()
    merged.load_lora(lsd, scale=1.0, name="style")
    merged.enable_fp8("row")
    assert same(state(m), state(merged)) and not same(state(m), state(fresh))
    assert not torch.equal(m._fp8_row_scales["L1.qkv_w"][:256], fresh._fp8_row_scales["L1.qkv_w"][:256])      # q rows moved,
    assert torch.equal(m._fp8_row_scales["L1.qkv_w"][256:512], fresh._fp8_row_scales["L1.qkv_w"][256:512])    # k rows did not
    assert {k: v.data_ptr() for k, v in list(m._tensors.items()) + [("s." + k, v) for k, v in m._fp8_row_scales.items()]} == ptrs
    assert list(m._fp8_row_table) == table and m._weights_version != version and not m._graphs
    m.unload_lora()
    assert same(state(m), state(fresh)) and m._lora_base == {}
