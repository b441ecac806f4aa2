"""The MXFP6 mode on the GPU (enable_mxfp6(); include/rtv_hip_mxfp6.h): the quantiser, the LayerNorm-fused quantiser and the
block-scaled GEMM against the restatement of the OCP Microscaling conversion in tests/mxfp6_oracle.py, then the model.  The mode is
no reference mode (the reference has no FP6 path); tests/test_mxfp6_cpu.py vets the inputs used here."""
import pytest
import torch

import mxfp6_oracle as mx
from conftest import rel_l2
from mx_cases import BF, CFG, DEV, TEXT_DIM, dev_operands
from mx_cases import build as _build, caches as _caches, inputs as _inputs, oracle_forwards as _oracle_forwards, three_forwards as _three_forwards

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------------------- quantiser
# the wave path, its edge (2048), the workgroup path (2080: a short last K-tile of scales), and the most chunks per thread
@pytest.mark.parametrize("M,d", [(5, 256), (5, 2048), (3, 2080), (5, 5120), (2, 13824)])
def test_quantiser_matches_the_restatement_bit_for_bit(ops, M, d):
    x = mx.structured_rows(M, d)
    v, e = mx.mx_quantize(x)                                           # the restatement, evaluated on the host
    codes, scales = ops.quantize_mxfp6(x.to(DEV))
    torch.cuda.synchronize()
    assert codes.shape == (M, mx.code_bytes(d)) and scales.shape == (M, mx.scale_bytes(d))
    assert torch.equal(scales.cpu(), mx.pack_scales(e))                # scale bytes exactly (bytes no block owns stay 0)
    assert torch.equal(mx.unpack_codes(codes.cpu()), mx.sextets(v))    # codes modulo the sign of zero
    assert int(scales.max()) < 255


def test_quantiser_clamps_subnormal_and_smallest_normal_block_maxima(ops):
    """Blocks whose maximum has an fp32 exponent field of 0 (bf16 subnormals), 1 or 2 clamp to the scale byte 0 (e = -127); field 3
    is the first that does not.  The values are multiples of 2^-133 given by their bf16 bit patterns, of both signs: in units of
    2^-127 multiples of 1/64, so the ties of e2m3 (odd multiples of 1/16, ...) are among them, several named."""
    g = torch.Generator().manual_seed(17)
    M, d = 4, 256
    bits = torch.randint(0, 0x80, (M, d), generator=g)                 # subnormals: k x 2^-133, k < 128
    bits[1] = torch.randint(0, 0x100, (d,), generator=g)               # up to exponent field 1
    bits[2] = torch.randint(0, 0x180, (d,), generator=g)               # up to field 2
    bits[3] = torch.randint(0, 0x200, (d,), generator=g)               # up to field 3: E = 1 where a block reaches it
    bits[0, :8] = torch.tensor([0x40, 0x60, 0x04, 0x0C, 0x3C, 0x7C, 0x01, 0x7F])   # 1, 1.5, 1/16, 3/16, 15/16, 31/16 x 2^-127, ...
    bits[0, 32:64] = 0x01                                              # a block whose maximum is the smallest subnormal
    bits[3, 5] = 0x1C0                                                 # 1.5 x 2^-124
    bits = bits | (torch.randint(0, 2, (M, d), generator=g) << 15)
    x = bits.to(torch.int16).view(BF)
    assert 0 < float(x[0].double().abs().max()) < 2.0 ** -126
    v, e = mx.mx_quantize(x)
    assert bool((e[:3] == -127).all()) and int(e[3].max()) == -126 and int((mx.sextets(v)[0] & 31).max()) >= 15
    codes, scales = ops.quantize_mxfp6(x.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(scales.cpu(), mx.pack_scales(e))
    assert torch.equal(mx.unpack_codes(codes.cpu()), mx.sextets(v))


def test_quantiser_with_padded_row_strides(ops):
    M, d = 5, 2080
    x = mx.structured_rows(M, d)
    v, e = mx.mx_quantize(x)
    xw = torch.zeros(M, d + 64, dtype=BF, device=DEV)
    xw[:, :d] = x.to(DEV)
    nc = mx.code_bytes(d)
    cw = torch.full((M, nc + 12), 0x55, dtype=torch.uint8, device=DEV)
    sw = torch.full((M, mx.scale_bytes(d) + 5), 0x55, dtype=torch.uint8, device=DEV)
    codes, scales = ops.quantize_mxfp6(xw[:, :d], codes=cw[:, :nc], scales=sw[:, :mx.scale_bytes(d)])
    torch.cuda.synchronize()
    assert torch.equal(mx.unpack_codes(codes.cpu()), mx.sextets(v))
    want = mx.pack_scales(e)
    owned = torch.zeros(mx.scale_bytes(d), dtype=torch.bool)
    owned[[mx.scale_pos(b) for b in range(d // 32)]] = True
    assert torch.equal(scales.cpu()[:, owned], want[:, owned])
    assert bool((scales.cpu()[:, ~owned] == 0x55).all())               # bytes of blocks the short last K-tile lacks: not written
    assert bool((cw[:, nc:] == 0x55).all()) and bool((sw[:, mx.scale_bytes(d):] == 0x55).all())


# ----------------------------------------------------------------------------------------- LayerNorm + modulate + quantise
@pytest.mark.parametrize("d", [256, 5120, 8192])                       # 8192: the widest row, all four chunks of every thread
@pytest.mark.parametrize("form", ["modulated", "affine"])
def test_fused_layernorm_quantiser_equals_the_two_kernels_bit_for_bit(ops, d, form):
    F_, fs = 2, 7
    x = _randn(F_ * fs, d, seed=1, scale=2.0)
    if form == "modulated":
        emod = _randn(4, 6, d, seed=2, scale=0.5)
        kw = dict(shift=emod[0, 0], scale=emod[0, 1], frame_stride=6 * d, rows_per_frame=fs, row_offset=2 * fs)
    else:
        kw = dict(weight=_randn(d, seed=3) * 0.1 + 1, bias=_randn(d, seed=4) * 0.1)
    c_ref, s_ref = ops.quantize_mxfp6(ops.layernorm_modulate(x, 1e-6, **kw))
    c, s = ops.layernorm_modulate_mxfp6(x, 1e-6, **kw)
    assert torch.equal(c, c_ref) and torch.equal(s, s_ref)
    assert int(s.max()) > 100 and int((mx.unpack_codes(c.cpu()) & 31).max()) >= 28   # live scales, codes of the top binade
    if form == "modulated":                                           # the row offset selects other frames' modulation
        c0, _ = ops.layernorm_modulate_mxfp6(x, 1e-6, **dict(kw, row_offset=0))
        assert not torch.equal(c0, c)


# ----------------------------------------------------------------------------------------- GEMM
def _dev_operands(c):
    return dev_operands(mx, c)


# The MXFP4 shapes (two to sixteen of this kernel's 128-element K-tiles; M and N tails, N % 256 != 0 throughout), and with the
# 128-element K-tile K = 128 (one tile: prologue and tail only), 384 (an odd tile count: the loop leaves after a first-parity
# tile) and 2176 (17 tiles in two split segments of 8 and 9: a segment of odd length whose successor starts at an odd tile).
# (257, 264, 2048) is the smallest shape that takes the split-K hand-off, as under MXFP4: the kernel tells plan_split_k (gemm8.hip)
# of K / 256 tiles, which splits the tiles of a partial round into S = min(CUs / tiles, 8, (K / 256) / 4) segments when S >= 2 -
# here 4 tiles on 256 CUs and 2048 / 256 = 8 give S = 2, and any K below 2048 gives S < 2.  (ops.gemm_mxfp6 provides the split
# workspace.)
@pytest.mark.parametrize("M,N,K", [(257, 264, 128), (257, 264, 256), (257, 264, 384), (300, 520, 512), (257, 264, 768),
                                   (513, 1536, 1024), (257, 264, 2048), (257, 264, 2176)])
def test_gemm_exact_case_bit_for_bit(ops, M, N, K):
    """tests/test_mxfp6_cpu.py verifies in fp64 that every partial sum of this case is exact in fp32: the output must be
    bf16(fp64 sum) bit for bit.  Asymmetric operands, scales that differ from row to row and from block to block."""
    c = mx.exact_case(M, N, K)
    total, _ = mx.product_fp64(c["a"], c["ea"], c["w"], c["ew"])
    out = ops.gemm_mxfp6(*_dev_operands(c))
    torch.cuda.synchronize()
    want = total.to(BF)
    bad = (_bits(out.cpu()) != _bits(want)).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), out.cpu()[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("K", [256, 1280])
@pytest.mark.parametrize("with_bias", [False, True])
def test_gemm_wide_scales(ops, K, with_bias):
    """Random codes, block exponents in [-20, 20].  Per element |got - want| <= 2^-7 |want| + K 2^-23 sum|terms| against fp64: one
    bf16 rounding, and twice the fp32 accumulation bound (K - 1) 2^-24 sum|terms|."""
    M, N = 130, 136
    g = torch.Generator().manual_seed(K + with_bias)
    c = mx.exact_case(M, N, K, seed=K)
    c["ea"] = torch.randint(-20, 21, c["ea"].shape, generator=g)
    c["ew"] = torch.randint(-20, 21, c["ew"].shape, generator=g)
    total, mag = mx.product_fp64(c["a"], c["ea"], c["w"], c["ew"])
    bias = (torch.randn(N, generator=g) * 64).to(BF) if with_bias else None
    want = total + bias.double() if with_bias else total
    out = ops.gemm_mxfp6(*_dev_operands(c), bias=bias.to(DEV) if with_bias else None)
    torch.cuda.synchronize()
    err = (out.cpu().double() - want).abs()
    bound = 2.0 ** -7 * want.abs() + K * 2.0 ** -23 * mag
    print(f"K={K} bias={with_bias}: worst err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


def test_gemm_fused_epilogues(ops):
    """Bias + GELU(tanh), and gate + residual, each within one bf16 ulp (2^-7 relative + 1e-5) of rtv_gemm's epilogue
    (y = bf16(acc + bias); y = bf16(act(y)); t = bf16(y * gate); out = bf16(res + t)) applied to the fp64 product."""
    M, N, K, F_ = 300, 520, 512, 3
    c = mx.exact_case(M, N, K, seed=11)
    total, _ = mx.product_fp64(c["a"], c["ea"], c["w"], c["ew"])
    total = total / 64                                                 # (the same power of two off both operands' scales)
    c["ea"], c["ew"] = c["ea"] - 3, c["ew"] - 3
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(N, generator=g).to(BF)
    gate = torch.randn(F_, N, generator=g).to(BF)
    res = (torch.randn(M, N, generator=g) * 4).to(BF)
    y = (total + bias.double()).to(BF)

    def close(got, want):
        return bool(((got.cpu().double() - want.double()).abs() <= 2.0 ** -7 * want.double().abs() + 1e-5).all())

    dev = _dev_operands(c)
    out = ops.gemm_mxfp6(*dev, bias=bias.to(DEV), act=1)
    assert close(out, torch.nn.functional.gelu(y.double(), approximate="tanh").to(BF))
    out = ops.gemm_mxfp6(*dev, bias=bias.to(DEV), gate=gate.to(DEV), gate_stride=N, rows_per_frame=M // F_, residual=res.to(DEV))
    t = (y.double() * gate.repeat_interleave(M // F_, dim=0).double()).to(BF)
    assert close(out, (res.double() + t.double()).to(BF))
    # a row offset moves the rows to the next frame's gate
    out = ops.gemm_mxfp6(*dev, bias=bias.to(DEV), gate=gate.to(DEV), gate_stride=N, rows_per_frame=M // F_, residual=res.to(DEV),
                         row_offset=M // F_)
    t = (y.double() * gate[[1, 2, 2]].repeat_interleave(M // F_, dim=0).double()).to(BF)
    assert close(out[:2 * (M // F_)], (res.double() + t.double()).to(BF)[:2 * (M // F_)])


# ----------------------------------------------------------------------------------------- model
def test_model_forward_against_the_mx_oracle_and_the_bf16_model(monkeypatch):
    """Three forwards (denoise, recompute, denoise) of the tiny model.
    Bar 1 (SURVEY 8c's rule, err(ours, gold) <= 2 x err(reference bf16, gold)): ours lies within twice the distance between the MX
    oracle in bf16 arithmetic and the MX oracle in the oracle's fp32 gold arithmetic - same quantisation points, same inputs; the
    bar comes from two evaluations of the restatement, never from the code under test.
    Bar 2: 0 < rel-L2(ours, our bf16 model) <= 1.25 x the MX oracle's own distance from the bf16 oracle (DESIGN config 5's factor).
    Then the same weights under enable_mxfp4(): the MXFP6 distance from the bf16 model must be the smaller one on each forward.
    Numbers of the run that delivered the mode: profiles/r17_mxfp6_parity.txt."""
    from oracle import wan_oracle as wo
    w = wo.make_weights(CFG, seed=0, text_dim=TEXT_DIM)
    lat, ctx = _inputs()
    t = torch.ones([1, 3], dtype=torch.int64) * 700
    t0 = torch.zeros([1, 3], dtype=torch.int64)
    plain = _oracle_forwards(wo, w, lat, ctx, t, t0, BF)
    monkeypatch.setattr(wo, "fp8_linear", mx.mx_linear)
    wmx = dict(w)
    wmx[wo.FP8_FLAG] = True
    mx_bf16 = _oracle_forwards(wo, wmx, lat, ctx, t, t0, BF)
    mx_gold = _oracle_forwards(wo, wmx, lat, ctx, t, t0, torch.float32)
    outs = {}
    for mode in ("bf16", "mxfp6", "mxfp4"):
        model, wr = _build(w)
        if mode == "mxfp6":
            assert model.enable_mxfp6() is model and model._cfg.use_fp8 == 4
        if mode == "mxfp4":
            assert model.enable_mxfp4() is model and model._cfg.use_fp8 == 3
        outs[mode] = _three_forwards(model, wr, lat, ctx, t, t0)
    ours_gold = [rel_l2(o, g) for o, g in zip(outs["mxfp6"], mx_gold)]
    oracle_gold = [rel_l2(o, g) for o, g in zip(mx_bf16, mx_gold)]
    ours_bf16 = [rel_l2(o, b) for o, b in zip(outs["mxfp6"], outs["bf16"])]
    oracle_bf16 = [rel_l2(o, b) for o, b in zip(mx_bf16, plain)]
    fmt = lambda vs: " ".join(f"{v:.3e}" for v in vs)
    print(f"mxfp6 (denoise, recompute, denoise) rel-L2: ours vs MX gold {fmt(ours_gold)} | MX oracle bf16 vs MX gold {fmt(oracle_gold)} | "
          f"ours vs our bf16 model {fmt(ours_bf16)} | MX oracle vs bf16 oracle {fmt(oracle_bf16)}")
    assert all(o <= 2 * r for o, r in zip(ours_gold, oracle_gold))
    assert all(0 < o <= 1.25 * r for o, r in zip(ours_bf16, oracle_bf16))
    # the reason for the mode: on the same weights MXFP6 lies closer to the bf16 model than MXFP4 does, on each forward
    fp4_bf16 = [rel_l2(o, b) for o, b in zip(outs["mxfp4"], outs["bf16"])]
    print(f"mxfp4 vs our bf16 model {fmt(fp4_bf16)} | mxfp6 / mxfp4 {fmt([a / b for a, b in zip(ours_bf16, fp4_bf16)])}")
    assert all(a < b for a, b in zip(ours_bf16, fp4_bf16))


def test_lora_requantises_mxfp6_in_place():
    """Adapter loaded, enable_mxfp6(), set_lora_scale, unload: the merged matrices are re-quantised into the existing code and
    block-scale tensors (same addresses, graphs dropped), and after the unload codes and scales are those of a fresh
    enable_mxfp6().  (tests/test_fp8_rows_gpu.py's test for the per-row fp8 mode, on this mode.)"""
    from oracle import wan_oracle as wo
    from realtime_video_amd.causal_model import CausalWanModel
    sd = wo.make_weights(CFG, seed=5, text_dim=TEXT_DIM)
    g = torch.Generator().manual_seed(9)
    lsd = {}
    for name, (o, k) in {"self_attn.q": (256, 256), "self_attn.v": (256, 256), "cross_attn.k": (256, 256), "ffn.0": (512, 256),
                         "ffn.2": (256, 512)}.items():
        lsd[f"blocks.1.{name}.lora_A.weight"] = (0.05 * torch.randn(8, k, generator=g)).to(BF)
        lsd[f"blocks.1.{name}.lora_B.weight"] = (0.05 * torch.randn(o, 8, generator=g)).to(BF)

    def model():
        m = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=TEXT_DIM, device=DEV)
        m.load_state_dict(sd)
        return m

    def state(m):
        torch.cuda.synchronize()
        return ({k: v.clone() for k, v in m._tensors.items() if v.dtype == torch.uint8}, {k: v.clone() for k, v in m._mx_scales.items()})

    def same(a, b):
        return all(x.keys() == y.keys() and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))

    def addresses(m):
        return {k: v.data_ptr() for k, v in list(m._tensors.items()) + [("s." + k, v) for k, v in m._mx_scales.items()]}

    fresh = model().enable_mxfp6()
    assert len(fresh._mx_scales) == 6 + 8 * 2 and fresh._mx_scales["L0.qkv_w"].shape == (768, 8) and fresh._tensors["L0.qkv_w"].shape == (768, 192)
    m = model()
    m.load_lora(lsd, scale=0.0, name="style")
    m.enable_mxfp6()
    assert same(state(m), state(fresh))                                 # strength 0: the bases
    ptrs, table, version = addresses(m), list(m._fp8_row_table), m._weights_version
    m.set_lora_scale("style", 1.0)
    merged = model()
    merged.load_lora(lsd, scale=1.0, name="style")
    merged.enable_mxfp6()
    assert same(state(m), state(merged)) and not same(state(m), state(fresh))
    assert not torch.equal(m._tensors["L1.qkv_w"][:256], fresh._tensors["L1.qkv_w"][:256])          # q rows moved,
    assert torch.equal(m._tensors["L1.qkv_w"][256:512], fresh._tensors["L1.qkv_w"][256:512])        # k rows did not
    assert addresses(m) == ptrs and list(m._fp8_row_table) == table and m._weights_version != version and not m._graphs
    m.unload_lora()
    assert same(state(m), state(fresh)) and m._lora_base == {} and m.lora_adapters() == {}


def test_mode_state_and_graph_replay():
    """A second enable_mxfp6() is a no-op, enable_fp8() / enable_mxfp4() raise and enable_mxfp6() raises on a model in one of those
    modes, load_lora() is refused, and a hipGraph-enabled forward replays with the bits of the eager one."""
    from oracle import wan_oracle as wo
    w = wo.make_weights(CFG, seed=0, text_dim=TEXT_DIM)
    lat, ctx = _inputs()
    t = torch.ones([1, 3], dtype=torch.int64) * 700
    model, wr = _build(w)
    model.enable_mxfp6()
    version, ptr = model._weights_version, model._tensors["L0.qkv_w"].data_ptr()
    assert model._tensors["L0.qkv_w"].dtype == torch.uint8 and tuple(model._tensors["L0.qkv_w"].shape) == (768, 192)
    assert model.enable_mxfp6() is model and model._weights_version == version and model._tensors["L0.qkv_w"].data_ptr() == ptr
    for other in (model.enable_fp8, lambda: model.enable_fp8("row"), model.enable_mxfp4):
        with pytest.raises(RuntimeError, match="reload the weights first"):
            other()
    for first in (lambda m: m.enable_fp8(), lambda m: m.enable_fp8("row"), lambda m: m.enable_mxfp4()):   # and the other order
        m2, _ = _build(w)
        first(m2)
        with pytest.raises(RuntimeError, match="reload the weights first"):
            m2.enable_mxfp6()
    g = torch.Generator().manual_seed(3)
    lsd = {"blocks.1.ffn.0.lora_A.weight": (0.05 * torch.randn(8, 256, generator=g)).to(BF),
           "blocks.1.ffn.0.lora_B.weight": (0.05 * torch.randn(512, 8, generator=g)).to(BF)}
    with pytest.raises(RuntimeError, match="load adapters first"):
        model.load_lora(lsd)
    cond = {"prompt_embeds": [ctx.to(DEV)]}

    def run():
        kv, ca = _caches()
        out, _ = wr(lat[0].to(DEV), cond, t.to(DEV), kv, ca, current_start=0)
        torch.cuda.synchronize()
        return out.cpu()

    ops_ = __import__("realtime_video_amd.ops", fromlist=["ops"])
    ops_.dispatch_counts(reset=True)
    eager = run()
    counts = ops_.dispatch_counts()
    assert counts.get("gemm_mxfp6_kernel<256x256>", 0) > 0                                   # its own counter,
    assert not [k for k in counts if "fp8" in k or "mxfp4" in k], counts                      # and no fp8 / MXFP4 GEMM
    model.use_hip_graphs = True
    first, replay = run(), run()
    assert torch.equal(_bits(first), _bits(eager)) and torch.equal(_bits(replay), _bits(eager))
