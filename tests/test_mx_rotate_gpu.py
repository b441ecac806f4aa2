"""The rotated MXFP4 / MXFP6 modes on the GPU (enable_mxfp4(rotate=True), enable_mxfp6(rotate=True); include/rtv_hip_mx_rotate.h):
the rotated quantisers and LayerNorm-fused quantisers bit for bit against the restatement tests/mx_rotate_oracle.py, the rotated
operands through the unchanged block-scaled GEMMs, then the model and its state.  tests/test_mx_rotate_cpu.py vets the inputs used
here: each mutant of the restatement changes codes or scale bytes on them."""
import ctypes
import functools

import pytest
import torch

import mx_rotate_oracle as ro
import mxfp4_oracle
import mxfp6_oracle
from conftest import rel_l2
from mx_cases import BF, CFG, DEV, TEXT_DIM, dev_operands
from mx_cases import build as _build, caches as _caches, inputs as _inputs, oracle_forwards as _oracle_forwards, three_forwards as _three_forwards
from mx_oracle import product_fp64

pytestmark = pytest.mark.gpu


class Fmt:
    """A format's oracle module with the names that differ between the two made equal."""

    def __init__(self, name, mx, mode, code_bytes, unpack, codes_of, k_multiple):
        self.name, self.mx, self.mode, self.code_bytes, self.unpack, self.codes_of = name, mx, mode, code_bytes, unpack, codes_of
        self.k_multiple = k_multiple

    def ops(self, what):
        from realtime_video_amd import ops
        return getattr(ops, what.format(self.name))


FORMATS = {"mxfp4": Fmt("mxfp4", mxfp4_oracle, 5, lambda d: d // 2, mxfp4_oracle.unpack_nibbles, mxfp4_oracle.nibbles, 256),
           "mxfp6": Fmt("mxfp6", mxfp6_oracle, 6, mxfp6_oracle.code_bytes, mxfp6_oracle.unpack_codes, mxfp6_oracle.sextets, 128)}


@pytest.fixture(params=list(FORMATS))
def f(request):
    return FORMATS[request.param]


@functools.lru_cache(maxsize=None)
def _rows(name, M, d):
    return ro.outlier_rows(FORMATS[name].mx, M, d)


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------------------- quantiser
# the wave path, its edge (2048), the workgroup path (2080: a short last K-tile of scales), and the most chunks per thread
@pytest.mark.parametrize("shift", [ro.SHIFT_WEIGHT, ro.SHIFT_ACT])
@pytest.mark.parametrize("M,d", [(5, 256), (5, 2048), (3, 2080), (2, 13824)])
def test_rotated_quantiser_matches_the_restatement_bit_for_bit(f, M, d, shift):
    x = _rows(f.name, M, d)
    v, e = ro.mx_quantize_rot(f.mx, x, shift)                          # the restatement, evaluated on the host
    codes, scales = f.ops("quantize_{}")(x.to(DEV), rotate_shift=shift)
    torch.cuda.synchronize()
    assert codes.shape == (M, f.code_bytes(d)) and scales.shape == (M, f.mx.scale_bytes(d))
    assert torch.equal(scales.cpu(), f.mx.pack_scales(e))              # scale bytes exactly (bytes no block owns stay 0)
    assert torch.equal(f.unpack(codes.cpu()), f.codes_of(v))           # codes modulo the sign of zero
    assert int(scales.max()) < 255
    plain, _ = f.ops("quantize_{}")(x.to(DEV))
    assert not torch.equal(plain, codes)                               # and the rotation is on


def test_a_single_value_spreads_to_32_equal_magnitudes(f):
    """shift = 0 on blocks of one non-zero value, at every place of the block: 32 codes of one magnitude (6 x 2^-2 = 1.5), signs of
    the Sylvester matrix - a wrong quad exchange leaves zeros or doubles."""
    x = torch.zeros(32, 256, dtype=BF)
    for blk in range(8):
        x[torch.arange(32), 32 * blk + torch.arange(32)] = 1.5
    codes, scales = f.ops("quantize_{}")(x.to(DEV), rotate_shift=0)
    torch.cuda.synchronize()
    got = f.unpack(codes.cpu(), canonical=False)
    six = int(f.codes_of(torch.tensor([6.0]))[0])
    sign_bit = int(f.codes_of(torch.tensor([-6.0]))[0]) - six
    assert bool(((got & (0xFF ^ sign_bit)) == six).all())
    v, e = ro.mx_quantize_rot(f.mx, x, 0)
    assert torch.equal(got, f.codes_of(v)) and torch.equal(scales.cpu(), f.mx.pack_scales(e))     # no zeros here: the signs too
    assert bool((scales.cpu()[:, [f.mx.scale_pos(b) for b in range(8)]] == 125).all())


def test_rotated_quantiser_with_padded_row_strides(f):
    M, d = 5, 2080
    x = _rows(f.name, M, d)
    v, e = ro.mx_quantize_rot(f.mx, x, ro.SHIFT_ACT)
    cb, sb = f.code_bytes(d), f.mx.scale_bytes(d)
    xw = torch.zeros(M, d + 64, dtype=BF, device=DEV)
    xw[:, :d] = x.to(DEV)
    cw = torch.full((M, cb + 12), 0x55, dtype=torch.uint8, device=DEV)
    sw = torch.full((M, sb + 5), 0x55, dtype=torch.uint8, device=DEV)
    codes, scales = f.ops("quantize_{}")(xw[:, :d], codes=cw[:, :cb], scales=sw[:, :sb], rotate_shift=ro.SHIFT_ACT)
    torch.cuda.synchronize()
    assert torch.equal(f.unpack(codes.cpu()), f.codes_of(v))
    want = f.mx.pack_scales(e)
    owned = torch.zeros(sb, dtype=torch.bool)
    owned[[f.mx.scale_pos(b) for b in range(d // 32)]] = True
    assert torch.equal(scales.cpu()[:, owned], want[:, owned])
    assert bool((scales.cpu()[:, ~owned] == 0x55).all())               # bytes of blocks the short last K-tile lacks: not written
    assert bool((cw[:, cb:] == 0x55).all()) and bool((sw[:, sb:] == 0x55).all())


# ----------------------------------------------------------------------------------------- LayerNorm + modulate + rotate + quantise
@pytest.mark.parametrize("d", [256, 2080, 5120, 8192])                 # 2080: a short last K-tile; 8192: all four chunks of every thread
@pytest.mark.parametrize("form", ["modulated", "affine", "plain"])
def test_fused_layernorm_quantiser_equals_the_two_kernels_bit_for_bit(f, d, form):
    from realtime_video_amd import ops
    fs, M = 3, 7                                                        # 7 rows over 3 frames
    x = _randn(M, d, seed=1, scale=2.0)
    if form == "modulated":
        emod = _randn(4, 6, d, seed=2, scale=0.5)
        kw = dict(shift=emod[0, 0], scale=emod[0, 1], frame_stride=6 * d, rows_per_frame=fs)
    elif form == "affine":
        kw = dict(weight=_randn(d, seed=3) * 0.1 + 1, bias=_randn(d, seed=4) * 0.1)
    else:
        kw = {}
    c_ref, s_ref = f.ops("quantize_{}")(ops.layernorm_modulate(x, 1e-6, **kw), rotate_shift=ro.SHIFT_ACT)
    c, s = f.ops("layernorm_modulate_{}_rot")(x, 1e-6, **kw)
    assert torch.equal(c, c_ref) and torch.equal(s, s_ref)
    assert int(s.max()) > 100
    c_plain, _ = f.ops("layernorm_modulate_{}")(x, 1e-6, **kw)
    assert not torch.equal(c_plain, c)
    if form == "modulated":                                            # the row offset selects other frames' modulation
        c1, _ = f.ops("layernorm_modulate_{}_rot")(x, 1e-6, **dict(kw, row_offset=fs))
        assert not torch.equal(c1, c)


# ----------------------------------------------------------------------------------------- through the unchanged GEMM
def _device_product(f, x, w, rotate):
    quantize, gemm = f.ops("quantize_{}"), f.ops("gemm_{}")
    kx, kw = (dict(rotate_shift=ro.SHIFT_ACT), dict(rotate_shift=ro.SHIFT_WEIGHT)) if rotate else ({}, {})
    ac, asc = quantize(x.to(DEV), **kx)
    wc, wsc = quantize(w.to(DEV), **kw)
    out = gemm(ac, asc, wc, wsc)
    torch.cuda.synchronize()
    return out.cpu()


def test_rotated_operands_through_the_unchanged_gemm(f):
    """M, N, K = 64, 96, 512.  Per element |got - want| <= 2^-7 |want| + K 2^-23 sum|terms| against the float64 product of the
    restatement's dequantised rotated operands (tests/test_mxfp4_gpu.py::test_gemm_wide_scales' bound: one bf16 rounding and twice
    the fp32 accumulation bound).  Then what the rotation is for, on the device: with every 32nd activation column times 32 the
    rotated result's rel-L2 against x w^T in float64 is at most 0.85 of the unrotated result's."""
    x, w = ro.product_operands()
    K = x.shape[1]
    for xs in (x, ro.outlier_columns(x)):
        a, ea = ro.mx_quantize_rot(f.mx, xs, ro.SHIFT_ACT)
        b, eb = ro.mx_quantize_rot(f.mx, w, ro.SHIFT_WEIGHT)
        want, mag = product_fp64(a, ea, b, eb)
        got = _device_product(f, xs, w, True)
        err = (got.double() - want).abs()
        bound = 2.0 ** -7 * want.abs() + K * 2.0 ** -23 * mag
        print(f"{f.name}: worst err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= bound).all())
    xo = ro.outlier_columns(x)
    exact = xo.double() @ w.double().t()
    e_rot, e_plain = rel_l2(_device_product(f, xo, w, True), exact), rel_l2(_device_product(f, xo, w, False), exact)
    print(f"{f.name} device rel-L2 vs x w^T, every 32nd column x32: unrotated {e_plain:.4f} rotated {e_rot:.4f} (ratio {e_rot / e_plain:.3f})")
    assert e_rot <= 0.85 * e_plain


def test_a_gate_table_that_ends_in_front_of_the_last_frame_is_never_read_past_its_end(f):
    """ops.gemm_mxfp4 / gemm_mxfp6 with a row offset that moves the last rows past the gate's last frame (what
    tests/test_mxfp4_gpu.py::test_gemm_fused_epilogues does in its last call): the epilogue would read the table past its
    allocation, so the wrapper hands it over continued with zeros.  The output is that of a table with a zero frame appended, bit
    for bit, and the rows past the table are the residual."""
    M, N, K, F_ = 300, 520, 512, 3
    dev = dev_operands(f.mx, f.mx.exact_case(M, N, K, seed=11))
    g = torch.Generator().manual_seed(5)
    gate = torch.randn(F_, N, generator=g).to(BF)
    res = (torch.randn(M, N, generator=g) * 4).to(BF).to(DEV)
    kw = dict(gate_stride=N, rows_per_frame=M // F_, residual=res, row_offset=M // F_)
    short = f.ops("gemm_{}")(*dev, gate=gate.to(DEV), **kw)
    whole = f.ops("gemm_{}")(*dev, gate=torch.cat([gate, torch.zeros(1, N, dtype=BF)]).to(DEV), **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(short), _bits(whole))
    assert torch.equal(_bits(short[2 * (M // F_):]), _bits(res[2 * (M // F_):]))
    assert not torch.equal(_bits(short[:2 * (M // F_)]), _bits(res[:2 * (M // F_)]))


# ----------------------------------------------------------------------------------------- model
def _enable(model, f, rotate=True):
    return getattr(model, "enable_" + f.name)(rotate=rotate)


def test_model_forward_against_the_rotated_oracle_and_the_bf16_model(f, monkeypatch):
    """Three forwards (denoise, recompute, denoise) of the tiny model, the two bars of
    tests/test_mxfp4_gpu.py::test_model_forward_against_the_mx_oracle_and_the_bf16_model with mx_linear_rot in the oracle.
    Bar 1: err(ours, gold) <= 2 x err(oracle in bf16 arithmetic, gold) - two evaluations of the restatement set the bar.
    Bar 2: 0 < rel-L2(ours, our bf16 model) <= 1.25 x the rotated oracle's own distance from the bf16 oracle.
    And the outputs differ from the unrotated mode's: the mode is on.  Numbers of the run that delivered the mode:
    profiles/r18_mx_rotate_parity.txt."""
    from oracle import wan_oracle as wo
    w = wo.make_weights(CFG, seed=0, text_dim=TEXT_DIM)
    lat, ctx = _inputs()
    t = torch.ones([1, 3], dtype=torch.int64) * 700
    t0 = torch.zeros([1, 3], dtype=torch.int64)
    plain = _oracle_forwards(wo, w, lat, ctx, t, t0, BF)
    monkeypatch.setattr(wo, "fp8_linear", ro.mx_linear_rot(f.mx))
    wmx = dict(w)
    wmx[wo.FP8_FLAG] = True
    mx_bf16 = _oracle_forwards(wo, wmx, lat, ctx, t, t0, BF)
    mx_gold = _oracle_forwards(wo, wmx, lat, ctx, t, t0, torch.float32)
    outs = {}
    for mode in ("bf16", "rotated", "unrotated"):
        model, wr = _build(w)
        if mode != "bf16":
            assert _enable(model, f, mode == "rotated") is model and model._cfg.use_fp8 == (f.mode if mode == "rotated" else f.mode - 2)
        outs[mode] = _three_forwards(model, wr, lat, ctx, t, t0)
    ours_gold = [rel_l2(o, g) for o, g in zip(outs["rotated"], mx_gold)]
    oracle_gold = [rel_l2(o, g) for o, g in zip(mx_bf16, mx_gold)]
    ours_bf16 = [rel_l2(o, b) for o, b in zip(outs["rotated"], outs["bf16"])]
    oracle_bf16 = [rel_l2(o, b) for o, b in zip(mx_bf16, plain)]
    unrotated_bf16 = [rel_l2(o, b) for o, b in zip(outs["unrotated"], outs["bf16"])]
    fmt = lambda vs: " ".join(f"{v:.3e}" for v in vs)
    print(f"{f.name} rotated (denoise, recompute, denoise) rel-L2: ours vs MX gold {fmt(ours_gold)} | MX oracle bf16 vs MX gold {fmt(oracle_gold)} | "
          f"ours vs our bf16 model {fmt(ours_bf16)} | MX oracle vs bf16 oracle {fmt(oracle_bf16)} | unrotated mode vs our bf16 model {fmt(unrotated_bf16)}")
    assert all(o <= 2 * r for o, r in zip(ours_gold, oracle_gold))
    assert all(0 < o <= 1.25 * r for o, r in zip(ours_bf16, oracle_bf16))
    assert all(not torch.equal(_bits(a), _bits(b)) for a, b in zip(outs["rotated"], outs["unrotated"]))


def test_lora_requantises_the_rotated_mode_in_place(f):
    """Adapter loaded, rotated enable, set_lora_scale, unload: the merged matrices are re-quantised by the rotated quantiser into the
    existing code and block-scale tensors, and after the unload codes and scales are those of a fresh rotated enable, bit for bit
    (tests/test_mxfp4_gpu.py's test on the rotated modes)."""
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

    fresh = _enable(model(), f)
    assert not same(state(fresh), state(_enable(model(), f, rotate=False)))                          # other codes than the unrotated mode's
    # the weights' codes are the rotated quantiser's at the weight shift
    wq = sd["blocks.0.ffn.0.weight"].to(BF)
    v, e = ro.mx_quantize_rot(f.mx, wq, ro.SHIFT_WEIGHT)
    assert torch.equal(f.unpack(fresh._tensors["L0.ffn0_w"].cpu()), f.codes_of(v))
    assert torch.equal(fresh._mx_scales["L0.ffn0_w"].cpu(), f.mx.pack_scales(e))
    m = model()
    m.load_lora(lsd, scale=0.0, name="style")
    _enable(m, f)
    assert same(state(m), state(fresh))                                 # strength 0: the bases
    ptrs, table, version = addresses(m), list(m._fp8_row_table), m._weights_version
    m.set_lora_scale("style", 1.0)
    merged = model()
    merged.load_lora(lsd, scale=1.0, name="style")
    _enable(merged, f)
    assert same(state(m), state(merged)) and not same(state(m), state(fresh))
    assert addresses(m) == ptrs and list(m._fp8_row_table) == table and m._weights_version != version and not m._graphs
    m.unload_lora()
    assert same(state(m), state(fresh)) and m._lora_base == {} and m.lora_adapters() == {}


def test_mode_state_and_graph_replay(f):
    """use_fp8 is 5 / 6, code and scale tensors have the shapes of modes 3 / 4, a second enable is a no-op, every other enable_* is
    refused, load_lora() is refused, and a hipGraph-enabled forward replays with the bits of the eager one."""
    from oracle import wan_oracle as wo
    w = wo.make_weights(CFG, seed=0, text_dim=TEXT_DIM)
    lat, ctx = _inputs()
    t = torch.ones([1, 3], dtype=torch.int64) * 700
    model, wr = _build(w)
    _enable(model, f)
    assert model._cfg.use_fp8 == f.mode
    version, ptr = model._weights_version, model._tensors["L0.qkv_w"].data_ptr()
    assert model._tensors["L0.qkv_w"].dtype == torch.uint8 and tuple(model._tensors["L0.qkv_w"].shape) == (768, f.code_bytes(256))
    assert tuple(model._mx_scales["L0.qkv_w"].shape) == (768, 8) and tuple(model._mx_scales["L0.ffn2_w"].shape) == (256, 16)
    assert _enable(model, f) is model and model._weights_version == version and model._tensors["L0.qkv_w"].data_ptr() == ptr
    for call in (lambda: model.enable_fp8(), lambda: model.enable_fp8("row"), lambda: model.enable_mxfp4(), lambda: model.enable_mxfp6(),
                 lambda: _enable(model, FORMATS["mxfp6" if f.name == "mxfp4" else "mxfp4"])):
        with pytest.raises(RuntimeError, match="reload the weights first"):
            call()
    assert model._cfg.use_fp8 == f.mode and model._weights_version == version
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
    assert counts.get(f"gemm_{f.name}_kernel<256x256>", 0) > 0 and "gemm_fp8_kernel<256x256>" not in counts   # the unrotated mode's GEMM
    model.use_hip_graphs = True
    first, replay = run(), run()
    assert torch.equal(_bits(first), _bits(eager)) and torch.equal(_bits(replay), _bits(eager))


# ----------------------------------------------------------------------------------------- refusals, before any launch
def test_bad_arguments_are_refused_without_a_launch(f):
    """Unknown shifts, d % 32 != 0 and misaligned pointers return the documented errors; the outputs stay untouched."""
    from realtime_video_amd import _lib, ops
    lib = _lib.load()
    x = _randn(2, 64, seed=5)
    codes = torch.full((2, 64), 0x55, dtype=torch.uint8, device=DEV)
    scales = torch.full((2, 8), 0x55, dtype=torch.uint8, device=DEV)
    quantize = getattr(lib, f"rtv_quantize_{f.name}_rot")
    layernorm = getattr(lib, f"rtv_layernorm_modulate_{f.name}_rot")
    i64 = ctypes.c_int64

    def q(xp=x.data_ptr(), d=64, cp=codes.data_ptr(), shift=3):
        st = quantize(xp, i64(64), 2, d, cp, i64(64), scales.data_ptr(), i64(8), shift, None)
        return st, lib.rtv_last_error().decode()

    for kw, what in ((dict(shift=-1), "shift must be in 0 .. 5"), (dict(shift=6), "shift must be in 0 .. 5"),
                     (dict(d=48), "d must be a multiple of 32"), (dict(xp=x.data_ptr() + 8), "x must be 16-byte aligned"),
                     (dict(cp=codes.data_ptr() + 2), "codes 4-byte aligned")):
        st, msg = q(**kw)
        assert st != 0 and msg.startswith(f"quantize_{f.name}: ") and what in msg, (kw, msg)
    for kw, what in ((dict(d=48), "d must be a multiple of 32 and <= 8192"), (dict(xp=x.data_ptr() + 8), "x must be 16-byte aligned"),
                     (dict(cp=codes.data_ptr() + 2), "codes 4-byte aligned")):
        a = dict(dict(xp=x.data_ptr(), d=64, cp=codes.data_ptr()), **kw)
        st = layernorm(a["xp"], a["cp"], i64(64), scales.data_ptr(), i64(8), 2, a["d"], 1e-6, None, None, 0, 0, 0, None, None, None)
        msg = lib.rtv_last_error().decode()
        assert st != 0 and msg.startswith(f"layernorm_modulate_{f.name}: ") and what in msg, (kw, msg)
    with pytest.raises(ValueError, match="rotate_shift must be in 0 .. 5"):
        f.ops("quantize_{}")(x, rotate_shift=6)
    torch.cuda.synchronize()
    assert bool((codes == 0x55).all()) and bool((scales == 0x55).all())
