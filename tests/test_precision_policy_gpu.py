"""The per-Linear precision policy on the GPU (CausalWanModel.set_linear_precision; rtv_dit_config.use_fp8 == 7): bit-for-bit
identities against the pure modes and the bf16 model, a mixed forward against the composed oracle of tests/mixed_oracle.py, state and
refusals, the argument checks of the native side, and LoRA.  All on the tiny model of tests/mx_cases.py (the smallest widths MXFP4
takes) and its three forwards (denoise, recompute, denoise)."""
import ctypes
import functools
import types

import pytest
import torch

import mixed_oracle
import mxfp4_oracle
import mxfp6_oracle
from conftest import rel_l2
from mx_cases import BF, CFG, DEV, TEXT_DIM
from mx_cases import build as _build, caches as _caches, inputs as _inputs, oracle_forwards as _oracle_forwards, three_forwards as _three_forwards

pytestmark = pytest.mark.gpu

L = CFG["num_layers"]
T = torch.ones([1, 3], dtype=torch.int64) * 700
T0 = torch.zeros([1, 3], dtype=torch.int64)
# test 4's policy: four modes in one forward, a layer override, a top-level Linear kept in bf16
MIXED = {"default": "fp8_row", "ffn0": "mxfp4", "ffn2": "mxfp4", "head": "bf16", "L0.qkv": "mxfp6"}
PURE = {"fp8": lambda m: m.enable_fp8(), "fp8_row": lambda m: m.enable_fp8("row"), "mxfp4": lambda m: m.enable_mxfp4(),
        "mxfp6": lambda m: m.enable_mxfp6(), "mxfp4_rot": lambda m: m.enable_mxfp4(rotate=True),
        "mxfp6_rot": lambda m: m.enable_mxfp6(rotate=True)}


@functools.lru_cache(maxsize=None)
def _weights(seed=0):
    from oracle import wan_oracle as wo
    return wo.make_weights(CFG, seed=seed, text_dim=TEXT_DIM)


def _zeroed(names):
    """The weights with the Linears `names` (state-dict names inside a block) zeroed, weight and bias, in every layer."""
    w = dict(_weights())
    for l in range(L):
        for n in names:
            for part in ("weight", "bias"):
                w[f"blocks.{l}.{n}.{part}"] = torch.zeros_like(w[f"blocks.{l}.{n}.{part}"])
    return w


def _run(w, setup=None):
    """Three forwards of a fresh model on the weights `w` after setup(model) -> (model, outputs)."""
    lat, ctx = _inputs()
    model, wr = _build(w)
    if setup is not None:
        setup(model)
    return model, _three_forwards(model, wr, lat, ctx, T, T0)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _pure_outputs(mode):
    """The three forwards of the plain model (mode "bf16") or of a pure mode, computed once and shared; never modified."""
    return _run(_weights(), PURE.get(mode))[1]


# ----------------------------------------------------------------------------------------- 1. uniform policy = pure mode
@pytest.mark.parametrize("mode", list(PURE))
def test_uniform_policy_equals_the_pure_mode_bit_for_bit(mode):
    model, outs = _run(_weights(), lambda m: m.set_linear_precision({"default": mode}))
    assert model._cfg.use_fp8 == 7 and set(model.linear_precision().values()) == {mode}
    assert _same(outs, _pure_outputs(mode))
    assert not _same(outs, _pure_outputs("bf16"))


@pytest.mark.parametrize("mode", list(PURE))
def test_uniform_policy_prepares_the_state_of_the_pure_mode(mode):
    """Test 1 compares outputs; this one the prepared state, without a forward: after the enable_* call and after the uniform policy
    every Linear weight has the same dtype, shape and bits, the scale stores the same keys and bits, the per-tensor scales are equal,
    and rtv_dit_config.use_fp8 is the mode's number and 7."""
    from realtime_video_amd import precision_policy as pp
    a, _ = _build(_weights())
    PURE[mode](a)
    b, _ = _build(_weights())
    b.set_linear_precision({"default": mode})
    torch.cuda.synchronize()
    assert a._cfg.use_fp8 == pp.MODE_NAMES.index(mode) and b._cfg.use_fp8 == 7
    for name in pp.linear_names(L):
        x, y = a._tensors[name + "_w"], b._tensors[name + "_w"]
        assert x.dtype == y.dtype != BF and x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    for store in ("_mx_scales", "_fp8_row_scales"):
        sa, sb = getattr(a, store), getattr(b, store)
        assert list(sa) == list(sb), store
        assert all(sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]) for k in sa), store
    assert len(a._mx_scales) + len(a._fp8_row_scales) == (0 if mode == "fp8" else 6 + 8 * L)
    assert list(a._fp8_scales) == list(b._fp8_scales) and (all(s > 0 for s in a._fp8_scales) if mode == "fp8" else not any(a._fp8_scales))


# ----------------------------------------------------------------------------------------- 2. no leak into unselected Linears
@pytest.mark.parametrize("mode", ["mxfp4", "mxfp6"])
def test_unselected_linears_stay_bf16_bit_for_bit(mode):
    """ffn.2 is zero in every layer, so the FFN branch adds gate * 0 whatever ffn.0 / ffn.2 compute: with only those two in an MX
    mode, every difference from the bf16 model would come from a Linear the policy did not select.  (The bf16 model runs with
    fold_cross_v off: the cross-attention V fold stays off under a policy, and it is another summation order.)"""
    fmt = {"mxfp4": mxfp4_oracle, "mxfp6": mxfp6_oracle}[mode]
    w = _zeroed(["ffn.2"])
    v, e = fmt.mx_quantize(w["blocks.0.ffn.2.weight"])                   # the defined all-zero block: zero codes, exponent -127
    assert not bool(v.any()) and bool((e == -127).all())
    model, outs = _run(w, lambda m: m.set_linear_precision({"ffn0": mode, "ffn2": mode}))
    assert model._cfg.use_fp8 == 7 and model._tensors["L0.ffn2_w"].dtype == torch.uint8 and model._tensors["L0.qkv_w"].dtype == BF
    assert not bool(model._tensors["L1.ffn2_w"].any())

    def plain(m):
        m.fold_cross_v = False

    _, ref = _run(w, plain)
    assert _same(outs, ref)


# ----------------------------------------------------------------------------------------- 3. selected Linears run their mode
@pytest.mark.parametrize("mode", ["mxfp4", "mxfp6"])
def test_selected_linears_run_their_mode_bit_for_bit(mode):
    """self_attn.o and cross_attn.o are zero in every layer: both attention branches add zero whatever their projections compute.
    With the attention projections in bf16 and everything else in the MX mode, the forward must be the pure MX mode's: the
    top-level Linears and the FFN (LayerNorm-fused quantiser included) really run it."""
    fmt = {"mxfp4": mxfp4_oracle, "mxfp6": mxfp6_oracle}[mode]
    w = _zeroed(["self_attn.o", "cross_attn.o"])
    for n in ("self_attn.o", "cross_attn.o"):
        v, e = fmt.mx_quantize(w[f"blocks.1.{n}.weight"])
        assert not bool(v.any()) and bool((e == -127).all())
    policy = {"default": mode, "qkv": "bf16", "o": "bf16", "cq": "bf16", "ck": "bf16", "cv": "bf16", "co": "bf16"}
    model, outs = _run(w, lambda m: m.set_linear_precision(policy))
    assert model._cfg.use_fp8 == 7 and model._tensors["L0.ffn0_w"].dtype == torch.uint8 and model._tensors["L0.co_w"].dtype == BF
    pure, ref = _run(w, PURE[mode])
    assert not bool(pure._tensors["L0.o_w"].any()) and not bool(pure._tensors["L1.co_w"].any())      # zero codes on the device too
    assert _same(outs, ref)
    _, bf = _run(w)
    assert not _same(outs, bf)                                          # and they are not the bf16 model's


# ----------------------------------------------------------------------------------------- 4. a mixed forward against the composed oracle
def test_mixed_forward_against_the_composed_oracle(monkeypatch):
    """Bars as in the tests of the pure modes, from two evaluations of the restatements and never from the code under test:
    rel-L2(ours, mixed oracle in fp32 gold) <= 2 x rel-L2(mixed oracle in bf16, mixed oracle in fp32 gold) on each forward, and
    0 < rel-L2(ours, our bf16 model) <= 1.25 x rel-L2(mixed oracle in bf16, bf16 oracle).  The mixed output is none of the pure
    modes'.  Numbers of the run that delivered the policy: profiles/r21_mixed_precision_parity.txt."""
    from oracle import wan_oracle as wo
    w = _weights()
    lat, ctx = _inputs()
    model, outs = _run(w, lambda m: m.set_linear_precision(MIXED))
    modes = model.linear_precision()
    assert model._cfg.use_fp8 == 7
    assert (modes["L0.qkv"], modes["L1.qkv"], modes["L1.ffn0"], modes["L0.ffn2"], modes["head"], modes["text0"], modes["L1.co"]) == \
        ("mxfp6", "fp8_row", "mxfp4", "mxfp4", "bf16", "fp8_row", "fp8_row")
    plain = _oracle_forwards(wo, w, lat, ctx, T, T0, BF)
    linear, served = mixed_oracle.dispatcher(wo, w, L, modes)
    monkeypatch.setattr(wo, "fp8_linear", linear)
    wm = dict(w)
    wm[wo.FP8_FLAG] = True
    mixed_bf16 = _oracle_forwards(wo, wm, lat, ctx, T, T0, BF)
    assert set(served) == set(modes)                                    # every Linear went through the dispatcher
    mixed_gold = _oracle_forwards(wo, wm, lat, ctx, T, T0, torch.float32)
    bf16 = _pure_outputs("bf16")
    ours_gold = [rel_l2(o, g) for o, g in zip(outs, mixed_gold)]
    oracle_gold = [rel_l2(o, g) for o, g in zip(mixed_bf16, mixed_gold)]
    ours_bf16 = [rel_l2(o, b) for o, b in zip(outs, bf16)]
    oracle_bf16 = [rel_l2(o, b) for o, b in zip(mixed_bf16, plain)]
    fmt = lambda vs: " ".join(f"{v:.3e}" for v in vs)
    print(f"mixed policy (denoise, recompute, denoise) rel-L2: ours vs mixed gold {fmt(ours_gold)} | mixed oracle bf16 vs mixed gold "
          f"{fmt(oracle_gold)} | ours vs our bf16 model {fmt(ours_bf16)} | mixed oracle vs bf16 oracle {fmt(oracle_bf16)}")
    for mode in PURE:
        d = [rel_l2(o, p) for o, p in zip(outs, _pure_outputs(mode))]
        print(f"mixed policy vs pure {mode}: {fmt(d)}")
    assert all(o <= 2 * r for o, r in zip(ours_gold, oracle_gold))
    assert all(0 < o <= 1.25 * r for o, r in zip(ours_bf16, oracle_bf16))
    for mode in PURE:
        assert not any(torch.equal(_bits(o), _bits(p)) for o, p in zip(outs, _pure_outputs(mode))), mode


# ----------------------------------------------------------------------------------------- 5. state, refusals, graph replay
def test_state_refusals_and_graph_replay():
    w = _weights()
    lat, ctx = _inputs()
    model, wr = _build(w)
    assert set(model.linear_precision().values()) == {"bf16"}
    assert model.set_linear_precision({"default": "bf16", "qkv": "bf16"}) is model and model._cfg.use_fp8 == 0      # all bf16: untouched
    assert model._tensors["L0.qkv_w"].dtype == BF
    assert model.set_linear_precision(MIXED) is model and model._cfg.use_fp8 == 7
    version, ptr = model._weights_version, model._tensors["L0.qkv_w"].data_ptr()
    same = {"L0.qkv": "mxfp6", "head": "bf16", "ffn2": "mxfp4", "ffn0": "mxfp4", "default": "fp8_row", "L1.o": "fp8_row"}   # resolves alike
    assert model.set_linear_precision(same) is model and model._weights_version == version
    assert model._tensors["L0.qkv_w"].data_ptr() == ptr
    names = model.linear_precision()
    assert list(names) == ["text0", "text2", "time0", "time2", "tproj", "head"] + \
        [f"L{l}.{k}" for l in range(L) for k in ("qkv", "o", "cq", "ck", "cv", "co", "ffn0", "ffn2")]
    assert names["L0.qkv"] == "mxfp6" and names["L1.qkv"] == "fp8_row" and names["head"] == "bf16" and names["L1.ffn2"] == "mxfp4"
    for other in (lambda: model.set_linear_precision({"default": "fp8_row"}), model.enable_fp8, lambda: model.enable_fp8("row"),
                  model.enable_mxfp4, model.enable_mxfp6, lambda: model.enable_mxfp4(rotate=True), lambda: model.enable_mxfp6(rotate=True)):
        with pytest.raises(RuntimeError, match="reload the weights first"):
            other()
    for first in PURE.values():                                         # and the other order
        m2, _ = _build(w)
        first(m2)
        with pytest.raises(RuntimeError, match="reload the weights first"):
            m2.set_linear_precision(MIXED)
    with pytest.raises(RuntimeError, match="load adapters first"):
        model.load_lora({"blocks.1.ffn.0.lora_A.weight": torch.zeros(8, 256, dtype=BF), "blocks.1.ffn.0.lora_B.weight": torch.zeros(512, 8, dtype=BF)})
    with pytest.raises(ValueError, match="unknown key"):
        model.set_linear_precision({"ffn": "mxfp4"})
    from realtime_video_amd.causal_model import CausalWanModel
    with pytest.raises(RuntimeError, match="load weights before"):
        CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=TEXT_DIM).set_linear_precision(MIXED)
    # context parallelism, in either order
    m3, wr3 = _build(w)
    m3.context_parallel = types.SimpleNamespace(world=2)
    with pytest.raises(RuntimeError, match="context parallelism"):
        m3.set_linear_precision(MIXED)
    assert m3._cfg.use_fp8 == 0
    m3.context_parallel = None
    m3.set_linear_precision(MIXED)
    m3.context_parallel = types.SimpleNamespace(world=2)
    kv, ca = _caches()
    with pytest.raises(RuntimeError, match="context parallelism"):
        wr3(lat[0].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=0)
    # hipGraph replay
    cond = {"prompt_embeds": [ctx.to(DEV)]}

    def run():
        kv, ca = _caches()
        out, _ = wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
        torch.cuda.synchronize()
        return out.cpu()

    from realtime_video_amd import ops
    ops.dispatch_counts(reset=True)
    eager = run()
    counts = ops.dispatch_counts()
    for part in ("gemm_mxfp6", "gemm_mxfp4", "fp8"):                    # the GEMMs of three quantised modes ran in one forward
        assert any(part in k and n > 0 for k, n in counts.items()), (part, counts)
    model.use_hip_graphs = True
    first, replay = run(), run()
    assert torch.equal(_bits(first), _bits(eager)) and torch.equal(_bits(replay), _bits(eager))
    # a reload is a bf16 model again
    model.load_state_dict(w)
    assert model._cfg.use_fp8 == 0 and set(model.linear_precision().values()) == {"bf16"} and not model._graphs
    assert not model._w.fp8_row_scales and not model._w.fp8_scales and model._tensors["L0.qkv_w"].dtype == BF      # a fresh weight table
    model.use_hip_graphs = False
    assert torch.equal(_bits(run()), _bits(_pure_outputs("bf16")[0]))


# ----------------------------------------------------------------------------------------- 6. the native argument checks
def test_native_side_refuses_bad_mode_tables_before_any_launch():
    """Each bad table makes the forward return an error with a message - an argument check in front of the first launch - and the
    next valid forward gives the bits it gave before."""
    w = _weights()
    lat, ctx = _inputs()
    model, wr = _build(w)
    model.set_linear_precision(MIXED)
    cond = {"prompt_embeds": [ctx.to(DEV)]}

    def run():
        kv, ca = _caches()
        out, _ = wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
        torch.cuda.synchronize()
        return out.cpu()

    good = run()
    assert torch.equal(_bits(good), _bits(run()))
    table, row_table = model._linear_modes, model._fp8_row_table
    ffn0 = 6 + 8 * 1 + 6                                                # L1.ffn0: MXFP4
    assert model.linear_precision()["L1.ffn0"] == "mxfp4" and table[ffn0] == 3 and row_table[ffn0]

    n = 6 + 8 * L                                                       # linear_modes: the entry behind the scale entries
    assert len(row_table) == n + 1 and row_table[n] == ctypes.addressof(table)
    row_table[n] = None
    with pytest.raises(RuntimeError, match="use_fp8 == 7 needs linear_modes"):
        run()
    row_table[n] = ctypes.addressof(table)
    assert torch.equal(_bits(run()), _bits(good))
    model._w.fp8_row_scales = None                                      # no table at all
    with pytest.raises(RuntimeError, match="use_fp8 == 7 needs linear_modes"):
        run()
    model._w.fp8_row_scales = ctypes.cast(row_table, ctypes.POINTER(ctypes.c_void_p))
    assert torch.equal(_bits(run()), _bits(good))

    table[ffn0] = 9
    with pytest.raises(RuntimeError, match=r"L1\.ffn0: mode 9 is not a mode"):
        run()
    table[ffn0] = 3
    assert torch.equal(_bits(run()), _bits(good))

    scales = row_table[ffn0]
    row_table[ffn0] = None
    with pytest.raises(RuntimeError, match=r"L1\.ffn0: mode 3 needs its rtv_dit_weights.fp8_row_scales entry"):
        run()
    row_table[ffn0] = scales
    assert torch.equal(_bits(run()), _bits(good))

    # the workspace of the mixed mode is the union: no smaller than any pure mode's
    from realtime_video_amd import _lib
    cfg = type(model._cfg).from_buffer_copy(model._cfg)
    sizes = {}
    for mode in range(8):
        cfg.use_fp8 = mode
        sizes[mode] = _lib.load().rtv_dit_workspace_bytes(ctypes.byref(cfg), 3, 30, 52)
    assert sizes[7] == max(sizes.values()) == sizes[2]


# ----------------------------------------------------------------------------------------- 7. LoRA
def test_lora_requantises_each_linear_with_its_own_mode_in_place():
    """Adapter on qkv and ffn.0 of both layers, the policy of test 4 (L0.qkv MXFP6, L1.qkv fp8 per row, ffn0 MXFP4),
    set_lora_scale, unload: every merged matrix is re-quantised with its own mode into the existing code and scale tensors (same
    addresses, graphs dropped), and after the unload every tensor is that of a fresh model under the same policy.
    (tests/test_mxfp6_gpu.py's test_lora_requantises_mxfp6_in_place, on a policy.)"""
    from realtime_video_amd.causal_model import CausalWanModel
    sd = _weights(5)
    g = torch.Generator().manual_seed(9)
    lsd = {}
    for layer in range(L):
        for name, (o, k) in {"self_attn.q": (256, 256), "self_attn.v": (256, 256), "ffn.0": (512, 256)}.items():
            lsd[f"blocks.{layer}.{name}.lora_A.weight"] = (0.05 * torch.randn(8, k, generator=g)).to(BF)
            lsd[f"blocks.{layer}.{name}.lora_B.weight"] = (0.05 * torch.randn(o, 8, generator=g)).to(BF)

    def model():
        m = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=TEXT_DIM, device=DEV)
        m.load_state_dict(sd)
        return m

    def tensors(m):
        out = dict(m._tensors)
        out.update({"mx." + k: v for k, v in m._mx_scales.items()})
        out.update({"row." + k: v for k, v in m._fp8_row_scales.items()})
        return out

    def state(m):
        torch.cuda.synchronize()
        return {k: v.clone().view(torch.uint8) if v.element_size() == 1 else v.clone() for k, v in tensors(m).items()}

    def same(a, b):
        return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)

    def addresses(m):
        return {k: v.data_ptr() for k, v in tensors(m).items()}

    fresh = model().set_linear_precision(MIXED)
    assert fresh._tensors["L0.qkv_w"].shape == (768, 192) and fresh._tensors["L1.qkv_w"].dtype == torch.float8_e4m3fn
    assert fresh._tensors["L1.ffn0_w"].shape == (512, 128) and fresh._tensors["head_w"].dtype == BF
    assert set(fresh._mx_scales) == {"L0.qkv_w", "L0.ffn0_w", "L0.ffn2_w", "L1.ffn0_w", "L1.ffn2_w"}
    assert len(fresh._fp8_row_scales) == 22 - 5 - 1
    m = model()
    m.load_lora(lsd, scale=0.0, name="style")
    m.set_linear_precision(MIXED)
    assert same(state(m), state(fresh))                                 # strength 0: the bases
    ptrs, table, modes, version = addresses(m), list(m._fp8_row_table), list(m._linear_modes), m._weights_version
    m.set_lora_scale("style", 1.0)
    merged = model()
    merged.load_lora(lsd, scale=1.0, name="style")
    merged.set_linear_precision(MIXED)
    assert same(state(m), state(merged)) and not same(state(m), state(fresh))
    for key in ("L0.qkv_w", "L1.qkv_w"):                                # MXFP6 codes / e4m3 codes: q rows moved, k rows did not
        a, b = m._tensors[key].view(torch.uint8), fresh._tensors[key].view(torch.uint8)
        assert not torch.equal(a[:256], b[:256]) and torch.equal(a[256:512], b[256:512])
    assert not torch.equal(m._tensors["L1.ffn0_w"], fresh._tensors["L1.ffn0_w"])
    assert addresses(m) == ptrs and list(m._fp8_row_table) == table and list(m._linear_modes) == modes
    assert m._weights_version != version and not m._graphs and m._cfg.use_fp8 == 7
    m.unload_lora()
    assert same(state(m), state(fresh)) and m._lora_base == {} and m.lora_adapters() == {}
    assert addresses(m) == ptrs
