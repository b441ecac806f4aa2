"""The extended LoRA merges on the GPU: rtv_lora_merge_ex and rtv_lora_merge_dora against the float64 oracles
(tests/lora_ext_oracle.py), and extended adapters - every key style, every kind of target, DoRA - loaded, scaled and unloaded on the
tiny CausalWanModel of test_lora_gpu.py (dim 256, ffn 512, 2 heads, 2 layers)."""
import pytest
import torch

import lora_ext_oracle as xo
import lora_oracle as lo
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _dev(x):
    return None if x is None else x.to(DEV)


# ------------------------------------------------------------------ kernel: merge_ex
def _ex(base, out, terms):
    from realtime_video_amd import lora
    lora.merge_ex(base, out, [(_dev(A), _dev(B), s, _dev(d), ds) for A, B, s, d, ds in terms])
    torch.cuda.synchronize()
    return out


def test_merge_ex_rank4_and_diff_on_ragged_tiles():
    """72 x 136: a partial row tile, a partial K tile, rank 4 (the scalar B path, padded to the MFMA step)."""
    base, [(A, B)], _, diff = xo.make_inputs(72, 136, [4], seed=76)
    terms = [(A, B, 0.7, diff, -1.3)]
    ref, mag = xo.merge_ex_oracle(base, terms)
    W = _ex(base.to(DEV), torch.full((72, 136), 7.0, dtype=BF, device=DEV), terms)
    lo.assert_meets(W, ref, mag, "merge_ex 72x136 r4 + diff")


def test_merge_ex_three_terms_two_rank_chunks():
    """160 x 392 with ranks 80 (two rank chunks) + 16 as two terms and a diff-only third."""
    base, [(A0, B0), (A1, B1)], _, diff = xo.make_inputs(160, 392, [80, 16], seed=240)
    terms = [(A0, B0, 0.7, None, 0.0), (A1, B1, -0.4, None, 0.0), (None, None, 0.0, diff, 0.9)]
    ref, mag = xo.merge_ex_oracle(base, terms)
    W = _ex(base.to(DEV), torch.empty(160, 392, dtype=BF, device=DEV), terms)
    lo.assert_meets(W, ref, mag, "merge_ex 160x392 r80 + r16 + diff")


def test_merge_ex_vector():
    """N = 1, K = 256, diff only: how a bias or a norm weight is merged."""
    base, _, _, diff = xo.make_inputs(1, 256, [], seed=5)
    terms = [(None, None, 0.0, diff, 0.7)]
    ref, mag = xo.merge_ex_oracle(base, terms)
    W = _ex(base.to(DEV), torch.full((1, 256), 7.0, dtype=BF, device=DEV), terms)
    lo.assert_meets(W, ref, mag, "merge_ex vector")
    assert not torch.equal(_bits(W), _bits(base))


def test_merge_ex_row_range_in_place_leaves_other_rows():
    """Rows [256, 512) of a 768 x 256 matrix (k inside a fused qkv), base == W, the diff a row range too; the other rows keep every bit."""
    from realtime_video_amd import lora
    full, [(A, B)], _, diff = xo.make_inputs(768, 256, [16], seed=4)
    B = B[256:512].contiguous()
    ref, mag = xo.merge_ex_oracle(full[256:512], [(A, B, 0.7, diff[256:512], 0.5)])
    W, d = full.to(DEV), diff.to(DEV)
    lora.merge_ex(W[256:512], W[256:512], [(A.to(DEV), B.to(DEV), 0.7, d[256:512], 0.5)])
    torch.cuda.synchronize()
    lo.assert_meets(W[256:512], ref, mag, "merge_ex rows [256, 512) in place")
    assert torch.equal(_bits(W[:256]), _bits(full[:256])) and torch.equal(_bits(W[512:]), _bits(full[512:]))


def test_merge_ex_strided_views():
    """ldb / ldw / ldd above K: column blocks of wider matrices; the columns outside are not written."""
    base, [(A, B)], _, diff = xo.make_inputs(96, 64, [16], seed=5)
    wide_b = torch.zeros(96, 80, dtype=BF, device=DEV)
    wide_b[:, 8:72] = base.to(DEV)
    wide_d = torch.zeros(96, 72, dtype=BF, device=DEV)
    wide_d[:, 8:72] = diff.to(DEV)
    wide_w = torch.full((96, 96), 3.0, dtype=BF, device=DEV)
    ref, mag = xo.merge_ex_oracle(base, [(A, B, 0.7, diff, -0.6)])
    from realtime_video_amd import lora
    lora.merge_ex(wide_b[:, 8:72], wide_w[:, 16:80], [(A.to(DEV), B.to(DEV), 0.7, wide_d[:, 8:72], -0.6)])
    torch.cuda.synchronize()
    lo.assert_meets(wide_w[:, 16:80], ref, mag, "merge_ex strided")
    assert bool((wide_w[:, :16] == 3.0).all()) and bool((wide_w[:, 80:] == 3.0).all())


@pytest.mark.parametrize("case", ["count0", "scales0", "cancel"])
def test_merge_ex_zero_total_keeps_the_bits(case):
    base, [(A, B)], _, diff = xo.make_inputs(160, 136, [16], seed=6)
    base[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30]).to(BF)
    terms = {"count0": [], "scales0": [(A, B, 0.0, diff, 0.0)],
             "cancel": [(None, None, 0.0, diff, 0.5), (None, None, 0.0, diff, -0.5)]}[case]
    W = _ex(base.to(DEV), torch.full((160, 136), 7.0, dtype=BF, device=DEV), terms)
    assert torch.equal(_bits(W), _bits(base))


@pytest.mark.parametrize("N, K, ranks", [(72, 136, [4]), (160, 392, [80, 16]), (128, 512, [256, 8, 24, 64])])
def test_merge_ex_low_rank_only_equals_merge_bit_for_bit(N, K, ranks):
    from realtime_video_amd import lora
    base, ab, _, _ = xo.make_inputs(N, K, ranks, seed=N + K)
    scales = [0.7, -1.3, 0.25, 1.0][:len(ranks)]
    ads = [(A.to(DEV), B.to(DEV), s) for (A, B), s in zip(ab, scales)]
    old = lora.merge(base.to(DEV), torch.empty(N, K, dtype=BF, device=DEV), ads)
    new = lora.merge_ex(base.to(DEV), torch.empty(N, K, dtype=BF, device=DEV), [(A, B, s, None, 0.0) for A, B, s in ads])
    torch.cuda.synchronize()
    assert torch.equal(_bits(old), _bits(new)) and not torch.equal(_bits(new), _bits(base))


# ------------------------------------------------------------------ kernel: merge_dora
def _dora(base, out, A, B, factor, mag, strength, ws=None):
    from realtime_video_amd import lora
    N, K = base.shape
    if ws is None:
        ws = torch.empty(lora.dora_workspace_bytes(N, K), dtype=torch.uint8, device=DEV)
    lora.merge_dora(base, out, A.to(DEV), B.to(DEV), factor, mag.to(DEV), strength, ws)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("N, K, rank, strength", [(72, 136, 4, 1.0), (160, 392, 80, 0.7), (64, 13824, 16, 1.0)])
def test_dora_matches_oracle(N, K, rank, strength):
    """A ragged tile with the scalar B path, two rank chunks with a partial blend, and the widest K of the 14B model (108 partials
    per row)."""
    base, [(A, B)], mag, _ = xo.make_inputs(N, K, [rank], seed=N + rank)
    factor = 8.0 / rank
    ref, bound_mag = xo.dora_oracle(base, A, B, factor, mag, strength)
    W = _dora(base.to(DEV), torch.full((N, K), 7.0, dtype=BF, device=DEV), A, B, factor, mag, strength)
    lo.assert_meets(W, ref, bound_mag, f"dora {N}x{K} r{rank}")
    # two calls, and in place against out of place: the same bits
    again = _dora(base.to(DEV), torch.empty(N, K, dtype=BF, device=DEV), A, B, factor, mag, strength)
    inplace = base.to(DEV)
    _dora(inplace, inplace, A, B, factor, mag, strength)
    assert torch.equal(_bits(W), _bits(again)) and torch.equal(_bits(W), _bits(inplace))


def test_dora_strength_zero_and_zero_rows_keep_the_bits():
    base, [(A, B)], mag, _ = xo.make_inputs(72, 136, [8], seed=9)
    base[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30]).to(BF)
    W = _dora(base.to(DEV), torch.full((72, 136), 7.0, dtype=BF, device=DEV), A, B, 1.0, mag, 0.0)
    assert torch.equal(_bits(W), _bits(base))
    base[5] = 0
    base[5, 3] = -0.0
    base[70] = 0
    B[5] = 0
    B[70] = 0
    W = _dora(base.to(DEV), torch.full((72, 136), 7.0, dtype=BF, device=DEV), A, B, 1.0, mag, 1.0)
    assert torch.equal(_bits(W[5]), _bits(base[5])) and torch.equal(_bits(W[70]), _bits(base[70]))
    ref, bound_mag = xo.dora_oracle(base, A, B, 1.0, mag, 1.0)
    lo.assert_meets(W, ref, bound_mag, "dora with zero rows")


def test_dora_one_hot_rows_are_exact():
    """Each row of V has a single non-zero element: nrm = |v| exactly, so the result is bf16(mag * sign(v)) in that column and the
    zeros of base elsewhere.  Exact equality."""
    N, K, rank = 72, 392, 8
    g = torch.Generator().manual_seed(12)
    col = torch.randint(0, K, (rank,), generator=g)
    A = torch.zeros(rank, K)
    A[torch.arange(rank), col] = torch.randn(rank, generator=g)
    j = torch.arange(N) % rank
    B = torch.zeros(N, rank)
    B[torch.arange(N), j] = torch.randn(N, generator=g)
    base = torch.zeros(N, K)
    base[torch.arange(N)[::2], col[j][::2]] = 0.05 * torch.randn(N, generator=g)[::2]      # every other row: base in the same column
    base[1, 0 if int(col[j[1]]) else 1] = -0.0
    A, B, base = A.to(BF), B.to(BF), base.to(BF)
    mag = (torch.rand(N, generator=g) + 0.5).to(BF)
    V = base.double() + 0.5 * (B.double() @ A.double())
    assert bool(((V != 0).sum(dim=1) == 1).all())
    want = torch.zeros(N, K, dtype=torch.float64)
    want[torch.arange(N), col[j]] = mag.double() * V[torch.arange(N), col[j]].sign()
    W = _dora(base.to(DEV), torch.full((N, K), 7.0, dtype=BF, device=DEV), A, B, 0.5, mag, 1.0)
    assert torch.equal(W.cpu().double(), want)
    assert _bits(W)[1, 0 if int(col[j[1]]) else 1] == _bits(base)[1, 0 if int(col[j[1]]) else 1]      # -0 stays -0


# ------------------------------------------------------------------ model
CFG = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=2, freq_dim=256, text_len=512, eps=1e-6)
SCALE = 0.7


@pytest.fixture(scope="module")
def base_sd():
    """The oracle's weights with every Linear redrawn at 0.02 N(0,1), the scale the merge criterion is stated for."""
    from oracle import wan_oracle as wo
    out = {}
    for td in (64, 128):
        w = dict(wo.make_weights(CFG, seed=0, text_dim=td))
        g = torch.Generator().manual_seed(11)
        linears, _ = xo.all_targets()
        for t in linears:
            w[t + ".weight"] = (lo.BASE_STD * torch.randn(w[t + ".weight"].shape, generator=g)).to(BF)
        out[td] = w
    return out


def _model(sd, text_dim=64):
    from realtime_video_amd.causal_model import CausalWanModel
    m = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=text_dim, device=DEV)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def adapters(base_sd):
    out = {}
    for td, sd in base_sd.items():
        m = _model(sd, td)
        out[td] = xo.full_adapter(m.state_dict_shapes(), base=sd)
    return out


def _all_bits(m):
    return {k: v.clone().view(torch.uint8) for k, v in m._tensors.items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def _locate(m, key):
    """The model's view of the state-dict tensor `key`, through lora.extended_targets' mapping of names."""
    from realtime_video_amd.lora import extended_targets
    target, part = key.rsplit(".", 1)
    _, tensor, row0, rows, cols, bias, bias0, bias_n = extended_targets(m.state_dict_shapes())[target]
    if part == "bias":
        return bias, m._tensors[bias][bias0:bias0 + bias_n]
    t = m._tensors[tensor]
    return tensor, (t if t.ndim == 1 else t[row0:row0 + rows])


def _inputs(text_dim=64):
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(1, 16, 3, 30, 52, generator=g).to(BF).to(DEV)
    ctx = torch.randn(32, text_dim, generator=g).to(BF).to(DEV)
    return lat, ctx, torch.tensor([[500.0, 500.0, 500.0]], device=DEV)


def _caches():
    kv = [{"k": torch.zeros(1, 1170, 2, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 1170, 2, 128, dtype=BF, device=DEV),
           "global_end_index": 0, "local_end_index": 0} for _ in range(2)]
    ca = [{"k": torch.zeros(1, 512, 2, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, 2, 128, dtype=BF, device=DEV),
           "is_init": False} for _ in range(2)]
    return kv, ca


def _forward(m, inputs, caches=None):
    lat, ctx, t = inputs
    kv, ca = caches or _caches()
    out = m(lat, t=t, context=[ctx], kv_cache=kv, crossattn_cache=ca, current_start=0)
    torch.cuda.synchronize()
    return out.clone()


def test_model_every_tensor_meets_the_criterion_and_nothing_else_moves(base_sd, adapters):
    sd, ad = base_sd[64], adapters[64]
    m = _model(sd)
    before, ptrs = _all_bits(m), {k: v.data_ptr() for k, v in m._tensors.items()}
    n_params = len(list(m.parameters()))
    name = m.load_lora(xo.spell(ad, "kohya"), scale=SCALE, extended=True)
    assert m.lora_adapters() == {name: SCALE} and len(list(m.parameters())) == n_params
    assert {k: v.data_ptr() for k, v in m._tensors.items()} == ptrs
    ora = xo.merged_state_dict(sd, ad, SCALE)
    linears, norms = xo.all_targets()
    assert len(ora) == 2 * len(linears) + len(norms) + 2          # every Linear's weight and bias, every norm weight, norm3's biases
    touched = set()
    for key, (ref, mag) in ora.items():
        tensor, view = _locate(m, key)
        touched.add(tensor)
        lo.assert_meets(view, ref, mag, key)
        assert not torch.equal(view.cpu(), sd[key].to(BF)), key
    after = _all_bits(m)
    assert set(m._lora_base) == touched
    assert all(torch.equal(after[k], before[k]) for k in before if k not in touched)
    assert {"patch_w", "patch_b", "modulation", "head_modulation", "rope_cs"} <= set(before) - touched


def test_forward_equals_premerged_model(base_sd, adapters):
    sd, ad = base_sd[64], adapters[64]
    inputs = _inputs()
    m = _model(sd)
    y_base = _forward(m, inputs)
    m.load_lora(xo.spell(ad, "diffusers", "transformer."), scale=SCALE, name="style", extended=True)
    y = _forward(m, inputs)
    pre = dict(sd)
    for key, (ref, _) in xo.merged_state_dict(sd, ad, SCALE).items():
        pre[key] = ref.to(BF)
    y_pre = _forward(_model(pre), inputs)
    e_merge, e_lora = rel_l2(y, y_pre), rel_l2(y, y_base)
    print(f"rel_l2(extended lora, premerged) = {e_merge:.3e}, rel_l2(lora, base) = {e_lora:.3e}")
    assert e_lora > 0 and e_merge <= 0.1 * e_lora


def test_three_key_styles_give_identical_weights(base_sd, adapters):
    sd, ad = base_sd[64], adapters[64]
    bits = []
    for style, prefix in (("canonical", "diffusion_model."), ("diffusers", "transformer."), ("kohya", "")):
        m = _model(sd)
        m.load_lora(xo.spell(ad, style, prefix, column=style == "kohya"), scale=SCALE, extended=True)
        torch.cuda.synchronize()
        bits.append(_all_bits(m))
    assert _same(bits[0], bits[1]) and _same(bits[0], bits[2])
    assert not _same(bits[0], _all_bits(_model(sd)))


def test_scale_round_trip_and_unload_restore_every_bit(base_sd, adapters):
    sd, ad = base_sd[64], adapters[64]
    m = _model(sd)
    before, ptrs = _all_bits(m), {k: v.data_ptr() for k, v in m._tensors.items()}
    a = m.load_lora(xo.spell(ad, "canonical"), scale=SCALE, name="a", extended=True)
    first = _all_bits(m)
    for s in (0.1, -2.0, 0.0, SCALE):
        m.set_lora_scale(a, s)
        if s == 0.0:
            torch.cuda.synchronize()
            assert _same(_all_bits(m), before)          # strength 0: the bits of the bases, DoRA ranges included
    torch.cuda.synchronize()
    assert _same(_all_bits(m), first)
    # a plain adapter of the default dialect over ranges without DoRA, then out again
    plain = {"blocks.0.self_attn.q.lora_A.weight": torch.randn(8, 256).to(BF), "blocks.0.self_attn.q.lora_B.weight": torch.randn(256, 8).to(BF)}
    b = m.load_lora(plain, scale=0.01)
    assert not _same(_all_bits(m), first)
    m.unload_lora(b)
    assert _same(_all_bits(m), first)
    m.unload_lora()
    torch.cuda.synchronize()
    assert m.lora_adapters() == {} and m._lora_base == {}
    assert _same(_all_bits(m), before) and {k: v.data_ptr() for k, v in m._tensors.items()} == ptrs


@pytest.mark.parametrize("key", ["blocks.0.cross_attn.k.diff_b", "blocks.1.cross_attn.v.diff_b", "blocks.0.cross_attn.norm_k.diff"])
def test_cross_attention_cache_is_refilled_after_a_vector_change(base_sd, key):
    sd = base_sd[64]
    inputs = _inputs()
    m = _model(sd)
    caches = _caches()
    y0 = _forward(m, inputs, caches)
    v0 = m.lora_version
    m.load_lora({key: (0.2 * torch.randn(256, generator=torch.Generator().manual_seed(3))).to(BF)}, scale=1.0, name="x", extended=True)
    assert m.lora_version != v0
    y_reused = _forward(m, inputs, caches)
    y_fresh = _forward(m, inputs)
    assert torch.equal(y_reused, y_fresh) and not torch.equal(y_reused, y0)
    assert all(c["lora_version"] == m.lora_version for c in caches[1])
    v1 = m.lora_version
    m.load_lora({"blocks.0.self_attn.norm_k.diff": torch.ones(256).to(BF)}, name="y", extended=True)      # not a cross-attention tensor
    assert m.lora_version == v1


@pytest.mark.parametrize("first", ["dora", "plain"])
def test_dora_and_additive_adapters_exclude_each_other(base_sd, first):
    sd = base_sd[64]
    g = torch.Generator().manual_seed(8)
    pair = {"blocks.0.self_attn.k.lora_A.weight": (0.05 * torch.randn(4, 256, generator=g)).to(BF),
            "blocks.0.self_attn.k.lora_B.weight": (0.05 * torch.randn(256, 4, generator=g)).to(BF)}
    dora = {**pair, "blocks.0.self_attn.k.dora_scale": torch.full((256,), 0.3).to(BF)}
    other = {"lora_unet_blocks_0_self_attn_k.diff": (0.01 * torch.randn(256, 256, generator=g)).to(BF)}
    m = _model(sd)
    m.load_lora(dora if first == "dora" else other, scale=SCALE, name="one", extended=True)
    torch.cuda.synchronize()
    bits, version = _all_bits(m), m.lora_version
    with pytest.raises(ValueError) as e:
        m.load_lora(other if first == "dora" else dora, scale=SCALE, name="two", extended=True)
    assert all(w in str(e.value) for w in ("'one'", "'two'", "blocks.0.self_attn.k", "DoRA"))
    torch.cuda.synchronize()
    assert _same(_all_bits(m), bits) and list(m.lora_adapters()) == ["one"] and m.lora_version == version
    # q of the same layer is another range: the other kind lives there beside this one
    onto_q = {k.replace("_k.", "_q.").replace(".k.", ".q."): v for k, v in (other if first == "dora" else dora).items()}
    m.load_lora(onto_q, scale=SCALE, name="three", extended=True)
    assert list(m.lora_adapters()) == ["one", "three"]


def test_fp8_rows_requantises_from_the_bases(base_sd, adapters):
    sd, ad = base_sd[128], adapters[128]
    lsd = xo.spell(ad, "canonical")
    a = _model(sd, 128)
    a.load_lora(lsd, scale=SCALE, name="style", extended=True)
    a.enable_fp8("row")
    b = _model(sd, 128)
    b.load_lora(lsd, scale=0.0, name="style", extended=True)
    b.enable_fp8("row")
    ptrs, version = {k: v.data_ptr() for k, v in b._tensors.items()}, b._weights_version
    assert not _same(_all_bits(a), _all_bits(b))
    b.set_lora_scale("style", SCALE)
    torch.cuda.synchronize()
    assert {k: v.data_ptr() for k, v in b._tensors.items()} == ptrs and b._weights_version != version
    assert _same(_all_bits(a), _all_bits(b))
    assert all(torch.equal(a._fp8_row_scales[k], b._fp8_row_scales[k]) for k in a._fp8_row_scales)
    assert b._tensors["L0.qkv_w"].dtype == torch.float8_e4m3fn and b._tensors["L0.qkv_b"].dtype == BF      # quantised / kept in bf16
    c = _model(sd, 128)
    c.enable_fp8("row")
    with pytest.raises(RuntimeError, match="load adapters first"):
        c.load_lora(lsd, extended=True)
    b.unload_lora()
    torch.cuda.synchronize()
    assert _same(_all_bits(b), _all_bits(c)) and b._lora_base == {}
    assert all(torch.equal(b._fp8_row_scales[k], c._fp8_row_scales[k]) for k in c._fp8_row_scales)
