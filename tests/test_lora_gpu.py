"""LoRA adapters on the GPU: rtv_lora_merge against the float64 oracle (tests/lora_oracle.py), and load / scale / unload on a
tiny CausalWanModel (dim 256, ffn 512, 2 heads, 2 layers) - weights, forwards, hipGraphs, the cross-attention cache, fp8, a session."""
import pytest
import torch

import lora_oracle as lo
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


# ------------------------------------------------------------------ kernel
def _merge(base, out, adapters):
    from realtime_video_amd import lora
    lora.merge(base, out, adapters)
    torch.cuda.synchronize()
    return out


def _dev(adapters):
    return [(A.to(DEV), B.to(DEV), s) for A, B, s in adapters]


@pytest.mark.parametrize("N, K, rank, scale", [(160, 136, 4, 1.0), (256, 256, 16, 0.7), (384, 200, 48, -0.5), (128, 512, 256, 0.25)])
def test_merge_matches_oracle(N, K, rank, scale):
    """A ragged N (160 = 2.5 row tiles), a ragged K (136, 200: no multiple of the 128-column tile), a rank padded to the MFMA step
    (4), a rank that is no power of two (48: a 48-wide LDS chunk), and the cap (256: four rank chunks)."""
    base, [(A, B)] = lo.make_inputs(N, K, [rank], seed=N + rank)
    ad = [(A, B, scale)]
    ref, mag = lo.merge_oracle(base, ad)
    W = _merge(base.to(DEV), torch.full((N, K), 7.0, dtype=BF, device=DEV), _dev(ad))
    lo.assert_meets(W, ref, mag, f"{N}x{K} rank {rank}")


def test_merge_two_adapters_at_once():
    base, [(A0, B0), (A1, B1)] = lo.make_inputs(256, 256, [16, 8], seed=3)
    ad = [(A0, B0, 0.7), (A1, B1, -1.3)]
    ref, mag = lo.merge_oracle(base, ad)
    W = _merge(base.to(DEV), torch.empty(256, 256, dtype=BF, device=DEV), _dev(ad))
    lo.assert_meets(W, ref, mag, "two adapters")


def test_merge_row_range_in_place_leaves_other_rows():
    """Rows [256, 512) of a 768 x 256 matrix (k inside a fused qkv), base == W; the other rows keep every bit."""
    full, [(A, B)] = lo.make_inputs(768, 256, [16], seed=4)
    B = B[:256].contiguous()
    ad = [(A, B, 0.7)]
    ref, mag = lo.merge_oracle(full[256:512], ad)
    W = full.to(DEV)
    ptr = W.data_ptr()
    _merge(W[256:512], W[256:512], _dev(ad))
    assert W.data_ptr() == ptr
    lo.assert_meets(W[256:512], ref, mag, "rows [256, 512) in place")
    assert torch.equal(W[:256].cpu().view(torch.int16), full[:256].view(torch.int16))
    assert torch.equal(W[512:].cpu().view(torch.int16), full[512:].view(torch.int16))


def test_merge_strided_views():
    """ldb / ldw above K: a column block of wider matrices; the columns outside it are not written."""
    base, [(A, B)] = lo.make_inputs(96, 64, [16], seed=5)
    wide_b = torch.zeros(96, 80, dtype=BF, device=DEV)
    wide_b[:, 8:72] = base.to(DEV)
    wide_w = torch.full((96, 96), 3.0, dtype=BF, device=DEV)
    ad = [(A, B, 0.7)]
    ref, mag = lo.merge_oracle(base, ad)
    _merge(wide_b[:, 8:72], wide_w[:, 16:80], _dev(ad))
    lo.assert_meets(wide_w[:, 16:80], ref, mag, "strided")
    assert bool((wide_w[:, :16] == 3.0).all()) and bool((wide_w[:, 80:] == 3.0).all())


@pytest.mark.parametrize("case", ["count0", "scale0"])
def test_merge_zero_is_bit_exact(case):
    base, [(A, B)] = lo.make_inputs(160, 136, [16], seed=6)
    base[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30]).to(BF)
    W = _merge(base.to(DEV), torch.full((160, 136), 7.0, dtype=BF, device=DEV), [] if case == "count0" else _dev([(A, B, 0.0)]))
    assert torch.equal(W.cpu().view(torch.int16), base.view(torch.int16))


# ------------------------------------------------------------------ model
CFG = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=2, freq_dim=256, text_len=512, eps=1e-6)
LINEARS = {"self_attn.q": ("qkv_w", 0), "self_attn.k": ("qkv_w", 1), "self_attn.v": ("qkv_w", 2), "self_attn.o": ("o_w", 0),
           "cross_attn.q": ("cq_w", 0), "cross_attn.k": ("ck_w", 0), "cross_attn.v": ("cv_w", 0), "cross_attn.o": ("co_w", 0),
           "ffn.0": ("ffn0_w", 0), "ffn.2": ("ffn2_w", 0)}
SCALE = 0.7


@pytest.fixture(scope="module")
def weights():
    from oracle import wan_oracle as wo
    return {64: wo.make_weights(CFG, seed=0, text_dim=64), 128: wo.make_weights(CFG, seed=0, text_dim=128)}


def _std_weights(w):
    """The oracle's weights with every LoRA-able Linear redrawn at 0.02 N(0,1), the scale the merge criterion is stated for."""
    g = torch.Generator().manual_seed(11)
    w = dict(w)
    for i in range(CFG["num_layers"]):
        for name in LINEARS:
            k = f"blocks.{i}.{name}.weight"
            w[k] = (lo.BASE_STD * torch.randn(w[k].shape, generator=g)).to(BF)
    return w


@pytest.fixture(scope="module")
def base_sd(weights):
    return {td: _std_weights(w) for td, w in weights.items()}


def _lora_sd(sd, names=tuple(LINEARS), rank=16, seed=21, layers=(0, 1)):
    """An adapter over `names` in every layer, both key styles, every prefix, alpha on the ffn (alpha 8 at rank 16: factor 0.5,
    with B drawn twice as large so that the delta keeps its size)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i in layers:
        for n, name in enumerate(names):
            o, k = sd[f"blocks.{i}.{name}.weight"].shape
            prefix = ("", "diffusion_model.", "model.diffusion_model.", "model.")[n % 4]
            a, b = ((".lora_A.weight", ".lora_B.weight"), (".lora_down.weight", ".lora_up.weight"))[n % 2]
            alpha = name.startswith("ffn")
            out[f"{prefix}blocks.{i}.{name}{a}"] = (lo.AB_STD * torch.randn(rank, k, generator=g)).to(BF)
            out[f"{prefix}blocks.{i}.{name}{b}"] = ((2 if alpha else 1) * lo.AB_STD * torch.randn(o, rank, generator=g)).to(BF)
            if alpha:
                out[f"{prefix}blocks.{i}.{name}.alpha"] = torch.tensor(rank / 2.0)
    return out


def _oracle_merge(sd, lora_sd, scale):
    """{Linear weight key: (ref, mag)} of the float64 merge, through the parser's own mapping of names only."""
    from realtime_video_amd.lora import _strip
    out = {}
    for key in lora_sd:
        name = _strip(key)
        for a, b in ((".lora_A.weight", ".lora_B.weight"), (".lora_down.weight", ".lora_up.weight")):
            if name.endswith(a):
                t = name[:-len(a)]
                pre = key[:len(key) - len(name)]
                A, B = lora_sd[key], lora_sd[pre + t + b]
                alpha = lora_sd.get(pre + t + ".alpha")
                f = scale * (float(alpha) / A.shape[0] if alpha is not None else 1.0)
                out[t + ".weight"] = lo.merge_oracle(sd[t + ".weight"], [(A, B, f)])
    return out


def _model(sd, text_dim=64, **kw):
    from realtime_video_amd.causal_model import CausalWanModel
    m = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=text_dim, device=DEV)
    m.load_state_dict(sd)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _linear(m, i, name):
    field, blk = LINEARS[name]
    t = m._tensors[f"L{i}.{field}"]
    return t[blk * 256:(blk + 1) * 256] if field == "qkv_w" else t


def _bits(m):
    return {k: v.clone().view(torch.uint8) for k, v in m._tensors.items()}


def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def _inputs(text_dim=64):
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(1, 16, 3, 30, 52, generator=g).to(BF).to(DEV)          # 3 latent frames of 30 x 52: 390 tokens per frame
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


def _merged_state_dict(sd, m):
    out = dict(sd)
    for i in range(2):
        for name in LINEARS:
            out[f"blocks.{i}.{name}.weight"] = _linear(m, i, name).clone()
    return out


def test_model_weights_meet_the_criterion_and_nothing_else_moves(base_sd):
    sd = base_sd[64]
    names = ("self_attn.q", "self_attn.v", "self_attn.o", "cross_attn.k", "ffn.0", "ffn.2")      # k, cross q / v / o untouched
    lsd = _lora_sd(sd, names)
    m = _model(sd)
    before, ptrs = _bits(m), {k: v.data_ptr() for k, v in m._tensors.items()}
    n_params = len(list(m.parameters()))
    name = m.load_lora(lsd, scale=SCALE)
    assert m.lora_adapters() == {name: SCALE} and len(list(m.parameters())) == n_params
    assert {k: v.data_ptr() for k, v in m._tensors.items()} == ptrs
    ora = _oracle_merge(sd, lsd, SCALE)
    assert len(ora) == 12
    for i in range(2):
        for lin in LINEARS:
            key = f"blocks.{i}.{lin}.weight"
            if lin in names:
                lo.assert_meets(_linear(m, i, lin), *ora[key], key)
            else:
                assert torch.equal(_linear(m, i, lin).cpu().view(torch.int16), sd[key].view(torch.int16)), key
    after = _bits(m)
    touched = {f"L{i}.{LINEARS[n][0]}" for i in range(2) for n in names}
    assert all(torch.equal(after[k], before[k]) for k in before if k not in touched)
    assert all(not torch.equal(after[k], before[k]) for k in touched)


def test_forward_equals_reloaded_and_premerged_models(base_sd):
    sd = base_sd[64]
    lsd = _lora_sd(sd)
    inputs = _inputs()
    m = _model(sd)
    y_base = _forward(m, inputs)
    m.load_lora(lsd, scale=SCALE, name="style")
    y = _forward(m, inputs)
    # nothing stale: a model loaded from the merged tensors computes the same bits
    y_reload = _forward(_model(_merged_state_dict(sd, m)), inputs)
    assert torch.equal(y, y_reload)
    # nothing missed or mis-scaled: against the float64-merged checkpoint, far below the adapter's own effect
    pre = dict(sd)
    for key, (ref, _) in _oracle_merge(sd, lsd, SCALE).items():
        pre[key] = ref.to(BF)
    y_pre = _forward(_model(pre), inputs)
    e_merge, e_lora = rel_l2(y, y_pre), rel_l2(y, y_base)
    print(f"rel_l2(lora, premerged) = {e_merge:.3e}, rel_l2(lora, base) = {e_lora:.3e}")
    assert e_lora > 0 and e_merge <= 0.1 * e_lora


def test_scale_changes_do_not_drift_and_unload_restores(base_sd):
    sd = base_sd[64]
    m = _model(sd)
    before, ptrs = _bits(m), {k: v.data_ptr() for k, v in m._tensors.items()}
    a = m.load_lora(_lora_sd(sd), scale=SCALE, name="a")
    first = _bits(m)
    for s in (0.1, -2.0, 0.0, 1.5, SCALE):
        m.set_lora_scale(a, s)
    torch.cuda.synchronize()
    assert m.lora_adapters() == {"a": SCALE} and _same_bits(_bits(m), first)
    # a second adapter over some matrices, then out again: back at the first merge
    b = m.load_lora(_lora_sd(sd, ("self_attn.k", "ffn.0"), rank=8, seed=5), scale=-1.3)
    assert not _same_bits(_bits(m), first) and list(m.lora_adapters()) == ["a", b]
    m.unload_lora(b)
    assert _same_bits(_bits(m), first)
    for i in range(3):
        m.load_lora(_lora_sd(sd, ("ffn.2",), rank=4, seed=30 + i, layers=(0,)), scale=0.0)
    with pytest.raises(RuntimeError, match="at most 4"):
        m.load_lora(_lora_sd(sd, ("ffn.2",), rank=4, seed=40, layers=(0,)))
    m.unload_lora()
    torch.cuda.synchronize()
    assert m.lora_adapters() == {} and m._lora_base == {}
    assert _same_bits(_bits(m), before) and {k: v.data_ptr() for k, v in m._tensors.items()} == ptrs
    # load_state_dict drops adapters
    m.load_lora(_lora_sd(sd), name="a")
    m.load_state_dict(sd)
    assert m.lora_adapters() == {} and m._lora_base == {} and _same_bits(_bits(m), before)


def test_captured_graphs_follow_a_scale_change(base_sd):
    sd = base_sd[64]
    lsd = _lora_sd(sd)
    inputs = _inputs()
    g = _model(sd, use_hip_graphs=True)
    g.load_lora(lsd, scale=SCALE, name="style")
    caches = _caches()
    for _ in range(4):                      # cross-attention fill, first sighting, capture, replay
        y0 = _forward(g, inputs, caches)
    graphs = dict(g._graphs)
    assert any(isinstance(e, dict) for e in graphs.values())
    g.set_lora_scale("style", -0.4)
    assert list(g._graphs) == list(graphs) and all(g._graphs[k] is graphs[k] for k in graphs)     # kept: the weights changed in place
    _forward(g, inputs, caches)             # (refills the text K / V eagerly: ck_w / cv_w changed)
    y1 = _forward(g, inputs, caches)        # replayed
    e = _model(sd)
    e.load_lora(lsd, scale=-0.4)
    ecaches = _caches()
    _forward(e, inputs, ecaches)
    y_eager = _forward(e, inputs, ecaches)
    assert torch.equal(y1, y_eager) and not torch.equal(y1, y0)


def test_cross_attention_cache_is_refilled_after_a_change(base_sd):
    sd = base_sd[64]
    inputs = _inputs()
    m = _model(sd)
    m.load_lora(_lora_sd(sd, ("cross_attn.k", "cross_attn.v")), scale=SCALE, name="x")
    caches = _caches()
    y0 = _forward(m, inputs, caches)
    v0 = m.lora_version
    assert all(c["is_init"] and c["lora_version"] == v0 for c in caches[1])
    m.set_lora_scale("x", 2.0)
    assert m.lora_version != v0
    y_reused = _forward(m, inputs, caches)
    y_fresh = _forward(m, inputs)
    assert torch.equal(y_reused, y_fresh) and not torch.equal(y_reused, y0)
    assert all(c["lora_version"] == m.lora_version for c in caches[1])


def test_fp8_requantises_from_the_bases(base_sd):
    sd = base_sd[128]
    lsd = _lora_sd(sd)
    inputs = _inputs(128)
    a = _model(sd, text_dim=128)
    a.load_lora(lsd, scale=SCALE, name="style")
    a.enable_fp8()
    b = _model(sd, text_dim=128)
    b.load_lora(lsd, scale=0.0, name="style")
    b.enable_fp8()
    ptrs, version = {k: v.data_ptr() for k, v in b._tensors.items()}, b._weights_version
    yb0 = _forward(b, inputs)
    b.set_lora_scale("style", SCALE)
    assert {k: v.data_ptr() for k, v in b._tensors.items()} == ptrs and b._weights_version != version and not b._graphs
    assert _same_bits(_bits(a), _bits(b))
    assert list(a._fp8_scales) == list(b._fp8_scales)
    ya, yb = _forward(a, inputs), _forward(b, inputs)
    assert torch.equal(ya, yb) and not torch.equal(yb, yb0)
    c = _model(sd, text_dim=128)
    c.enable_fp8()
    with pytest.raises(RuntimeError, match="load adapters first"):
        c.load_lora(lsd)
    # unloading under fp8 goes back to the quantisation of the bases
    b.unload_lora()
    assert _same_bits(_bits(b), _bits(c)) and list(b._fp8_scales) == list(c._fp8_scales) and b._lora_base == {}


def test_session_set_lora_scale_between_blocks(base_sd):
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
    sd = base_sd[64]
    lsd = _lora_sd(sd)
    g = torch.Generator().manual_seed(5)
    ctx = torch.randn(64, 64, generator=g).to(BF)
    noise = torch.randn(1, 6, 16, 60, 104, generator=g).to(BF)
    padded = torch.zeros(1, 512, 64, dtype=BF)
    padded[0, :64] = ctx

    def session():
        m = _model(sd)
        wr = WanDiffusionWrapper(m, timestep_shift=5.0)
        assert wr.load_lora(lsd, scale=0.2, name="style") == "style" and wr.lora_adapters() == {"style": 0.2}
        pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 500]), DEV, generator=wr,
                                       text_encoder=None, vae=None)
        sess = GenerationSession(GenerateParams(seed=9, num_blocks=2, num_denoising_steps=2, keep_first_frame=True),
                                 Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(padded.to(DEV))), device=DEV)
        sess.noise = noise.to(DEV)
        rnd = torch.Generator().manual_seed(9)
        sess._randn = lambda shape: torch.randn(*shape, generator=rnd, dtype=BF).to(DEV)
        return sess, m

    blocks = {}
    for how in ("session", "by hand", "unchanged"):
        sess, m = session()
        b0 = sess.generate_block().clone()
        if how == "session":
            sess.set_lora_scale("style", 1.0)
        elif how == "by hand":
            m.set_lora_scale("style", 1.0)
        blocks[how] = (b0, sess.generate_block().clone())
    assert torch.equal(blocks["session"][0], blocks["unchanged"][0])
    assert torch.equal(blocks["session"][1], blocks["by hand"][1])
    assert not torch.equal(blocks["session"][1], blocks["unchanged"][1])
