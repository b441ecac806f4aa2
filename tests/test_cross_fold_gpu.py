"""The text cross-attention with V folded into the output projection (rtv_dit_step.ca_vo_ld): the probabilities kernel, the folded
weight, the branch built from them, the decisions that switch it on and off, and the tiny model with it on against off.
Inputs, the fp64 definition and the bound of the probabilities: tests/cross_fold_cases.py."""
import math

import pytest
import torch

import cross_fold_cases as cf
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ the probabilities kernel
@pytest.mark.parametrize("keys", cf.KEYS)
@pytest.mark.parametrize("H", cf.HEADS)
@pytest.mark.parametrize("family", cf.FAMILIES)
def test_probabilities_match_the_fp64_softmax(family, H, keys):
    """rtv_attn_probs_dup against the fp64 softmax of the same bf16 q / k with + log(count) on the counted key, for every Lq and
    count of cross_fold_cases: |P - P_ref| <= C_BOUND u P_ref + TINY per element, the padding columns (keys .. kh of every head
    and the tail up to the row's width) exactly zero although the buffer held NaN, every row sums to 1 within keys * u."""
    from realtime_video_amd import ops
    kh = cf.round_up(keys, 8)
    cols = cf.round_up(H * kh, 64)
    for Lq in cf.LQ:
        for count in cf.COUNTS:
            q, k, dup = cf.probs_inputs(family, Lq, H, keys, count)
            q, k = q.to(DEV), k.to(DEV)
            ref = cf.probs_ref64(q, k, dup, count)
            buf = torch.full((Lq + 1, cols + 8), math.nan, dtype=torch.bfloat16, device=DEV)       # a wider row stride, a guard row
            p = ops.attn_probs_dup(q, k, dup, count, kh, cols, out=buf[:Lq, :cols])
            heads = p[:, :H * kh].view(Lq, H, kh)
            ratio = cf.probs_ratio(heads[..., :keys], ref)
            print(f"{family} H{H} keys{keys} Lq{Lq} count{count}: ratio {ratio:.3f}")
            assert ratio <= cf.C_BOUND, (Lq, count, ratio)
            assert bool((heads[..., keys:] == 0).all()) and bool((p[:, H * kh:] == 0).all()), (Lq, count)
            assert bool(torch.isnan(buf[:Lq, cols:]).all()) and bool(torch.isnan(buf[Lq]).all()), (Lq, count)   # nothing written outside
            assert float((heads.double().sum(-1) - 1).abs().max()) <= keys * cf.U, (Lq, count)


def test_probabilities_refuse_what_the_kernel_cannot_hold():
    from realtime_video_amd import ops
    q = torch.zeros(4, 2, 128, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros(129, 2, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ops.attn_probs_dup(q, k, 0, 1, 136, 320)                  # more than 128 keys
    with pytest.raises(RuntimeError):
        ops.attn_probs_dup(q, k[:9], 0, 1, 12, 64)                # kh not a multiple of 8
    with pytest.raises(RuntimeError):
        ops.attn_probs_dup(q, k[:9], 0, 1, 16, 24)                # the heads do not fit the row
    with pytest.raises(RuntimeError):
        ops.attn_probs_dup(q, k[:9], 9, 2, 16, 64)                # the counted key outside the window


# ------------------------------------------------------------------------------------------------ the folded weight
@pytest.mark.parametrize("text_rows", [1, 7, 64])
@pytest.mark.parametrize("H", [2, 3])
def test_folded_weight_matches_torch(H, text_rows):
    """rtv_cross_fold_weight against torch fp32 co_w_h @ v_h^T rounded to bf16: within one bf16 ulp on every real column (fp32 sums
    in another order may round the other way), exact zeros in every other column although the buffer held NaN.
    One bf16 ulp OF THE ELEMENT alone cannot be met by any fp32 sum in another order than torch's where the 128 products cancel:
    the reference's own fp32 sum is then uncertain by more than that ulp (first run: 5 of the 6 cases passed, [3-64] missed on
    such elements).  So the bound is one ulp plus the reference's own uncertainty, twice the textbook bound of an fp32 dot product
    of 128 terms, 2 * 128 * 2^-24 * sum |w| |v| (one for each of the two orders) - 0.4 % of an ulp where nothing cancels."""
    from realtime_video_amd import ops
    d = 128 * H
    g = torch.Generator().manual_seed(10 * H + text_rows)
    co_w = (torch.randn(d, d, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    v = torch.randn(80, d, generator=g).to(torch.bfloat16).to(DEV)
    ok, kh, kf = ops.cross_fold_dims(H, text_rows)
    assert ok and (kh, kf) == cf.fold_dims(H, text_rows)
    buf = torch.full((d, kf + 8), math.nan, dtype=torch.bfloat16, device=DEV)
    vo = ops.cross_fold_weight(co_w, v, text_rows + 1, kh, kf, out=buf[:, :kf])
    assert bool(torch.isnan(buf[:, kf:]).all())
    rows = text_rows + 1
    real = torch.zeros(kf, dtype=torch.bool, device=DEV)
    for h in range(H):
        wh, vh = co_w[:, h * 128:(h + 1) * 128].float(), v[:rows, h * 128:(h + 1) * 128].float()
        ref = wh @ vh.T
        got = vo[:, h * kh:h * kh + rows].float()
        ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)      # bf16: 8 significant bits
        floor = 2 * 128 * 2.0 ** -24 * (wh.abs() @ vh.abs().T)
        err = (got - ref.to(torch.bfloat16).float()).abs()
        print(f"H{H} text_rows{text_rows} head {h}: largest error {float((err / ulp).max()):.2f} ulp, "
              f"{int((err > ulp).sum())} of {err.numel()} elements beyond one ulp")
        assert bool((err <= ulp + floor).all()), h
        real[h * kh:h * kh + rows] = True
    assert bool((vo[:, ~real] == 0).all())


# ------------------------------------------------------------------------------------------------ the branch
@pytest.mark.parametrize("text_rows", [5, 64])
def test_cross_attention_branch_folded_against_today_and_fp64(text_rows):
    """q -> probabilities -> folded GEMM (+ bias + residual) against today's branch (rtv_attn_fwd_dup -> GEMM with co_w) and an fp64
    gold from the same bf16 inputs; errors on the branch's contribution out - x.  e_fold <= 2 e_today + 2e-3 (rel-L2 against
    gold): the form tests/test_depth_gpu.py uses for ours against the oracle."""
    from realtime_video_amd import ops
    M, H, d, text_len = 300, 2, 256, 512
    g = torch.Generator().manual_seed(text_rows)
    bf = lambda t: t.to(torch.bfloat16).to(DEV)
    q, x = bf(torch.randn(M, H, 128, generator=g)), bf(torch.randn(M, d, generator=g))
    k, v = bf(torch.randn(text_rows + 1, H, 128, generator=g)), bf(torch.randn(text_rows + 1, H, 128, generator=g))
    co_w, co_b = bf(torch.randn(d, d, generator=g) * 0.05), bf(torch.randn(d, generator=g) * 0.1)
    count = text_len - text_rows
    ok, kh, kf = ops.cross_fold_dims(H, text_rows)
    assert ok
    p64 = cf.probs_ref64(q, k, text_rows, count)
    gold = torch.einsum("qhk,khd->qhd", p64, v.double()).reshape(M, d) @ co_w.double().T + co_b.double()
    ao = ops.attn_fwd_dup(q[None], k[None], v[None], text_rows, count)[0].reshape(M, d)
    today = ops.gemm(ao, co_w, bias=co_b, residual=x)
    vo = ops.cross_fold_weight(co_w, v.view(text_rows + 1, d), text_rows + 1, kh, kf)
    fold = ops.gemm(ops.attn_probs_dup(q, k, text_rows, count, kh, kf), vo, bias=co_b, residual=x)
    e_today, e_fold = rel_l2(today.double() - x.double(), gold), rel_l2(fold.double() - x.double(), gold)
    print(f"text_rows {text_rows}: branch rel-L2 against fp64 gold: today {e_today:.3e}, folded {e_fold:.3e}")
    assert e_fold <= 2 * e_today + 2e-3, (e_today, e_fold)


# ------------------------------------------------------------------------------------------------ decisions, model level
def _tiny(heads=2):
    from oracle.make_golden import TEXT_DIM, TINY, tiny_inputs
    cfg = dict(TINY)
    cfg.update(num_heads=heads, dim=128 * heads)
    return cfg, TEXT_DIM, tiny_inputs


def _build(cfg, text_dim, weights):
    from realtime_video_amd.causal_model import CausalWanModel
    from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
    m = CausalWanModel(dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"],
                       text_dim=text_dim, freq_dim=cfg.get("freq_dim", 256))
    m.load_state_dict(weights)
    return m, WanDiffusionWrapper(m, timestep_shift=5.0)


def _caches(cfg, kv_size=9360):
    L, H = cfg["num_layers"], cfg["num_heads"]
    z = lambda rows: torch.zeros(1, rows, H, 128, dtype=torch.bfloat16, device=DEV)
    kv = [{"k": z(kv_size), "v": z(kv_size), "global_end_index": 0, "local_end_index": 0} for _ in range(L)]
    ca = [{"k": z(512), "v": z(512), "is_init": False} for _ in range(L)]
    return kv, ca


@pytest.fixture(scope="module")
def tiny():
    """The tiny model's weights and inputs, and one forward pair per (prompt rows, setup) shared by the tests below."""
    from oracle import wan_oracle as wo
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    g = torch.Generator().manual_seed(3)
    long_ctx = torch.randn(200, text_dim, generator=g).to(torch.bfloat16)
    t = torch.ones([1, 3], dtype=torch.int64, device=DEV) * 700
    memo = {}

    def run(ctx_rows=64, fold=True, setup=None, tile_cfg=0):
        """Two forwards (cache fill + a second block) -> (flow 0, flow 1, model, caches); `setup(model)` runs before them."""
        key = (ctx_rows, fold, tile_cfg) if setup is None else None
        if key in memo:
            return memo[key]
        model, wr = _build(cfg, text_dim, w)
        model.fold_cross_v = fold
        model.gemm_tile_cfg = tile_cfg
        if setup is not None:
            setup(model)
        c = (ctx if ctx_rows == 64 else long_ctx[:ctx_rows]).to(DEV)
        kv, ca = _caches(cfg)
        cond = {"prompt_embeds": [c]}
        a, _ = wr(lat[0].to(DEV), cond, t, kv, ca, current_start=0)
        b, _ = wr(lat[3].to(DEV), cond, t, kv, ca, current_start=4680)
        res = (a.clone(), b.clone(), model, (kv, ca, wr, cond))
        if key is not None:
            memo[key] = res
        return res

    return dict(cfg=cfg, text_dim=text_dim, w=w, lat=lat, ctx=ctx, t=t, run=run)


def _folded(ca):
    return all(c.get("vo_for") is not None for c in ca)


def test_model_fold_on_against_off(tiny):
    """The tiny model (2 layers), two forwards, fold on against off: the latents differ (the fold really ran: other rounding
    points) by far less than the suite's 2e-2 against the oracle; the text K / V caches are the same bits."""
    on, off = tiny["run"](fold=True), tiny["run"](fold=False)
    assert _folded(on[3][1]) and not _folded(off[3][1])
    for i in range(2):
        e = rel_l2(on[i], off[i])
        print(f"tiny model, forward {i}: rel-L2 fold on against off {e:.3e}")
        assert 0 < e <= 2e-2
    for a, b in zip(on[3][1], off[3][1]):
        assert torch.equal(a["k"], b["k"]) and torch.equal(a["v"], b["v"])


def test_unfolded_cases_are_bit_identical_with_fold_off(tiny, monkeypatch):
    """Prompt longer than the cut, fold_text_padding off, fp8 weights, RTV_FOLD_CROSS_V=0: each runs today's code, bit for bit."""
    from realtime_video_amd import ops
    from realtime_video_amd.causal_model import CausalWanModel
    run = tiny["run"]
    rows = 120                                               # kh = 128 > RTV_CROSS_FOLD_KH_MAX
    assert not ops.cross_fold_dims(2, rows)[0]
    a, b = run(ctx_rows=rows, fold=True), run(ctx_rows=rows, fold=False)
    assert not _folded(a[3][1]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    def no_padding_fold(m):
        m.fold_text_padding = False
    ref = run(fold=False, setup=no_padding_fold)
    got = run(fold=True, setup=no_padding_fold)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])

    ref = run(fold=False, setup=lambda m: m.enable_fp8())
    got = run(fold=True, setup=lambda m: m.enable_fp8())
    assert not _folded(got[3][1]) and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])

    monkeypatch.setenv("RTV_FOLD_CROSS_V", "0")
    assert CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64).fold_cross_v is False
    monkeypatch.delenv("RTV_FOLD_CROSS_V")
    assert CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64).fold_cross_v is True
    off = run(fold=False)

    def env_off(m):
        monkeypatch.setenv("RTV_FOLD_CROSS_V", "0")
        m.fold_cross_v = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64).fold_cross_v
        monkeypatch.delenv("RTV_FOLD_CROSS_V")
    got = run(setup=env_off)
    assert torch.equal(got[0], off[0]) and torch.equal(got[1], off[1])


def _fresh_vo(model, ca, layer):
    from realtime_video_amd import ops
    rows = int(ca[layer]["text_rows"])
    ok, kh, kf = ops.cross_fold_dims(model.num_heads, rows)
    assert ok
    fresh = ops.cross_fold_weight(model._tensors[f"L{layer}.co_w"], ca[layer]["v"][0].view(512, model.dim), rows + 1, kh, kf)
    return fresh, ca[layer]["vo"][:model.dim * kf].view(model.dim, kf)


def test_folded_weights_follow_the_caches(tiny):
    """A second prompt of another length on the same caches, then a LoRA load (lora_version bump): the folded weights equal a fresh
    computation from the caches and the live co_w, the buffers never move, and the forward equals a model that starts there."""
    cfg, lat, t = tiny["cfg"], tiny["lat"], tiny["t"]
    _, _, model, (kv, ca, wr, cond) = tiny["run"](setup=lambda m: None)
    ptrs = [c["vo"].data_ptr() for c in ca]
    g = torch.Generator().manual_seed(8)
    ctx2 = torch.randn(23, tiny["text_dim"], generator=g).to(torch.bfloat16).to(DEV)
    for c in ca:
        c["is_init"] = False                                  # a new prompt: the session resets the cross-attention caches
    kv2, _ = _caches(cfg)
    out2, _ = wr(lat[0].to(DEV), {"prompt_embeds": [ctx2]}, t, kv2, ca, current_start=0)
    assert [c["vo"].data_ptr() for c in ca] == ptrs and ca[0]["text_rows"] == 23 and _folded(ca)
    for l in range(cfg["num_layers"]):
        fresh, held = _fresh_vo(model, ca, l)
        assert torch.equal(fresh, held)
    model2, wr2 = _build(cfg, tiny["text_dim"], tiny["w"])
    kv3, ca3 = _caches(cfg)
    ref2, _ = wr2(lat[0].to(DEV), {"prompt_embeds": [ctx2]}, t, kv3, ca3, current_start=0)
    assert torch.equal(out2, ref2)
    # a LoRA on the cross-attention v and o projections of layer 1
    d, r = cfg["dim"], 4
    sd = {}
    for m_ in ("v", "o"):
        sd[f"blocks.1.cross_attn.{m_}.lora_A.weight"] = torch.randn(r, d, generator=g) * 0.05
        sd[f"blocks.1.cross_attn.{m_}.lora_B.weight"] = torch.randn(d, r, generator=g) * 0.05
    v0 = model.lora_version
    model.load_lora(sd, name="a", scale=1.0)
    assert model.lora_version != v0
    kv4, _ = _caches(cfg)
    wr(lat[0].to(DEV), {"prompt_embeds": [ctx2]}, t, kv4, ca, current_start=0)
    assert [c["vo"].data_ptr() for c in ca] == ptrs and _folded(ca)
    for l in range(cfg["num_layers"]):
        fresh, held = _fresh_vo(model, ca, l)
        assert torch.equal(fresh, held)


@pytest.mark.parametrize("heads,world,exchange", [(2, 2, "rows"), (3, 3, "heads"), (12, 4, "heads")])
def test_phase_api_equals_whole_forward_with_the_fold(heads, world, exchange):
    """Fold on, tile config 4 (shard-invariant GEMMs): the context-parallel phase API (simulated ranks) and the whole forward are
    the same bits - both take the same decision and the probabilities kernel computes a row whoever shares its wave.  H = 2, 3
    and 12: H * kh is a multiple of 64 for none of them at 64 prompt rows (144, 216, 864)."""
    from oracle import wan_oracle as wo
    from realtime_video_amd.parallel import SimulatedContextParallel
    cfg, text_dim, tiny_inputs = _tiny(heads)
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    t = torch.ones([1, 3], dtype=torch.int64, device=DEV) * 700
    outs = []
    for cp in (None, SimulatedContextParallel(world, exchange)):
        model, wr = _build(cfg, text_dim, w)
        model.context_parallel = cp
        model.gemm_tile_cfg = 4
        kv, ca = _caches(cfg)
        a, _ = wr(lat[0].to(DEV), cond, t, kv, ca, current_start=0)
        b, _ = wr(lat[3].to(DEV), cond, t, kv, ca, current_start=4680)
        assert _folded(ca)
        outs.append((a.clone(), b.clone(), ca[1]["vo"].clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_hipgraph_replay_of_a_folded_forward_equals_eager(tiny):
    """use_hip_graphs: the third sighting of a launch geometry replays the captured graph, which embeds the addresses and the
    leading dimension of the folded weights: same bits as the eager forward."""
    lat, t = tiny["lat"], tiny["t"]
    _, eager, _, _ = tiny["run"](fold=True)
    _, _, model, (kv, ca, wr, cond) = tiny["run"](setup=lambda m: setattr(m, "use_hip_graphs", True))
    outs = []
    for _ in range(3):                        # the same block again, as the denoise steps do: (seen ->) captured + replayed -> replayed
        o, _ = wr(lat[3].to(DEV), cond, t, kv, ca, current_start=4680)
        outs.append(o.clone())
    assert any(isinstance(v, dict) for v in model._graphs.values()) and _folded(ca)
    for o in outs:
        assert torch.equal(o, eager)
