"""CausalWanModel.enable_fp8_attention(): the tiny model and the three forwards of tests/test_fp8_rows_gpu.py (denoise, block-causal
recompute, second-block denoise) against the oracle graph whose self-attention is the fp8 restatement of tests/attn_fp8_cases.py,
against the bf16 model, and the shadow's bookkeeping: consistency with the bf16 cache, the wrapped ring, hipGraph replay, the
composition with enable_fp8(), the off path and the refusal under context parallelism."""
import gc

import pytest
import torch

import attn_fp8_cases as fc
from conftest import rel_l2
from test_fp8_rows_gpu import _build, _caches, _on_dev, _three_forwards, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
T = torch.ones([1, 3], dtype=torch.int64) * 700
T0 = torch.zeros([1, 3], dtype=torch.int64)


def _fp8_attn_fn(q, k, v):
    """Self-attention in fp8, the text cross-attention (512 keys) as it was."""
    from oracle import wan_oracle as wo
    return wo.attention_sdpa(q, k, v) if k.shape[1] == 512 else fc.restated_attention(q, k, v)


def _fp8_block_causal(q, k, v, block_len):
    from oracle import wan_oracle as wo
    return fc.restated_attention(q, k, v, limits=wo.block_causal_limits(q.shape[1], block_len))


def _oracle_three(wo, w, cfg, lat_d, ctx_d, attn_fn):
    sched = wo.FlowMatchScheduler()
    kvc = wo.initialize_kv_cache(cfg["num_layers"], 1, 9360, cfg["num_heads"], 128, BF, DEV)
    cac = wo.initialize_crossattn_cache(cfg["num_layers"], 1, cfg["num_heads"], 128, BF, device=DEV)
    a, _ = wo.wrapper_forward(w, cfg, sched, lat_d[0], [ctx_d], T.to(DEV), kvc, cac, 0, attn_fn=attn_fn)
    wo.reset_kv_cache(kvc)
    rc, _ = wo.wrapper_forward(w, cfg, sched, lat_d[2], [ctx_d], T0.to(DEV), kvc, cac, 4680, recompute=True, attn_fn=attn_fn)
    b, _ = wo.wrapper_forward(w, cfg, sched, lat_d[3], [ctx_d], T.to(DEV), kvc, cac, 4680, attn_fn=attn_fn)
    return [x.cpu() for x in (a, rc, b)]


def _shadow_matches_cache(kv, scales=(1.0, 1.0)):
    """Every layer's shadow equals a whole-cache quantisation of its bf16 cache (the restatement), bit for bit."""
    for c in kv:
        rows, H = c["k"].shape[1], c["k"].shape[2]
        k8, v8t = fc.empty_shadow(rows, H, device=DEV)
        fc.quantize_kv(c["k"][0], c["v"][0], k8, v8t, 0, rows, *scales)
        assert torch.equal(c["k8"], k8) and torch.equal(c["v8t"], v8t)


def _key_window(lo, hi, ring_lo, ring_size, ring_shift):
    """The physical row ranges of the logical window [lo, hi) of a ring-indexed cache, as csrc/dit_forward.hip's key_window cuts
    them: logical row r >= ring_lo lives at ring_lo + (r - ring_lo + ring_shift) % ring_size.  -> (seg0, seg1), each (row, rows)."""
    S, R = ring_lo, ring_size
    if R <= 0 or hi <= S:
        return (lo, hi - lo), (0, 0)
    rl = max(lo, S)
    n = hi - rl
    p0 = S + (rl - S + ring_shift) % R
    first = n if p0 + n <= S + R else S + R - p0
    sink = S - lo if lo < S else 0
    if first == n:
        if sink == 0:
            return (p0, n), (0, 0)
        return ((lo, sink + n), (0, 0)) if p0 == S else ((lo, sink), (p0, n))
    return (lo if sink else S, sink + n - first), (p0, first)


@pytest.fixture(scope="module")
def tiny():
    from oracle import wan_oracle as wo
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    model, wr = _build(cfg, text_dim, w)
    bf16 = _three_forwards(model, wr, lat, ctx, T, T0)
    return dict(wo=wo, cfg=cfg, text_dim=text_dim, w=w, lat=lat, ctx=ctx, bf16=bf16)


def test_fp8_attention_against_the_oracle_and_the_bf16_model(tiny, monkeypatch):
    """rel-L2 <= 3e-2 per forward against the oracle with the fp8 restatement as self-attention (the bound every quantised mode of
    this project holds against its oracle); against the bf16 model 0 < rel-L2 <= 2 x rel-L2(fp8-attention oracle, bf16 oracle).
    Then: the shadows equal a whole-cache quantisation of the bf16 caches, and disable_fp8_attention() restores the bits of a
    model that never enabled the mode.
    Measured (MI355X), denoise / recompute / second block: 2.85e-3 2.84e-3 2.80e-3 against the fp8 oracle, 3.03e-3 3.03e-3 3.00e-3
    against the bf16 model, 3.23e-3 3.23e-3 3.21e-3 between the two oracles (so the second bound stands at 6.5e-3)."""
    wo, cfg, w, lat, ctx = tiny["wo"], tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    wd, ctx_d, lat_d = _on_dev(dict(w)), ctx.to(DEV), [x.to(DEV) for x in lat]
    ref_bf16 = _oracle_three(wo, wd, cfg, lat_d, ctx_d, None)
    monkeypatch.setattr(wo, "attention_block_causal", _fp8_block_causal)
    ref_fp8 = _oracle_three(wo, wd, cfg, lat_d, ctx_d, _fp8_attn_fn)
    monkeypatch.undo()
    model, wr = _build(cfg, tiny["text_dim"], w)
    assert model.enable_fp8_attention() is model
    with pytest.raises(RuntimeError):
        model.fp8_attention_amax()
    kv_seen = []
    orig = model._fp8_attention.shadow
    model._fp8_attention.shadow = lambda kv, use_cp: (kv_seen.append(kv), orig(kv, use_cp))[1]
    ours = _three_forwards(model, wr, lat, ctx, T, T0)
    vs_oracle = [rel_l2(o, r) for o, r in zip(ours, ref_fp8)]
    vs_bf16 = [rel_l2(o, b) for o, b in zip(ours, tiny["bf16"])]
    oracle_gap = [rel_l2(a, b) for a, b in zip(ref_fp8, ref_bf16)]
    print("fp8 attention vs fp8 oracle:", " ".join(f"{v:.3e}" for v in vs_oracle), "| vs bf16 model:", " ".join(f"{v:.3e}" for v in vs_bf16),
          "| fp8 oracle vs bf16 oracle:", " ".join(f"{v:.3e}" for v in oracle_gap))
    assert all(v <= 3e-2 for v in vs_oracle)
    assert all(0 < v <= 2 * g for v, g in zip(vs_bf16, oracle_gap))
    _shadow_matches_cache(kv_seen[-1])
    amax = model.fp8_attention_amax()
    assert amax.shape == (cfg["num_layers"], 2) and bool((amax > 0).all()) and bool((amax < 448).all())
    for l, c in enumerate(kv_seen[-1]):           # the running maxima cover at least what the caches hold now
        assert float(amax[l, 0]) >= float(c["k"].float().abs().max()) and float(amax[l, 1]) >= float(c["v"].float().abs().max())
    assert model.disable_fp8_attention() is model
    back = _three_forwards(model, wr, lat, ctx, T, T0)
    assert all(torch.equal(a, b) for a, b in zip(back, tiny["bf16"]))


def test_fp8_attention_with_fp8_linears(tiny, monkeypatch):
    """enable_fp8() and enable_fp8_attention() together: <= 3e-2 against the oracle with both restatements.
    Measured (MI355X): 1.47e-2 1.42e-2 2.28e-2."""
    wo, cfg, w, lat, ctx = tiny["wo"], tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    w8 = dict(w)
    w8[wo.FP8_FLAG] = True
    monkeypatch.setattr(wo, "attention_block_causal", _fp8_block_causal)
    ref = _oracle_three(wo, _on_dev(w8), cfg, [x.to(DEV) for x in lat], ctx.to(DEV), _fp8_attn_fn)
    model, wr = _build(cfg, tiny["text_dim"], w)
    model.enable_fp8()
    model.enable_fp8_attention()
    ours = _three_forwards(model, wr, lat, ctx, T, T0)
    errs = [rel_l2(o, r) for o, r in zip(ours, ref)]
    print("fp8 Linears + fp8 attention vs oracle:", " ".join(f"{v:.3e}" for v in errs))
    assert all(v <= 3e-2 for v in errs)


def test_fp8_attention_scale_change_refills_without_allocating(tiny):
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    model, wr = _build(cfg, tiny["text_dim"], w)
    model.enable_fp8_attention()
    kv, ca = _caches(cfg, 9360)
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    ptrs = [(c["k8"].data_ptr(), c["v8t"].data_ptr()) for c in kv]
    model.enable_fp8_attention(k_scale=2.0, v_scale=0.5)
    wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    assert ptrs == [(c["k8"].data_ptr(), c["v8t"].data_ptr()) for c in kv]
    _shadow_matches_cache(kv, (2.0, 0.5))


def test_fp8_attention_on_a_wrapped_ring(tiny, monkeypatch):
    """local_attn_size = 6, sink_size = 1, a cache of 6 x 1560 rows, four blocks: block 3 writes its rows across the end of the
    ring (two physical ranges) and attends a window of two ranges.  Every block <= 3e-2 against the oracle (whose cache is shifted,
    not rotated) with the fp8 restatement; the shadow equals a whole-cache quantisation of the bf16 cache after every block; and
    the self-attention output of every block equals ops.attn_fwd_fp8 on that block's window, bit for bit (the forward's query rows
    and attention output come from the test hook rtv_dit_lab_capture_self_attn).  Measured (MI355X): 2.3e-3 on every block."""
    from realtime_video_amd import _lib, ops
    wo, text_dim, lat, ctx = tiny["wo"], tiny["text_dim"], tiny["lat"], tiny["ctx"]
    cfg = dict(tiny["cfg"], num_layers=1, local_attn_size=6, sink_size=1)
    w = wo.make_weights(cfg, seed=3, text_dim=text_dim)
    model, wr = _build(cfg, text_dim, w)
    model.enable_fp8_attention()
    rows = 6 * 1560
    kv, ca = _caches(cfg, rows)
    kvc = wo.initialize_kv_cache(1, 1, rows, cfg["num_heads"], 128, BF, DEV)
    cac = wo.initialize_crossattn_cache(1, 1, cfg["num_heads"], 128, BF, device=DEV)
    wd, ctx_d = _on_dev(dict(w)), ctx.to(DEV)
    shifts, errs, windows = [], [], []
    M, H = 4680, cfg["num_heads"]
    q_cap, o_cap = (torch.zeros(M, H, 128, dtype=BF, device=DEV) for _ in range(2))
    for b in range(4):
        ref, _ = wo.wrapper_forward(wd, cfg, wo.FlowMatchScheduler(), lat[b].to(DEV), [ctx_d], T.to(DEV), kvc, cac, b * 4680,
                                    attn_fn=_fp8_attn_fn)
        _lib.call("rtv_dit_lab_capture_self_attn", q_cap.data_ptr(), o_cap.data_ptr())
        try:
            flow, _ = wr(lat[b].to(DEV), {"prompt_embeds": [ctx_d]}, T.to(DEV), kv, ca, current_start=b * 4680)
        finally:
            _lib.call("rtv_dit_lab_capture_self_attn", None, None)
        errs.append(rel_l2(flow, ref))
        shifts.append(int(kv[0].get("ring_start", 0)))
        _shadow_matches_cache(kv)
        hi = int(kv[0]["local_end_index"])
        seg0, seg1 = _key_window(max(0, hi - 6 * 1560), hi, int(kv[0]["ring_lo"]), int(kv[0]["ring_size"]), shifts[-1])
        windows.append((seg0, seg1))
        assert torch.equal(ops.attn_fwd_fp8(q_cap, kv[0]["k8"], kv[0]["v8t"], seg0, seg1), o_cap), (b, seg0, seg1)
    print("fp8 attention on the ring vs oracle:", " ".join(f"{v:.3e}" for v in errs), "ring_start", shifts)
    assert all(v <= 3e-2 for v in errs)
    # block 3: ring of 7800 rows behind 1560 sink rows, rotated by 1560: the 4680 new rows land at physical 6240 .. 9360 and 1560 .. 3120
    assert kv[0]["ring_size"] == 5 * 1560 and shifts[3] == 1560 and shifts[2] == 4680
    assert windows[3] == ((0, 3120), (3120, 6240)) and windows[2][1][1] > 0, windows      # two ranges: [sink | wrapped tail], [ring head]


def test_fp8_attention_hip_graph_replay_equals_eager(tiny):
    """use_hip_graphs: the replayed forwards equal the eager ones bit for bit, and nothing is allocated once the first block is over."""
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    outs = {}
    for graphs in (False, True):
        model, wr = _build(cfg, tiny["text_dim"], w)
        model.enable_fp8_attention()
        model.use_hip_graphs = graphs
        kv, ca = _caches(cfg, 9360)
        cond = {"prompt_embeds": [ctx.to(DEV)]}
        seq = []
        wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)            # fills the text caches and the shadows: never a graph
        lats = [x.to(DEV) for x in lat]
        tt = T.to(DEV)
        for rep in range(3):                                                    # the same step three times: eager, capture, replay
            if rep == 2:
                gc.collect()                                                    # garbage of earlier tests must not be freed inside the window
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
            for c in kv:
                c["global_end_index"] = c["local_end_index"] = 4680
            out, _ = wr(lats[1 + rep], cond, tt, kv, ca, current_start=4680)
            seq.append(out.cpu())
            del out
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, "a later block allocated"
        if graphs:
            assert any(isinstance(e, dict) for e in model._graphs.values()), "no graph was captured"
        _shadow_matches_cache(kv)
        outs[graphs] = seq
    assert all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))


def test_fp8_attention_refuses_context_parallelism(tiny):
    from realtime_video_amd.parallel import SimulatedContextParallel
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    model, wr = _build(cfg, tiny["text_dim"], w)
    model.context_parallel = SimulatedContextParallel(2, "heads")
    model.enable_fp8_attention()
    kv, ca = _caches(cfg, 9360)
    with pytest.raises(RuntimeError, match="context parallelism"):
        wr(lat[0].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=0)
    assert int(kv[0]["local_end_index"]) == 0 and "k8" not in kv[0]
    with pytest.raises(ValueError):
        model.enable_fp8_attention(k_scale=0.0)


def test_native_forward_refuses_sharded_and_split_fp8_steps(tiny, monkeypatch):
    """Behind the Python check: rtv_dit_forward_attn_fp8 with a step that is sharded (row_count < M) or asks for the KV split is an
    error that names the reason - it never runs in bf16.  The step is the one a real fp8 forward has just issued, altered; every altered call is refused before any launch."""
    import ctypes

    from realtime_video_amd import _lib
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    model, wr = _build(cfg, tiny["text_dim"], w)
    model.enable_fp8_attention()
    kv, ca = _caches(cfg, 9360)
    seen, real = [], _lib.call

    def spy(name, *args):
        if name == "rtv_dit_forward_attn_fp8":
            seen.append(args)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    wr(lat[0].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=0)
    monkeypatch.undo()
    assert len(seen) == 1, "the fp8 forward did not go through rtv_dit_forward_attn_fp8"
    args = seen[0]
    step = args[2]._obj
    step.row_count = 2340
    with pytest.raises(RuntimeError, match="fp8 attention does not support sharded calls"):
        real("rtv_dit_forward_attn_fp8", *args)
    step.row_begin, step.row_count = 2340, 0
    with pytest.raises(RuntimeError, match="fp8 attention does not support sharded calls"):
        real("rtv_dit_forward_attn_fp8", *args)
    step.row_begin, step.attn_kv_splits = 0, 2
    with pytest.raises(RuntimeError, match="fp8 attention does not support attn_kv_splits"):
        real("rtv_dit_forward_attn_fp8", *args)
    step.attn_kv_splits = 1
    with pytest.raises(RuntimeError, match="needs its shadow"):
        real("rtv_dit_forward_attn_fp8", *args[:3], None, *args[4:])
    torch.cuda.synchronize()
