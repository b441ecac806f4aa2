"""CausalWanModel.enable_fp8_attention(context_parallel=True): the sharded phases of include/rtv_hip_attn_fp8_cp.h on the tiny
model, several shards in lockstep on one GPU (SimulatedContextParallel).  The fp8 attention arithmetic is per row - Q is quantised
per (row, head), K and V per element with global scales, one lane owns one query column - so with attn_kv_splits = 1 a sharded
forward must equal the unsharded fp8-attention forward BIT FOR BIT: outputs, bf16 caches and e4m3 shadows.  With the KV split, and
on a rolling cache (which the context-parallel path shift-copies where the unsharded one rotates a ring), the bar is the oracle
with the fp8 restatement of tests/attn_fp8_cases.py."""
import gc

import pytest
import torch

import attn_fp8_cases as fc
from conftest import rel_l2
from test_attn_fp8_model_gpu import T, T0, _fp8_attn_fn, _fp8_block_causal, _oracle_three
from test_fp8_rows_gpu import _build, _caches, _on_dev, _three_forwards, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
M = 4680


def _cp(world, exchange, splits=1):
    from realtime_video_amd.parallel import SimulatedContextParallel
    return SimulatedContextParallel(world, exchange, attn_kv_splits=splits)


def _spy_caches(model):
    seen = []
    orig = model._fp8_attention.shadow
    model._fp8_attention.shadow = lambda kv, use_cp: (seen.append(kv), orig(kv, use_cp))[1]
    return seen


def _model(tiny, cp=None, cfg=None, w=None, **enable):
    model, wr = _build(cfg or tiny["cfg"], tiny["text_dim"], w or tiny["w"])
    model.context_parallel = cp
    model.enable_fp8_attention(context_parallel=cp is not None, **enable)
    return model, wr


def _shadows_match_cache(model, kv):
    """Every shadow equals a whole-cache quantisation (the restatement) of what it mirrors: the full-head shadow of the row exchange
    (and of the unsharded forward) the whole cache, the per-rank shadows of the head exchange the rank's head slice."""
    cp = model.context_parallel if model is not None else None      # (None: an unsharded forward's caches)
    for c in kv:
        rows, H = c["k"].shape[1], c["k"].shape[2]
        if cp is None or not cp.head_exchange(model.num_heads):
            k8, v8t = fc.empty_shadow(rows, H, device=DEV)
            fc.quantize_kv(c["k"][0], c["v"][0], k8, v8t, 0, rows)
            assert torch.equal(c["k8"], k8) and torch.equal(c["v8t"], v8t)
            continue
        hn = H // cp.world
        assert len(c["k8_hp"]) == cp.world
        for r in range(cp.world):
            k8, v8t = fc.empty_shadow(rows, hn, device=DEV)
            fc.quantize_kv(c["k"][0][:, r * hn:(r + 1) * hn], c["v"][0][:, r * hn:(r + 1) * hn], k8, v8t, 0, rows)
            assert torch.equal(c["k8_hp"][r], k8) and torch.equal(c["v8t_hp"][r], v8t), f"rank {r}"


def _same_caches(kv, ref):
    assert all(torch.equal(a[n], b[n]) for a, b in zip(kv, ref) for n in ("k", "v"))


@pytest.fixture(scope="module")
def tiny():
    from oracle import wan_oracle as wo
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    t = dict(wo=wo, cfg=cfg, text_dim=text_dim, w=w, lat=lat, ctx=ctx)
    model, wr = _model(t)
    seen = _spy_caches(model)
    t["whole"] = _three_forwards(model, wr, lat, ctx, T, T0)            # the unsharded fp8-attention forwards and what they leave
    t["whole_kv"] = seen[-1]
    return t


@pytest.fixture(scope="module")
def oracle_fp8(tiny):
    wo = tiny["wo"]
    old = wo.attention_block_causal
    wo.attention_block_causal = _fp8_block_causal
    try:
        return _oracle_three(wo, _on_dev(dict(tiny["w"])), tiny["cfg"], [x.to(DEV) for x in tiny["lat"]], tiny["ctx"].to(DEV), _fp8_attn_fn)
    finally:
        wo.attention_block_causal = old


def _largest_world(heads):
    return max(n for n in range(1, 9) if heads % n == 0 and M % n == 0)


@pytest.mark.parametrize("exchange,world", [("rows", 2), ("heads", 2), ("auto", 0)], ids=["rows2", "heads2", "largest"])
def test_sharded_forward_equals_the_unsharded_one_bit_for_bit(tiny, exchange, world):
    world = world or _largest_world(tiny["cfg"]["num_heads"])
    model, wr = _model(tiny, _cp(world, exchange))
    seen = _spy_caches(model)
    ours = _three_forwards(model, wr, tiny["lat"], tiny["ctx"], T, T0)
    for i, (a, b) in enumerate(zip(ours, tiny["whole"])):
        assert torch.equal(a, b), f"forward {i}: rel-L2 {rel_l2(a, b):.3e}"
    _same_caches(seen[-1], tiny["whole_kv"])
    _shadows_match_cache(model, seen[-1])
    _shadows_match_cache(None, tiny["whole_kv"])


def _recompute_then_denoise(tiny, model, wr, only):
    """tests/test_dit_gpu.py's kv_cache_only sequence: a full recompute forward that fills the text caches, the recompute pass proper
    (kv_cache_only takes effect here: the last layer stops behind its exchange), a denoise step on the recomputed cache."""
    lat, cond = tiny["lat"], {"prompt_embeds": [tiny["ctx"].to(DEV)]}
    kv, ca = _caches(tiny["cfg"], 9360)
    model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3)
    wr(lat[2].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680, kv_cache_only=only)
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    rc, _ = wr(lat[1].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680, kv_cache_only=only)
    model.block_mask = None
    if only:
        assert float(rc.float().abs().max()) == 0
        _shadows_match_cache(model, kv)                 # the last layer's shadow included: quantised behind its exchange
    nxt, _ = wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    return nxt.cpu(), kv


@pytest.mark.parametrize("exchange", ["rows", "heads"])
def test_kv_cache_only_pass_keeps_the_last_layers_shadow_current(tiny, exchange):
    want, want_kv = _recompute_then_denoise(tiny, *_model(tiny), only=False)
    model, wr = _model(tiny, _cp(2, exchange))
    got, kv = _recompute_then_denoise(tiny, model, wr, only=True)
    assert torch.equal(got, want), f"rel-L2 {rel_l2(got, want):.3e}"
    _same_caches(kv, want_kv)
    _shadows_match_cache(model, kv)


def test_fp8_row_linears_with_sharded_fp8_attention(tiny):
    outs = []
    for cp in (_cp(2, "auto"), None):
        model, wr = _build(tiny["cfg"], tiny["text_dim"], tiny["w"])
        model.context_parallel = cp
        model.enable_fp8("row")
        model.enable_fp8_attention(context_parallel=cp is not None)
        outs.append(_three_forwards(model, wr, tiny["lat"], tiny["ctx"], T, T0))
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), f"forward {i}: rel-L2 {rel_l2(a, b):.3e}"


@pytest.mark.parametrize("exchange", ["rows", "heads"])
def test_kv_split_against_the_oracle(tiny, oracle_fp8, exchange):
    """attn_kv_splits = 2: <= 3e-2 per forward against the oracle with the fp8 restatement (the bound every quantised mode here holds);
    the distance to the S = 1 run is printed and gets no bar (the split changes each range's reference point, hence P's rounding)."""
    model, wr = _model(tiny, _cp(2, exchange, splits=2))
    ours = _three_forwards(model, wr, tiny["lat"], tiny["ctx"], T, T0)
    errs = [rel_l2(o, r) for o, r in zip(ours, oracle_fp8)]
    print(f"ATTN_FP8_CP kv_splits=2 {exchange}: vs fp8 oracle", " ".join(f"{v:.3e}" for v in errs), "| vs S=1",
          " ".join(f"{rel_l2(o, w):.3e}" for o, w in zip(ours, tiny["whole"])))
    assert model._cfg.max_attn_kv_splits >= 2
    assert all(v <= 3e-2 for v in errs)


@pytest.mark.parametrize("exchange", ["rows", "heads"])
def test_hip_graph_replay_equals_eager(tiny, exchange):
    """use_hip_graphs under two shards: the replayed forwards equal the eager ones bit for bit, and nothing is allocated once the
    first block is over (the shadows of both exchanges are allocated once; captured graphs embed their addresses)."""
    lat, ctx = tiny["lat"], tiny["ctx"]
    outs = {}
    for graphs in (False, True):
        model, wr = _model(tiny, _cp(2, exchange))
        model.use_hip_graphs = graphs
        kv, ca = _caches(tiny["cfg"], 9360)
        cond = {"prompt_embeds": [ctx.to(DEV)]}
        seq = []
        wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)            # fills the text caches and the shadows: never a graph
        lats = [x.to(DEV) for x in lat]
        tt = T.to(DEV)
        for rep in range(3):                                                    # the same step three times: eager, capture, replay
            if rep == 2:
                gc.collect()
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
        _shadows_match_cache(model, kv)
        outs[graphs] = seq
    assert all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))


def test_refusals(tiny):
    model, wr = _build(tiny["cfg"], tiny["text_dim"], tiny["w"])
    with pytest.raises(ValueError, match="smooth_k"):
        model.enable_fp8_attention(smooth_k=True, context_parallel=True)
    model.context_parallel = _cp(2, "rows")
    model.enable_fp8_attention()                                                # without the keyword: today's refusal
    kv, ca = _caches(tiny["cfg"], 9360)
    with pytest.raises(RuntimeError, match="context parallelism"):
        wr(tiny["lat"][0].to(DEV), {"prompt_embeds": [tiny["ctx"].to(DEV)]}, T.to(DEV), kv, ca, current_start=0)
    assert int(kv[0]["local_end_index"]) == 0 and "k8" not in kv[0]


def test_rolling_cache_under_two_shards(tiny):
    """local_attn_size = 6, sink_size = 1, a cache of 6 x 1560 rows, four blocks, two shards, both exchanges: the context-parallel
    path shift-copies the rows (the shadows go stale and the same forward refills them whole).  Every block <= 3e-2 against the oracle
    with the fp8 restatement, and the shadows equal a whole-cache quantisation after every block.  Not bit-identical with the
    unsharded ring run: the kernel walks physical storage tiles, and the shifted cache places the keys differently."""
    wo, text_dim, lat, ctx = tiny["wo"], tiny["text_dim"], tiny["lat"], tiny["ctx"]
    cfg = dict(tiny["cfg"], num_layers=1, local_attn_size=6, sink_size=1)
    w = wo.make_weights(cfg, seed=3, text_dim=text_dim)
    rows = 6 * 1560
    wd, ctx_d = _on_dev(dict(w)), ctx.to(DEV)
    kvc = wo.initialize_kv_cache(1, 1, rows, cfg["num_heads"], 128, BF, DEV)
    cac = wo.initialize_crossattn_cache(1, 1, cfg["num_heads"], 128, BF, device=DEV)
    refs = [wo.wrapper_forward(wd, cfg, wo.FlowMatchScheduler(), lat[b].to(DEV), [ctx_d], T.to(DEV), kvc, cac, b * M, attn_fn=_fp8_attn_fn)[0]
            for b in range(4)]
    for exchange in ("rows", "heads"):
        model, wr = _model(tiny, _cp(2, exchange), cfg=cfg, w=w)
        kv, ca = _caches(cfg, rows)
        errs = []
        for b in range(4):
            flow, _ = wr(lat[b].to(DEV), {"prompt_embeds": [ctx_d]}, T.to(DEV), kv, ca, current_start=b * M)
            errs.append(rel_l2(flow, refs[b]))
            _shadows_match_cache(model, kv)
        print(f"ATTN_FP8_CP rolling cache, 2 shards ({exchange}) vs fp8 oracle:", " ".join(f"{v:.3e}" for v in errs))
        assert all(v <= 3e-2 for v in errs)
        assert int(kv[0]["local_end_index"]) == rows and int(kv[0].get("ring_start", 0)) == 0      # shifted, not rotated


def test_native_phases_refuse_a_missing_shadow_and_an_unplanned_split(tiny, monkeypatch):
    """Behind the Python side: the fp8 phases with a null shadow, a head count outside 1..num_heads, or a step that asks for more
    ranges than rtv_dit_config.max_attn_kv_splits planned the workspace for are errors that name the reason - before any launch of
    theirs, never a bf16 run.  The calls are those a real sharded forward has just issued, altered."""
    from realtime_video_amd import _lib
    model, wr = _model(tiny, _cp(2, "rows"))
    kv, ca = _caches(tiny["cfg"], 9360)
    seen, real = {}, _lib.call

    def spy(name, *args):
        seen.setdefault(name, args)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    cond = {"prompt_embeds": [tiny["ctx"].to(DEV)]}
    wr(tiny["lat"][0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    wr(tiny["lat"][1].to(DEV), cond, T.to(DEV), kv, ca, current_start=M, kv_cache_only=True)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert "rtv_dit_layer_rest" not in seen and "rtv_dit_forward_attn_fp8" not in seen
    rest, quant = seen["rtv_dit_layer_rest_attn_fp8"], seen["rtv_dit_quantize_block_attn_fp8"]
    with pytest.raises(RuntimeError, match="needs its shadow"):
        real("rtv_dit_layer_rest_attn_fp8", *rest[:4], None, *rest[5:])
    with pytest.raises(RuntimeError, match="needs its shadow"):
        real("rtv_dit_quantize_block_attn_fp8", *quant[:4], None, quant[5])
    for heads in (0, tiny["cfg"]["num_heads"] + 1):
        with pytest.raises(RuntimeError, match="heads must be"):
            real("rtv_dit_quantize_block_attn_fp8", *quant[:3], heads, *quant[4:])
    step = rest[2]._obj
    step.attn_kv_splits = model._cfg.max_attn_kv_splits + 1
    before = [c["k8"].clone() for c in kv]
    with pytest.raises(RuntimeError, match="max_attn_kv_splits"):
        real("rtv_dit_layer_rest_attn_fp8", *rest)
    step.attn_kv_splits = 1
    torch.cuda.synchronize()
    assert all(torch.equal(a, c["k8"]) for a, c in zip(before, kv))
