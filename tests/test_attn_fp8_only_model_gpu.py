"""CausalWanModel.enable_fp8_attention(bf16_cache=False): the e4m3-only KV cache (include/rtv_hip_attn_fp8_only.h) against the
shadow mode of the same model, bit for bit - outputs, codes and running maxima - on the tiny model and the forwards of
tests/test_fp8_rows_gpu.py / tests/test_attn_fp8_model_gpu.py; then what the mode is for (the allocation) and what it refuses."""
import gc

import pytest
import torch

from test_fp8_rows_gpu import _build, _caches, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
T = torch.ones([1, 3], dtype=torch.int64) * 700
T0 = torch.zeros([1, 3], dtype=torch.int64)


@pytest.fixture(scope="module")
def tiny():
    from oracle import wan_oracle as wo
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    return dict(wo=wo, cfg=cfg, text_dim=text_dim, w=w, lat=lat, ctx=ctx)


def _model(tiny, only, fp8_linears=False, cfg=None, w=None, scales=(1.0, 1.0)):
    model, wr = _build(cfg or tiny["cfg"], tiny["text_dim"], w or tiny["w"])
    if fp8_linears:
        model.enable_fp8()
    model.enable_fp8_attention(*scales, bf16_cache=not only)
    return model, wr


def _kv(model, cfg, rows, only):
    """The KV and cross-attention caches of one side: compact dicts in the mode, the bf16 ones of the other tests outside it."""
    kv, ca = _caches(cfg, rows)
    return (model.new_fp8_kv_cache(rows, DEV) if only else kv), ca


def _codes(kv):
    return [(c["k8"].clone(), c["v8t"].clone()) for c in kv]


def _same_codes(a, b):
    return all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def _three_forwards(model, wr, lat, ctx, kv, ca):
    """tests/test_fp8_rows_gpu.py's sequence on the caches given: denoise at offset 0, block-causal recompute, second-block denoise.
    -> (outputs, the codes of every layer behind each forward)."""
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    outs, codes = [], []
    outs.append(wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)[0].cpu())
    codes.append(_codes(kv))
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3)
    outs.append(wr(lat[2].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680)[0].cpu())
    model.block_mask = None
    codes.append(_codes(kv))
    outs.append(wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)[0].cpu())
    codes.append(_codes(kv))
    return outs, codes


@pytest.mark.parametrize("fp8_linears", [False, True])
def test_three_forwards_equal_the_shadow_mode(tiny, fp8_linears):
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    got = {}
    for only in (False, True):
        model, wr = _model(tiny, only, fp8_linears)
        kv, ca = _kv(model, cfg, 9360, only)
        outs, codes = _three_forwards(model, wr, lat, ctx, kv, ca)
        got[only] = (outs, codes, model.fp8_attention_amax().clone())
        if only:
            assert all("k" not in c and "v" not in c for c in kv) and int(kv[0]["local_end_index"]) == 9360
    (o_s, c_s, a_s), (o_o, c_o, a_o) = got[False], got[True]
    for i in range(3):
        assert torch.equal(o_o[i], o_s[i]), f"output of forward {i}"
        assert _same_codes(c_o[i], c_s[i]), f"codes behind forward {i}"
    assert torch.equal(a_o, a_s) and bool((a_o > 0).all())
    assert bool(c_o[2][0][0][:9360].any()) and bool(torch.isfinite(o_o[2]).all())


def test_wrapped_ring_equals_the_shadow_mode(tiny):
    """The configuration of test_fp8_attention_on_a_wrapped_ring: local_attn_size = 6, sink_size = 1, one layer, four blocks - block 3
    writes across the end of the ring and attends two ranges.  Outputs and codes after every block."""
    wo, lat, ctx = tiny["wo"], tiny["lat"], tiny["ctx"]
    cfg = dict(tiny["cfg"], num_layers=1, local_attn_size=6, sink_size=1)
    w = wo.make_weights(cfg, seed=3, text_dim=tiny["text_dim"])
    rows = 6 * 1560
    got = {}
    for only in (False, True):
        model, wr = _model(tiny, only, cfg=cfg, w=w)
        kv, ca = _kv(model, cfg, rows, only)
        seq = []
        for b in range(4):
            flow, _ = wr(lat[b].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=b * 4680)
            seq.append((flow.cpu(), _codes(kv), int(kv[0].get("ring_start", 0))))
        got[only] = (seq, model.fp8_attention_amax().clone())
    for b, (s, o) in enumerate(zip(got[False][0], got[True][0])):
        assert torch.equal(o[0], s[0]), f"output of block {b}"
        assert _same_codes(o[1], s[1]), f"codes behind block {b}"
        assert o[2] == s[2]
    assert got[True][0][3][2] == 1560 and got[True][0][2][2] == 4680          # the ring did rotate, and block 3's write wrapped
    assert torch.equal(got[True][1], got[False][1])


def test_hip_graph_replay_equals_eager(tiny):
    """use_hip_graphs in the mode: replayed forwards equal eager ones bit for bit, nothing is allocated once the first block is over,
    and a graph was captured."""
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    outs = {}
    for graphs in (False, True):
        model, wr = _model(tiny, True)
        model.use_hip_graphs = graphs
        kv, ca = _kv(model, cfg, 9360, True)
        cond = {"prompt_embeds": [ctx.to(DEV)]}
        seq = []
        wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)            # fills the text caches: never a graph
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
            assert all(k[-1][0] == "only" for k in model._graphs), "the graph key does not carry the mode"
        outs[graphs] = (seq, _codes(kv))
    assert all(torch.equal(a, b) for a, b in zip(outs[False][0], outs[True][0])) and _same_codes(outs[False][1], outs[True][1])


def _pipeline(wr):
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    return CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 750, 500, 250]), DEV, generator=wr,
                                   text_encoder=None, vae=None)


def test_pipeline_allocates_the_two_code_arrays_and_nothing_else(tiny):
    """What the mode is for.  Per layer exactly RTV_ATTN_FP8_K8_BYTES + RTV_ATTN_FP8_V8T_BYTES (include/rtv_hip_attn_fp8.h); the
    allocator may round each of the 2 L tensors up by at most 512 bytes."""
    cfg = tiny["cfg"]
    L, H = cfg["num_layers"], cfg["num_heads"]
    model, wr = _model(tiny, True, cfg=dict(cfg, local_attn_size=6))
    pipe = _pipeline(wr)
    rows = 6 * 1560
    k8_bytes, v8t_bytes = rows * H * 128, ((rows + 63) // 64) * H * 8192
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    pipe._initialize_kv_cache(1, BF, DEV)
    delta = torch.cuda.memory_allocated() - before
    kv = pipe.kv_cache1
    assert len(kv) == L and all("k" not in c and "v" not in c for c in kv)
    for c in kv:
        assert c["rows"] == rows and c["global_end_index"] == 0 and c["local_end_index"] == 0
        assert c["k8"].numel() * c["k8"].element_size() == k8_bytes and c["v8t"].numel() * c["v8t"].element_size() == v8t_bytes
    assert L * (k8_bytes + v8t_bytes) <= delta <= L * (k8_bytes + v8t_bytes + 2 * 512), delta
    # a reset resets the indices and allocates nothing; zero_on_reset stays honoured
    ptrs = [(c["k8"].data_ptr(), c["v8t"].data_ptr()) for c in kv]
    for zero in (False, True):
        for c in kv:
            c["k8"].fill_(3)
            c["v8t"].fill_(3)
            c["global_end_index"] = c["local_end_index"] = 1560
        pipe.zero_on_reset = zero
        pipe._initialize_kv_cache(1, BF, DEV)
        assert pipe.kv_cache1 is kv and ptrs == [(c["k8"].data_ptr(), c["v8t"].data_ptr()) for c in kv]
        assert all(c["global_end_index"] == 0 and c["local_end_index"] == 0 for c in kv)
        assert all(bool((c["k8"] == (0 if zero else 3)).all()) and bool((c["v8t"] == (0 if zero else 3)).all()) for c in kv)
    assert torch.cuda.memory_allocated() - before == delta


def test_session_equals_the_shadow_mode_session(tiny, monkeypatch):
    """A GenerationSession over three blocks at 416 x 240 (390 tokens per frame), recompute passes included: the latents of the
    compact-cache session equal the shadow-mode session's bit for bit."""
    from realtime_video_amd import _lib
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    text_dim, ctx = tiny["text_dim"], tiny["ctx"]
    g = torch.Generator().manual_seed(6)
    noise = torch.randn(1, 9, 16, 30, 52, generator=g).to(BF)
    padded = torch.zeros(1, 512, text_dim, dtype=BF)
    padded[0, :ctx.shape[0]] = ctx
    steps, real = [], _lib.call

    def spy(name, *args):
        if name.startswith("rtv_dit_forward"):
            steps.append((name, args[2]._obj.causal_block, args[2]._obj.kv_only))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    latents = {}
    for only in (False, True):
        model, wr = _model(tiny, only)
        pipe = _pipeline(wr)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(padded.to(DEV)))
        sess = GenerationSession(GenerateParams(seed=9, num_blocks=3, num_denoising_steps=4, keep_first_frame=True, width=416, height=240),
                                 models, device=DEV)
        assert ("k" in pipe.kv_cache1[0]) == (not only)
        sess.noise = noise.to(DEV)
        cpu_rnd = torch.Generator().manual_seed(9)
        sess._randn = lambda shape: torch.randn(*shape, generator=cpu_rnd, dtype=BF).to(DEV)
        del steps[:]
        blocks = [sess.generate_block().cpu() for _ in range(3)]
        names = {n for n, _, _ in steps}
        assert names == {"rtv_dit_forward_attn_fp8_only" if only else "rtv_dit_forward_attn_fp8"}, names
        assert any(cb > 0 for _, cb, _ in steps), "the session ran no recompute pass"
        latents[only] = (blocks, sess.all_latents.cpu(), _codes(pipe.kv_cache1))
    for b in range(3):
        assert torch.equal(latents[True][0][b], latents[False][0][b]), b
    assert torch.equal(latents[True][1], latents[False][1]) and bool(torch.isfinite(latents[True][1].float()).all())
    assert _same_codes(latents[True][2], latents[False][2])


def test_python_refusals_leave_the_indices_alone(tiny):
    from realtime_video_amd.parallel import SimulatedContextParallel
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    model, wr = _model(tiny, True)
    kv, ca = _kv(model, cfg, 9360, True)
    wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    codes = _codes(kv)

    def refused(exc, match, caches, call=None):
        before = [(c["global_end_index"], c["local_end_index"]) for c in caches]
        with pytest.raises(exc, match=match):
            (call or (lambda: wr(lat[3].to(DEV), cond, T.to(DEV), caches, ca, current_start=4680)))()
        assert before == [(c["global_end_index"], c["local_end_index"]) for c in caches]

    refused(ValueError, "smooth_k", kv, lambda: model.enable_fp8_attention(smooth_k=True, bf16_cache=False))
    refused(ValueError, "context parallelism", kv, lambda: model.enable_fp8_attention(context_parallel=True, bf16_cache=False))
    refused(RuntimeError, "smooth_k=True", kv, lambda: model.fp8_attention_recenter(kv))
    bf16_kv = _caches(cfg, 9360)[0]
    refused(RuntimeError, "needs the compact KV cache", bf16_kv)                                       # a dict with "k" / "v" in the mode
    mixed = [dict(c, k=b["k"], v=b["v"]) for c, b in zip(kv, bf16_kv)]
    refused(RuntimeError, "needs the compact KV cache", mixed)
    model.enable_fp8_attention(k_scale=2.0, v_scale=0.5, bf16_cache=False)                             # new scales on a cache that holds rows
    refused(RuntimeError, "reset the cache", kv)
    model.context_parallel = SimulatedContextParallel(2, "heads")                                      # context_parallel set behind the enable
    refused(RuntimeError, "context parallelism", kv)
    refused(ValueError, "context parallelism", kv, lambda: model.enable_fp8_attention(bf16_cache=False))
    model.context_parallel = None
    model.enable_fp8_attention()                                                                       # a compact dict outside the mode: shadow mode,
    refused(RuntimeError, "e4m3-only", kv)
    model.disable_fp8_attention()                                                                      # ... and bf16 attention
    refused(RuntimeError, "e4m3-only", kv)
    assert _same_codes(_codes(kv), codes), "a refused forward wrote into the cache"
    # back in the mode with the scales the rows were made with, the cache goes on; with new scales after a reset as well
    model.enable_fp8_attention(bf16_cache=False)
    wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    assert int(kv[0]["local_end_index"]) == 9360
    model.enable_fp8_attention(k_scale=2.0, v_scale=0.5, bf16_cache=False)
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    assert int(kv[0]["local_end_index"]) == 4680 and kv[0]["fp8_scales"] == (2.0, 0.5)


def test_native_forward_refusals(tiny, monkeypatch):
    """rtv_dit_forward_attn_fp8_only with the step a real forward has just issued, altered: sharded and split steps and a missing or
    unusable shadow are refused with rtv_dit_forward_attn_fp8's messages before any launch - the codes stay as they were.  The
    step's kv_k / kv_v are null pointers: the forward that has just run never followed them."""
    from realtime_video_amd import _lib
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    model, wr = _model(tiny, True)
    kv, ca = _kv(model, cfg, 9360, True)
    seen, real = [], _lib.call

    def spy(name, *args):
        if name.startswith("rtv_dit_forward"):
            seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    wr(lat[0].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=0)
    monkeypatch.undo()
    assert [n for n, _ in seen] == ["rtv_dit_forward_attn_fp8_only"]
    name, args = seen[0]
    step, shadow = args[2]._obj, args[3]._obj
    assert not step.kv_k and not step.kv_v
    torch.cuda.synchronize()
    codes = _codes(kv)

    def refused(match, *a):
        with pytest.raises(RuntimeError, match=match):
            real(name, *(a or args))

    step.row_count = 2340
    refused("fp8 attention does not support sharded calls")
    step.row_begin, step.row_count = 2340, 0
    refused("fp8 attention does not support sharded calls")
    step.row_begin, step.attn_kv_splits = 0, 2
    refused("fp8 attention does not support attn_kv_splits")
    step.attn_kv_splits = 1
    refused("needs its shadow", *args[:3], None, *args[4:])
    shadow.cache_rows = 0
    refused("needs the k8 / v8t shadow arrays and cache_rows")
    shadow.cache_rows = 4679                                 # the rows this call writes end outside the cache
    refused(r"outside \[0, cache_rows\)")
    shadow.cache_rows, shadow.k_scale = 9360, 0.0
    refused("scales must be finite and positive")
    shadow.k_scale = 1.0
    k8_0 = shadow.k8[0]
    shadow.k8[0] = None
    refused("a layer has no shadow")
    shadow.k8[0] = k8_0 + 8
    refused("16-byte aligned")
    shadow.k8[0] = k8_0
    step.ring_lo, step.ring_size, step.ring_shift = 0, 4680, 4680
    refused("bad ring window")
    step.ring_lo, step.ring_size, step.ring_shift = 0, 0, 0
    torch.cuda.synchronize()
    assert _same_codes(_codes(kv), codes), "a refused call wrote into the cache"
