"""CausalWanModel.enable_fp8_attention(bf16_cache=False, context_parallel="codes"): the e4m3-only KV cache under the row exchange of
context parallelism with the exchange carrying codes (include/rtv_hip_attn_fp8_only_cp.h), on the tiny model of
tests/test_fp8_rows_gpu.py - 4680 rows a block, 2340 / 585 rows a shard at 2 / 8 ranks, every shard boundary inside a 64-row storage
tile.  Everything is bit for bit: against the shadow mode's context_parallel=True run on the same shards (same GEMMs, same codes) and
against the unsharded compact forward.  Ranks run in lockstep on one GPU (SimulatedContextParallel), then as two real processes."""
import gc
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_attn_fp8_only_model_gpu import T, T0, _codes, _kv, _pipeline, _same_codes, _three_forwards
from test_context_parallel_gpu import _free_port
from test_fp8_rows_gpu import _build, _caches, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
M = 4680


def _cp(world, exchange="rows", splits=1):
    from realtime_video_amd.parallel import SimulatedContextParallel
    return SimulatedContextParallel(world, exchange, attn_kv_splits=splits)


def _model(tiny, mode, cp=None, cfg=None, w=None):
    """mode "codes": the compact cache, the exchange carrying codes; "compact": the compact cache (unsharded); "shadow": the bf16
    cache with its e4m3 shadow, context_parallel=True when sharded."""
    model, wr = _build(cfg or tiny["cfg"], tiny["text_dim"], w or tiny["w"])
    model.context_parallel = cp
    if mode == "codes":
        model.enable_fp8_attention(bf16_cache=False, context_parallel="codes")
    elif mode == "compact":
        model.enable_fp8_attention(bf16_cache=False)
    else:
        model.enable_fp8_attention(context_parallel=cp is not None)
    return model, wr


def _run_three(tiny, mode, cp=None):
    model, wr = _model(tiny, mode, cp)
    kv, ca = _kv(model, tiny["cfg"], 9360, mode != "shadow")
    outs, codes = _three_forwards(model, wr, tiny["lat"], tiny["ctx"], kv, ca)
    if mode != "shadow":
        assert all("k" not in c and "v" not in c for c in kv)
    return outs, codes, model.fp8_attention_amax().clone()


@pytest.fixture(scope="module")
def tiny():
    from oracle import wan_oracle as wo
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    t = dict(wo=wo, cfg=cfg, text_dim=text_dim, w=w, lat=lat, ctx=ctx)
    t["whole"] = _run_three(t, "compact")          # the unsharded compact forwards: computed once, never modified
    return t


def _assert_same_run(got, want, what):
    (o_g, c_g, a_g), (o_w, c_w, a_w) = got, want
    for i in range(len(o_w)):
        assert torch.equal(o_g[i], o_w[i]), f"{what}: output of forward {i}"
        assert _same_codes(c_g[i], c_w[i]), f"{what}: codes behind forward {i}"
    assert torch.equal(a_g, a_w), f"{what}: amax {a_g.tolist()} != {a_w.tolist()}"


@pytest.mark.parametrize("world", [2, 8])
def test_three_forwards_equal_the_shadow_mode_on_the_same_shards_and_the_unsharded_compact_forward(tiny, world):
    got = _run_three(tiny, "codes", _cp(world))
    _assert_same_run(got, _run_three(tiny, "shadow", _cp(world)), "shadow mode, same shards")
    _assert_same_run(got, tiny["whole"], "unsharded compact forward")
    assert bool(got[1][2][0][0][:9360].any()) and bool(torch.isfinite(got[0][2]).all()) and bool((got[2] > 0).all())


def _recompute_then_denoise(tiny, model, wr, only):
    """tests/test_attn_fp8_cp_gpu.py's kv_cache_only sequence on compact dicts: a full recompute forward that fills the text caches,
    the recompute pass proper (kv_cache_only takes effect here: the last layer stops behind its exchange, with the commit-only
    call), a denoise step on the recomputed cache."""
    lat, cond = tiny["lat"], {"prompt_embeds": [tiny["ctx"].to(DEV)]}
    kv, ca = _kv(model, tiny["cfg"], 9360, True)
    model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3)
    wr(lat[2].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680, kv_cache_only=only)
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    rc, _ = wr(lat[1].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680, kv_cache_only=only)
    model.block_mask = None
    if only:
        assert float(rc.float().abs().max()) == 0
    after_rc = _codes(kv)
    nxt, _ = wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    return nxt.cpu(), after_rc, _codes(kv)


def test_kv_cache_only_pass_commits_the_last_layers_codes(tiny, monkeypatch):
    from realtime_video_amd import _lib
    want = _recompute_then_denoise(tiny, *_model(tiny, "compact"), only=False)
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = _recompute_then_denoise(tiny, *_model(tiny, "codes", _cp(2)), only=True)
    monkeypatch.undo()
    assert "rtv_dit_commit_block_attn_fp8_only" in names, "the kv_only pass did not end with the commit-only call"
    assert torch.equal(got[0], want[0]) and _same_codes(got[1], want[1]) and _same_codes(got[2], want[2])


def test_rolling_cache_with_a_sink_under_two_shards(tiny):
    """The configuration of test_rolling_cache_under_two_shards (local_attn_size = 6, sink_size = 1, a cache of 6 x 1560 rows, one
    layer, four blocks) on compact dicts.  The commit places rows by the ring mapping, so the sharded cache rotates like the
    unsharded one - no shift copy - and equals it after every block: outputs, codes, ring_start."""
    wo, lat, ctx = tiny["wo"], tiny["lat"], tiny["ctx"]
    cfg = dict(tiny["cfg"], num_layers=1, local_attn_size=6, sink_size=1)
    w = wo.make_weights(cfg, seed=3, text_dim=tiny["text_dim"])
    rows = 6 * 1560
    got = {}
    for mode, cp in (("compact", None), ("codes", _cp(2))):
        model, wr = _model(tiny, mode, cp, cfg=cfg, w=w)
        kv, ca = _kv(model, cfg, rows, True)
        seq = []
        for b in range(4):
            flow, _ = wr(lat[b].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=b * M)
            seq.append((flow.cpu(), _codes(kv), int(kv[0].get("ring_start", 0))))
        got[mode] = (seq, model.fp8_attention_amax().clone())
    for b, (s, o) in enumerate(zip(got["compact"][0], got["codes"][0])):
        assert torch.equal(o[0], s[0]), f"output of block {b}"
        assert _same_codes(o[1], s[1]), f"codes behind block {b}"
        assert o[2] == s[2]
    assert got["codes"][0][3][2] == 1560 and got["codes"][0][2][2] == 4680          # the ring did rotate, and block 3's write wrapped
    assert torch.equal(got["codes"][1], got["compact"][1])


def test_kv_split_equals_the_shadow_modes_split(tiny):
    """attn_kv_splits = 2: the same split kernel on the same codes as the shadow mode's sharded run with two ranges."""
    model, wr = _model(tiny, "codes", _cp(2, splits=2))
    kv, ca = _kv(model, tiny["cfg"], 9360, True)
    outs, codes = _three_forwards(model, wr, tiny["lat"], tiny["ctx"], kv, ca)
    assert model._cfg.max_attn_kv_splits >= 2
    _assert_same_run((outs, codes, model.fp8_attention_amax().clone()), _run_three(tiny, "shadow", _cp(2, splits=2)), "shadow mode, two ranges")


def test_hip_graph_replay_equals_eager(tiny):
    """use_hip_graphs under two shards: replayed forwards equal eager ones bit for bit, nothing is allocated once the first block is
    over (the staging buffer is allocated once; captured graphs embed its address, and the graph key names it)."""
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    outs = {}
    for graphs in (False, True):
        model, wr = _model(tiny, "codes", _cp(2))
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
            kv8 = model._fp8_attention.staging(M, 2, torch.device(kv[0]["k8"].device))
            assert all(k[-1][0] == "only" and k[-1][-2:] == ("kv8", kv8.data_ptr()) for k in model._graphs), "the graph key does not name the staging buffer"
        outs[graphs] = (seq, _codes(kv))
    assert all(torch.equal(a, b) for a, b in zip(outs[False][0], outs[True][0])) and _same_codes(outs[False][1], outs[True][1])


def test_session_under_simulated_rows_equals_the_unsharded_compact_session(tiny, monkeypatch):
    """A GenerationSession over two blocks at 416 x 240 (390 tokens per frame, 585 rows a shard), the recompute pass included: latents
    and codes of the sharded session equal the unsharded compact session's, and the dicts hold no "k" / "v"."""
    from realtime_video_amd import _lib
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    text_dim, ctx = tiny["text_dim"], tiny["ctx"]
    g = torch.Generator().manual_seed(6)
    noise = torch.randn(1, 6, 16, 30, 52, generator=g).to(BF)
    padded = torch.zeros(1, 512, text_dim, dtype=BF)
    padded[0, :ctx.shape[0]] = ctx
    steps, real = [], _lib.call

    def spy(name, *args):
        if name.startswith("rtv_dit_forward") or name == "rtv_dit_begin":
            steps.append((name, args[2]._obj.causal_block, args[2]._obj.kv_only))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    latents = {}
    for mode, cp in (("compact", None), ("codes", _cp(2))):
        model, wr = _model(tiny, mode, cp)
        pipe = _pipeline(wr)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(padded.to(DEV)))
        sess = GenerationSession(GenerateParams(seed=9, num_blocks=2, num_denoising_steps=4, keep_first_frame=True, width=416, height=240),
                                 models, device=DEV)
        assert all("k" not in c and "v" not in c and "k8" in c for c in pipe.kv_cache1)
        assert pipe.kv_cache1[0]["k8"].shape[1] == model.num_heads          # full-head dicts under the row exchange
        sess.noise = noise.to(DEV)
        cpu_rnd = torch.Generator().manual_seed(9)
        sess._randn = lambda shape: torch.randn(*shape, generator=cpu_rnd, dtype=BF).to(DEV)
        del steps[:]
        blocks = [sess.generate_block().cpu() for _ in range(2)]
        names = {n for n, _, _ in steps}
        assert names == ({"rtv_dit_begin"} if cp is not None else {"rtv_dit_forward_attn_fp8_only"}), names
        assert any(cb > 0 for _, cb, _ in steps), "the session ran no recompute pass"
        assert all("k" not in c and "v" not in c for c in pipe.kv_cache1)
        latents[mode] = (blocks, sess.all_latents.cpu(), _codes(pipe.kv_cache1))
    for b in range(2):
        assert torch.equal(latents["codes"][0][b], latents["compact"][0][b]), b
    assert torch.equal(latents["codes"][1], latents["compact"][1]) and bool(torch.isfinite(latents["codes"][1].float()).all())
    assert _same_codes(latents["codes"][2], latents["compact"][2])


def test_python_refusals_leave_the_indices_alone(tiny):
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    model, wr = _model(tiny, "codes", _cp(2))
    kv, ca = _kv(model, cfg, 9360, True)
    wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    codes = _codes(kv)

    def refused(exc, match, caches, call=None):
        before = [(c["global_end_index"], c["local_end_index"]) for c in caches]
        with pytest.raises(exc, match=match):
            (call or (lambda: wr(lat[3].to(DEV), cond, T.to(DEV), caches, ca, current_start=4680)))()
        assert before == [(c["global_end_index"], c["local_end_index"]) for c in caches]

    model.context_parallel = _cp(2, "heads")                                                           # a head exchange
    refused(RuntimeError, r'ContextParallel\(exchange="rows"\)', kv)
    model.context_parallel = _cp(2, "auto")                                                            # ... and an "auto" that resolves to heads
    assert model.context_parallel.head_exchange(model.num_heads)
    refused(RuntimeError, r'ContextParallel\(exchange="rows"\)', kv)
    model.context_parallel = _cp(2)
    refused(RuntimeError, "needs the compact KV cache", _caches(cfg, 9360)[0])                         # "codes" mode with a bf16 dict
    refused(ValueError, "smooth_k", kv, lambda: model.enable_fp8_attention(bf16_cache=False, context_parallel="codes", smooth_k="codes"))
    refused(ValueError, "bf16_cache=False", kv, lambda: model.enable_fp8_attention(context_parallel="codes"))
    refused(RuntimeError, "context parallelism", kv, lambda: model.convert_kv_cache_to_fp8(_caches(cfg, 9360)[0]))
    model.enable_fp8_attention(context_parallel=True)                                                  # a compact dict under context_parallel=True
    refused(RuntimeError, "e4m3-only", kv)
    assert _same_codes(_codes(kv), codes), "a refused forward wrote into the cache"
    model.enable_fp8_attention(bf16_cache=False, context_parallel="codes")                             # back in the mode, the cache goes on
    wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    assert int(kv[0]["local_end_index"]) == 9360


def test_native_phases_refuse_before_any_launch(tiny, monkeypatch):
    """Behind the Python side: the three phases with the calls a real sharded forward has just issued, altered - a missing shadow or
    staging buffer, a misaligned one, a world that does not divide M, a window past cache_rows, bad scales and an unplanned split are
    errors that name the reason, and the codes stay as they were.  The step's kv_k / kv_v are null pointers."""
    from realtime_video_amd import _lib
    model, wr = _model(tiny, "codes", _cp(2))
    kv, ca = _kv(model, tiny["cfg"], 9360, True)
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
    assert not any(n in seen for n in ("rtv_dit_layer_rest", "rtv_dit_layer_proj", "rtv_dit_layer_rest_attn_fp8", "rtv_dit_forward_attn_fp8_only"))
    proj, rest, commit = (seen[n] for n in ("rtv_dit_layer_proj_attn_fp8_only", "rtv_dit_layer_rest_attn_fp8_only",
                                            "rtv_dit_commit_block_attn_fp8_only"))
    step = rest[2]._obj
    assert not step.kv_k and not step.kv_v and not commit[1]._obj.kv_k
    codes = _codes(kv)
    kv8_p = rest[5]
    off = type(kv8_p)(kv8_p.value + 8)
    # name, args, index of kv8, of the shadow, of world, of the layer (the commit-only call is the last layer's, of the second forward)
    calls = {"proj": ("rtv_dit_layer_proj_attn_fp8_only", proj, 6, 7, 5, 3), "rest": ("rtv_dit_layer_rest_attn_fp8_only", rest, 5, 6, 4, 3),
             "commit": ("rtv_dit_commit_block_attn_fp8_only", commit, 4, 5, 3, 2)}

    def refused(match, which, **alter):
        name, args, i_kv8, i_sh, i_w, _ = calls[which]
        a = list(args)
        for key, val in alter.items():
            a[{"kv8": i_kv8, "shadow": i_sh, "world": i_w}[key]] = val
        with pytest.raises(RuntimeError, match=match):
            real(name, *a)

    for which, (_, args, _, i_sh, _, i_l) in calls.items():
        shadow, layer = args[i_sh]._obj, args[i_l]
        refused("needs its staging buffer", which, kv8=None)
        refused("kv8 must be 16-byte aligned", which, kv8=off)
        refused("multiple of world", which, world=7)
        refused("multiple of world", which, world=0)
        refused("needs its shadow", which, shadow=None)
        shadow.k_scale = 0.0
        refused("scales must be finite and positive", which)
        shadow.k_scale, shadow.v_scale = 1.0, float("nan")
        refused("scales must be finite and positive", which)
        shadow.v_scale = 1.0
        k8_l = shadow.k8[layer]
        shadow.k8[layer] = None
        refused("a layer has no shadow", which)
        shadow.k8[layer] = k8_l + 8
        refused("16-byte aligned", which)
        shadow.k8[layer] = k8_l
    shadow = rest[6]._obj
    shadow.cache_rows = 4679                                 # the block's rows, and the attention window, end outside the cache
    refused(r"outside \[0, cache_rows\)", "rest")
    shadow.cache_rows = 9360
    shadow = commit[5]._obj
    shadow.cache_rows = commit[1]._obj.cache_row0 + M - 1
    refused(r"outside \[0, cache_rows\)", "commit")
    shadow.cache_rows = 9360
    step.attn_kv_splits = model._cfg.max_attn_kv_splits + 1
    refused("max_attn_kv_splits", "rest")
    step.attn_kv_splits = 1
    torch.cuda.synchronize()
    assert _same_codes(_codes(kv), codes), "a refused call wrote into the cache"


# ------------------------------------------------------------------------------------------------ two real processes
def _worker(rank, world, port, backend, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL between processes)
    torch.cuda.set_device(f"cuda:{rank}" if backend == "nccl" else "cuda:0")
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from oracle import wan_oracle as wo
        from realtime_video_amd.parallel import ContextParallel
        cfg, text_dim, tiny_inputs = _tiny()
        lat, ctx = tiny_inputs()
        t = dict(cfg=cfg, text_dim=text_dim, w=wo.make_weights(cfg, seed=0, text_dim=text_dim), lat=lat, ctx=ctx)
        outs, codes, amax = _run_three(t, "codes", ContextParallel(exchange="rows"))
        torch.cuda.synchronize()
        ret[rank] = (outs, [[(k.cpu(), v.cpu()) for k, v in per] for per in codes], amax.cpu())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_processes_equal_the_single_process_compact_run(tiny, backend):
    """Two ranks, the three forwards, no VAE.  gloo: both share cuda:0 and the all-gather of the codes is staged through the host;
    nccl: one GPU per rank over RCCL (needs two GPUs).  Every rank's outputs and codes equal the single-process compact run, and the
    elementwise maximum of the ranks' amax tables - a rank's table covers the rows it wrote - is that run's table."""
    world = 2
    if backend == "nccl" and torch.cuda.device_count() < world:
        pytest.skip(f"RCCL variant needs {world} GPUs, {torch.cuda.device_count()} visible")
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), backend, ret), nprocs=world, join=True)
    o_w, c_w, a_w = tiny["whole"]
    tables = []
    for rank in range(world):
        outs, codes, amax = ret[rank]
        for i in range(3):
            assert torch.equal(outs[i], o_w[i]), f"rank {rank}: output of forward {i}"
            assert all(torch.equal(k, wk.cpu()) and torch.equal(v, wv.cpu()) for (k, v), (wk, wv) in zip(codes[i], c_w[i])), \
                f"rank {rank}: codes behind forward {i}"
        assert bool((amax <= a_w.cpu()).all())
        tables.append(amax)
    assert torch.equal(torch.stack(tables).amax(0), a_w.cpu())
