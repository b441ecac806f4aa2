"""CausalWanModel.enable_fp8_attention(smooth_k=True) on the tiny model of tests/test_attn_fp8_model_gpu.py (its builders imported
unchanged): bit-identity with the plain mode until the first recentre; after fp8_attention_recenter the shadows hold the centred
codes of the bf16 caches and the forwards match the oracle whose self-attention is the centred restatement of
tests/attn_fp8_center_cases.py; the wrapped ring; no allocation across recentre + forward; hipGraph replay; the off path; the
refusals of the native entry point."""
import ctypes
import gc

import pytest
import torch

import attn_fp8_cases as fc
import attn_fp8_center_cases as cc
from conftest import rel_l2
from test_attn_fp8_model_gpu import T, T0, _shadow_matches_cache
from test_fp8_rows_gpu import _build, _caches, _on_dev, _three_forwards, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
TOL = 3e-2          # tests/test_attn_fp8_model_gpu.py: the plain mode against its oracle


class CentredOracle:
    """The oracle's attention functions with the fp8 restatement on k - centre as self-attention.  The oracle calls the
    self-attention of the layers in order, once per layer and forward: the call count gives the layer.  centers None: plain."""

    def __init__(self, num_layers):
        self.L, self.calls, self.centers = num_layers, 0, None

    def _center(self):
        l = self.calls % self.L
        self.calls += 1
        return None if self.centers is None else self.centers[l]

    def _attend(self, q, k, v, limits=None):
        c = self._center()
        if c is None:
            return fc.restated_attention(q, k, v, limits=limits)
        return cc.restated_attention_centered(q, k, v, c, limits=limits)

    def attn_fn(self, q, k, v):
        from oracle import wan_oracle as wo
        return wo.attention_sdpa(q, k, v) if k.shape[1] == 512 else self._attend(q, k, v)

    def block_causal(self, q, k, v, block_len):
        from oracle import wan_oracle as wo
        return self._attend(q, k, v, limits=wo.block_causal_limits(q.shape[1], block_len))


def _shadow_matches_centred_cache(kv, centers):
    """Every layer's shadow equals a whole-cache centred quantisation of its bf16 cache (the restatement), bit for bit."""
    for l, c in enumerate(kv):
        rows, H = c["k"].shape[1], c["k"].shape[2]
        k8, v8t = fc.empty_shadow(rows, H, device=DEV)
        cc.quantize_kv_centered(c["k"][0], c["v"][0], k8, v8t, 0, rows, centers[l])
        assert torch.equal(c["k8"], k8) and torch.equal(c["v8t"], v8t), l


@pytest.fixture(scope="module")
def tiny():
    from oracle import wan_oracle as wo
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    return dict(wo=wo, cfg=cfg, text_dim=text_dim, w=w, lat=lat, ctx=ctx)


def _spy_caches(model):
    seen = []
    orig = model._fp8_attention.shadow
    model._fp8_attention.shadow = lambda kv, use_cp: (seen.append(kv), orig(kv, use_cp))[1]
    return seen


def test_smooth_k_before_any_recentre_is_the_plain_mode(tiny):
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    runs = []
    for smooth in (False, True):
        model, wr = _build(cfg, tiny["text_dim"], w)
        model.enable_fp8_attention(smooth_k=smooth)
        seen = _spy_caches(model)
        outs = _three_forwards(model, wr, lat, ctx, T, T0)
        runs.append((outs, seen[-1], model))
    (plain, kv_p, _), (smooth, kv_s, m) = runs
    assert all(torch.equal(a, b) for a, b in zip(plain, smooth))
    for a, b in zip(kv_p, kv_s):
        assert torch.equal(a["k8"], b["k8"]) and torch.equal(a["v8t"], b["v8t"])
    assert m._fp8_attention.center.shape == (cfg["num_layers"], cfg["num_heads"], 128) and not bool(m._fp8_attention.center.any())
    assert runs[0][2]._fp8_attention.center is None, "the plain mode allocated a centre"
    assert torch.equal(runs[0][2].fp8_attention_amax(), m.fp8_attention_amax())
    _shadow_matches_cache(kv_s)


def test_recentred_forwards_against_the_centred_oracle(tiny, monkeypatch):
    """Denoise at offset 0, recentre, block-causal recompute, second-block denoise: each <= 3e-2 against the oracle with the centred
    restatement under the model's centres (read back from the device; any fixed centre is exact, so the oracle needs no means of
    its own), and after every forward the shadows are the centred codes of the bf16 caches."""
    wo, cfg, w, lat, ctx = tiny["wo"], tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    model, wr = _build(cfg, tiny["text_dim"], w)
    model.enable_fp8_attention(smooth_k=True)
    with pytest.raises(RuntimeError, match="has not run yet"):
        model.fp8_attention_recenter([])
    kv, ca = _caches(cfg, 9360)
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    a, _ = wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    assert model.fp8_attention_recenter(kv) is model
    centers = model._fp8_attention.center.cpu().to(DEV)
    for l, c in enumerate(kv):                        # the means of the rows written so far, within the mean kernel's bound
        want = c["k"][0, :4680].double().mean(0)
        assert bool(((centers[l].double() - want).abs() <= 4680 * 2.0 ** -24 * c["k"][0, :4680].double().abs().mean(0)).all()), l
    assert bool(centers.any())
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3)
    rc, _ = wr(lat[2].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680)
    model.block_mask = None
    _shadow_matches_centred_cache(kv, centers)
    b, _ = wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    _shadow_matches_centred_cache(kv, centers)
    assert torch.equal(model._fp8_attention.center, centers), "a forward wrote the centres"
    amax = model.fp8_attention_amax()
    assert bool((amax > 0).all()) and bool((amax < 448).all())

    orc = CentredOracle(cfg["num_layers"])
    monkeypatch.setattr(wo, "attention_block_causal", orc.block_causal)
    wd, ctx_d, lat_d = _on_dev(dict(w)), ctx.to(DEV), [x.to(DEV) for x in lat]
    sched = wo.FlowMatchScheduler()
    kvc = wo.initialize_kv_cache(cfg["num_layers"], 1, 9360, cfg["num_heads"], 128, BF, DEV)
    cac = wo.initialize_crossattn_cache(cfg["num_layers"], 1, cfg["num_heads"], 128, BF, device=DEV)
    ra, _ = wo.wrapper_forward(wd, cfg, sched, lat_d[0], [ctx_d], T.to(DEV), kvc, cac, 0, attn_fn=orc.attn_fn)
    orc.centers, orc.calls = centers, 0
    wo.reset_kv_cache(kvc)
    rrc, _ = wo.wrapper_forward(wd, cfg, sched, lat_d[2], [ctx_d], T0.to(DEV), kvc, cac, 4680, recompute=True, attn_fn=orc.attn_fn)
    rb, _ = wo.wrapper_forward(wd, cfg, sched, lat_d[3], [ctx_d], T.to(DEV), kvc, cac, 4680, attn_fn=orc.attn_fn)
    assert orc.calls == 2 * cfg["num_layers"]
    errs = [rel_l2(o, r) for o, r in zip((a, rc, b), (ra, rrc, rb))]
    print("smoothed fp8 attention vs centred oracle:", " ".join(f"{v:.3e}" for v in errs))
    assert all(v <= TOL for v in errs)


def test_smooth_k_on_a_wrapped_ring(tiny):
    """The ring of tests/test_attn_fp8_model_gpu.py (local_attn_size 6, sink 1, 6 x 1560 rows, four blocks; block 3 writes across the
    end of the ring) with a recentre behind block 0 and another behind block 2: every block <= 3e-2 against the oracle (whose cache
    is shifted, not rotated - a per-channel centre does not care) and the shadow is the centred code of the cache after every block."""
    wo, text_dim, lat, ctx = tiny["wo"], tiny["text_dim"], tiny["lat"], tiny["ctx"]
    cfg = dict(tiny["cfg"], num_layers=1, local_attn_size=6, sink_size=1)
    w = wo.make_weights(cfg, seed=3, text_dim=text_dim)
    model, wr = _build(cfg, text_dim, w)
    model.enable_fp8_attention(smooth_k=True)
    rows = 6 * 1560
    kv, ca = _caches(cfg, rows)
    kvc = wo.initialize_kv_cache(1, 1, rows, cfg["num_heads"], 128, BF, DEV)
    cac = wo.initialize_crossattn_cache(1, 1, cfg["num_heads"], 128, BF, device=DEV)
    wd, ctx_d = _on_dev(dict(w)), ctx.to(DEV)
    orc = CentredOracle(1)
    errs, shifts = [], []
    for b in range(4):
        ref, _ = wo.wrapper_forward(wd, cfg, wo.FlowMatchScheduler(), lat[b].to(DEV), [ctx_d], T.to(DEV), kvc, cac, b * 4680,
                                    attn_fn=orc.attn_fn)
        flow, _ = wr(lat[b].to(DEV), {"prompt_embeds": [ctx_d]}, T.to(DEV), kv, ca, current_start=b * 4680)
        errs.append(rel_l2(flow, ref))
        shifts.append(int(kv[0].get("ring_start", 0)))
        _shadow_matches_centred_cache(kv, model._fp8_attention.center)
        if b in (0, 2):
            model.fp8_attention_recenter(kv)
            orc.centers = model._fp8_attention.center.cpu().to(DEV)
            n = min(int(kv[0]["local_end_index"]), rows)
            assert n == (4680, 0, rows)[b]
            want = kv[0]["k"][0, :n].double().mean(0)
            assert float((orc.centers[0].double() - want).abs().max()) <= n * 2.0 ** -24 * float(kv[0]["k"][0, :n].double().abs().max())
    print("smoothed fp8 attention on the ring vs oracle:", " ".join(f"{v:.3e}" for v in errs), "ring_start", shifts)
    assert all(v <= TOL for v in errs)
    assert shifts[3] == 1560 and shifts[2] == 4680          # block 3 wrote two physical ranges through the centred quantiser


def test_recentre_allocates_nothing_and_graph_replay_equals_eager(tiny):
    """fill, recentre, then the same step three times (eager, capture, replay) with a second recentre between the capture and the
    replay: the graph holds the centre buffer's address, so the replay quantises under the new centre; outputs equal the eager
    model's bit for bit, and nothing is allocated across recentre + forward."""
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    outs, cents = {}, {}
    for graphs in (False, True):
        model, wr = _build(cfg, tiny["text_dim"], w)
        model.enable_fp8_attention(smooth_k=True)
        model.use_hip_graphs = graphs
        kv, ca = _caches(cfg, 9360)
        cond = {"prompt_embeds": [ctx.to(DEV)]}
        wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)            # fills the text caches, the shadows, the centres
        model.fp8_attention_recenter(kv)
        ptr = model._fp8_attention.center.data_ptr()
        lats = [x.to(DEV) for x in lat]
        tt = T.to(DEV)
        seq = []
        for rep in range(3):
            if rep == 2:
                gc.collect()
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                first = model._fp8_attention.center.clone().cpu()
                model.fp8_attention_recenter(kv)                                # rows [0, 9360) now: another centre, same buffer
                assert not torch.equal(model._fp8_attention.center.cpu(), first) and model._fp8_attention.center.data_ptr() == ptr
            for c in kv:
                c["global_end_index"] = c["local_end_index"] = 4680
            out, _ = wr(lats[1 + rep], cond, tt, kv, ca, current_start=4680)
            seq.append(out.cpu())
            del out
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, "recentre + forward allocated"
        if graphs:
            assert any(isinstance(e, dict) for e in model._graphs.values()), "no graph was captured"
        _shadow_matches_centred_cache(kv, model._fp8_attention.center)
        outs[graphs], cents[graphs] = seq, model._fp8_attention.center.cpu()
    assert torch.equal(cents[False], cents[True])
    assert all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))


def test_disable_restores_the_bf16_launches_and_reenabling_refills(tiny):
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    bf16_model, bf16_wr = _build(cfg, tiny["text_dim"], w)
    want = _three_forwards(bf16_model, bf16_wr, lat, ctx, T, T0)
    model, wr = _build(cfg, tiny["text_dim"], w)
    model.enable_fp8_attention(smooth_k=True)
    seen = _spy_caches(model)
    on = _three_forwards(model, wr, lat, ctx, T, T0)
    kv = seen[-1]
    model.fp8_attention_recenter(kv)
    assert model.disable_fp8_attention() is model
    back = _three_forwards(model, wr, lat, ctx, T, T0)
    assert all(torch.equal(a, b) for a, b in zip(back, want)) and not any(torch.equal(a, b) for a, b in zip(on, want))
    # back on: the centres are kept, and the stale shadows (wiped here, to see it) are refilled under them from the bf16 cache
    model.enable_fp8_attention(smooth_k=True)
    ca = _caches(cfg, 9360)[1]
    for c in kv:
        c["k8"].zero_()
        c["global_end_index"] = c["local_end_index"] = 4680
    wr(lat[3].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=4680)
    assert bool(model._fp8_attention.center.any())
    _shadow_matches_centred_cache(kv, model._fp8_attention.center)


def test_session_recentres_once_behind_its_first_block(tiny):
    """GenerationSession with a smooth_k model: one recentre behind block 0 (the first block that has filled the cache), none behind
    block 1, one more on request; the shadows follow the centres; a session without the mode refuses the request."""
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    cfg, text_dim, w, ctx = tiny["cfg"], tiny["text_dim"], tiny["w"], tiny["ctx"]
    model, wr = _build(cfg, text_dim, w)
    model.enable_fp8_attention(smooth_k=True)
    pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 750, 500, 250]),
                                   DEV, generator=wr, text_encoder=None, vae=None)
    padded = torch.zeros(1, 512, text_dim, dtype=BF)
    padded[0, :ctx.shape[0]] = ctx
    models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(padded.to(DEV)))
    sess = GenerationSession(GenerateParams(seed=9, num_blocks=2, num_denoising_steps=2, keep_first_frame=True), models, device=DEV)
    assert model._fp8_attention.center is None and not sess._fp8_recentered
    out0 = sess.generate_block()
    assert sess._fp8_recentered and model._fp8_attention.center_epoch == 1 and bool(model._fp8_attention.center.any())
    first = model._fp8_attention.center.clone()
    out1 = sess.generate_block()
    assert model._fp8_attention.center_epoch == 1 and torch.equal(model._fp8_attention.center, first), "the session recentred on its own again"
    assert bool(torch.isfinite(out0).all()) and bool(torch.isfinite(out1).all())
    _shadow_matches_centred_cache(pipe.kv_cache1, first)
    sess.fp8_attention_recenter()
    assert model._fp8_attention.center_epoch == 2 and not torch.equal(model._fp8_attention.center, first)
    model.enable_fp8_attention()
    with pytest.raises(RuntimeError, match="smooth_k=True"):
        sess.fp8_attention_recenter()


def test_native_centred_forward_refusals(tiny, monkeypatch):
    """rtv_dit_forward_attn_fp8_centered refuses what rtv_dit_forward_attn_fp8 refuses, with the same messages, and a missing centre
    table or entry - before any launch.  The step is the one a real smoothed forward has just issued, altered."""
    from realtime_video_amd import _lib
    cfg, w, lat, ctx = tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    model, wr = _build(cfg, tiny["text_dim"], w)
    model.enable_fp8_attention(smooth_k=True)
    kv, ca = _caches(cfg, 9360)
    seen, real = [], _lib.call

    def spy(name, *args):
        if name.startswith("rtv_dit_forward"):
            seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    wr(lat[0].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=0)
    monkeypatch.undo()
    assert [n for n, _ in seen] == ["rtv_dit_forward_attn_fp8_centered"]
    name, args = seen[0]
    torch.cuda.synchronize()
    k8_before = [c["k8"].clone() for c in kv]
    step = args[2]._obj
    step.row_count = 2340
    with pytest.raises(RuntimeError, match="fp8 attention does not support sharded calls"):
        real(name, *args)
    step.row_begin, step.row_count = 2340, 0
    with pytest.raises(RuntimeError, match="fp8 attention does not support sharded calls"):
        real(name, *args)
    step.row_begin, step.attn_kv_splits = 0, 2
    with pytest.raises(RuntimeError, match="fp8 attention does not support attn_kv_splits"):
        real(name, *args)
    step.attn_kv_splits = 1
    with pytest.raises(RuntimeError, match="needs its shadow"):
        real(name, *args[:3], None, *args[4:])
    with pytest.raises(RuntimeError, match="needs its table of K centres"):
        real(name, *args[:4], None, *args[5:])
    holes = (ctypes.c_void_p * cfg["num_layers"])(*[model._fp8_attention.center[l].data_ptr() for l in range(cfg["num_layers"])])
    holes[cfg["num_layers"] - 1] = None
    with pytest.raises(RuntimeError, match="a layer has no K centre"):
        real(name, *args[:4], holes, *args[5:])
    torch.cuda.synchronize()
    assert all(torch.equal(a, c["k8"]) for a, c in zip(k8_before, kv)), "a refused call launched"
