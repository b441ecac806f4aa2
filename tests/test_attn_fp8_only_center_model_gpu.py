"""CausalWanModel.enable_fp8_attention(bf16_cache=False, smooth_k="codes"): K smoothing on the e4m3-only KV cache
(include/rtv_hip_attn_fp8_only_center.h) on the tiny model of tests/test_attn_fp8_only_model_gpu.py (its helpers imported
unchanged).  Under given centres the mode equals the shadow mode under smooth_k=True bit for bit; a recentre moves the cached codes
as tests/attn_fp8_only_center_cases.py restates it; a live bf16 cache converts into a compact one; and what is refused."""
import ctypes
import gc
import os
import weakref

import pytest
import torch

import attn_fp8_cases as fc
import attn_fp8_only_center_cases as oc
from conftest import rel_l2
from test_attn_fp8_center_model_gpu import TOL, CentredOracle
from test_attn_fp8_only_center_gpu import PROFILE
from test_attn_fp8_only_model_gpu import T, T0, _codes, _kv, _pipeline, _same_codes, _three_forwards
from test_fp8_rows_gpu import _build, _caches, _on_dev, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def tiny():
    from oracle import wan_oracle as wo
    cfg, text_dim, tiny_inputs = _tiny()
    w = wo.make_weights(cfg, seed=0, text_dim=text_dim)
    lat, ctx = tiny_inputs()
    return dict(wo=wo, cfg=cfg, text_dim=text_dim, w=w, lat=lat, ctx=ctx)


def _model(tiny, mode, cfg=None, w=None, scales=(1.0, 1.0)):
    """mode: "codes" (compact cache, centred), "only" (compact, plain), "smooth" (shadow mode, smooth_k=True), "shadow" (plain)."""
    model, wr = _build(cfg or tiny["cfg"], tiny["text_dim"], w or tiny["w"])
    model.enable_fp8_attention(*scales, bf16_cache=mode not in ("codes", "only"), smooth_k={"codes": "codes", "smooth": True}.get(mode, False))
    return model, wr


def _given_centres(L, H, seed=1):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(L, H, 128, generator=g)
    c[:, :, ::8] += 4.0 * torch.where(torch.rand(L, H, 16, generator=g) < 0.5, -1.0, 1.0)
    return c.to(DEV)


def _same_written(a, b, n):
    """_same_codes on the rows written so far: the shadow mode fills the rows no forward has written yet with the codes of 0 - c,
    the compact cache leaves them zero; neither is ever read."""
    return all(torch.equal(x[0][:n], y[0][:n]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def _allocated():
    """torch.cuda.memory_allocated() with no garbage left and no work in flight.  What it counts for a tensor is the size of the
    block the tensor got: a request above 1 MiB that is served from a cached block takes the whole block when less than 1 MiB of
    it would remain, so the figure for a large tensor depends on what earlier tests left in the cache.  Tests that need exact bytes
    read the figure around the allocation as well."""
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated()


def _block_mask(model, on):
    model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3) if on else None


def test_codes_before_any_recentre_is_the_plain_compact_mode(tiny):
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    got = {}
    for mode in ("only", "codes"):
        model, wr = _model(tiny, mode)
        kv, ca = _kv(model, cfg, 9360, True)
        outs, codes = _three_forwards(model, wr, lat, ctx, kv, ca)
        got[mode] = (outs, codes, model.fp8_attention_amax().clone(), model, kv)
    (o_p, c_p, a_p, m_p, _), (o_c, c_c, a_c, m_c, kv_c) = got["only"], got["codes"]
    for i in range(3):
        assert torch.equal(o_c[i], o_p[i]), f"output of forward {i}"
        assert _same_codes(c_c[i], c_p[i]), f"codes behind forward {i}"
    assert torch.equal(a_c, a_p)
    shape = (cfg["num_layers"], cfg["num_heads"], 128)
    assert m_c._fp8_attention.center.shape == shape and m_c._fp8_attention.center_new.shape == shape
    assert not bool(m_c._fp8_attention.center.any()) and not bool(m_c._fp8_attention.center_new.any())
    assert m_c._fp8_attention.center_ws.numel() * 4 >= 37 * cfg["num_heads"] * 512
    assert m_p._fp8_attention.center is None, "the plain compact mode allocated a centre"
    assert all(c["fp8_center"] == m_c._fp8_attention.center_stamp() for c in kv_c)


def _sequence(tiny, model, wr, kv, ca, lat):
    """The three forwards of the sibling tests and, behind them, a kv_cache_only pass over the second block."""
    outs, codes = _three_forwards(model, wr, lat, tiny["ctx"], kv, ca)
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 4680
    z, _ = wr(lat[1].to(DEV), {"prompt_embeds": [tiny["ctx"].to(DEV)]}, T.to(DEV), kv, ca, current_start=4680, kv_cache_only=True)
    return outs + [z.cpu()], codes + [_codes(kv)]


def test_given_centres_equal_the_shadow_mode_under_the_same_centres(tiny):
    cfg, lat = tiny["cfg"], tiny["lat"]
    centres = _given_centres(cfg["num_layers"], cfg["num_heads"])
    got = {}
    for mode in ("smooth", "codes"):
        model, wr = _model(tiny, mode)
        kv, ca = _kv(model, cfg, 9360, mode == "codes")
        assert model.fp8_attention_set_centers(centres, kv if mode == "codes" else None) is model
        assert torch.equal(model._fp8_attention.center, centres) and model._fp8_attention.center.data_ptr() != centres.data_ptr()
        got[mode] = _sequence(tiny, model, wr, kv, ca, lat) + (model.fp8_attention_amax().clone(),)
    (o_s, c_s, a_s), (o_c, c_c, a_c) = got["smooth"], got["codes"]
    for i in range(4):
        assert torch.equal(o_c[i], o_s[i]), f"output of forward {i}"
        # (the recompute pass starts over at row 0: behind it the rows from 4680 on are still unwritten)
        assert _same_written(c_c[i], c_s[i], 4680 if i < 2 else 9360), f"codes behind forward {i}"
    assert torch.equal(a_c, a_s) and bool((a_c > 0).all())
    assert not bool(o_c[3].any()) and not _same_codes(c_c[3], c_c[2])      # the kv_cache_only pass: zeros out, rows written


def test_given_centres_on_a_wrapped_ring(tiny):
    """The ring of tests/test_attn_fp8_only_model_gpu.py: block 3 writes across the end of the ring."""
    wo, lat, ctx = tiny["wo"], tiny["lat"], tiny["ctx"]
    cfg = dict(tiny["cfg"], num_layers=1, local_attn_size=6, sink_size=1)
    w = wo.make_weights(cfg, seed=3, text_dim=tiny["text_dim"])
    centres = _given_centres(1, cfg["num_heads"], seed=2)
    rows = 6 * 1560
    got = {}
    for mode in ("smooth", "codes"):
        model, wr = _model(tiny, mode, cfg=cfg, w=w)
        kv, ca = _kv(model, cfg, rows, mode == "codes")
        model.fp8_attention_set_centers(centres)
        seq = []
        for b in range(4):
            flow, _ = wr(lat[b].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=b * 4680)
            seq.append((flow.cpu(), _codes(kv), int(kv[0].get("ring_start", 0))))
        got[mode] = (seq, model.fp8_attention_amax().clone())
    for b, (s, o) in enumerate(zip(got["smooth"][0], got["codes"][0])):
        assert torch.equal(o[0], s[0]), f"output of block {b}"
        assert _same_written(o[1], s[1], min((b + 1) * 4680, rows)), f"codes behind block {b}"
        assert o[2] == s[2]
    assert got["codes"][0][3][2] == 1560 and got["codes"][0][2][2] == 4680
    assert torch.equal(got["codes"][1], got["smooth"][1])


def test_recentre_moves_the_cached_codes_and_the_next_forwards_hold_the_bound(tiny, monkeypatch):
    """Denoise at offset 0, recentre, block-causal recompute, second-block denoise.  The recentre: every layer's k8 is the restatement
    applied to the codes from before, the centres are the means of the dequantised codes within the mean kernel's bound, nothing is
    allocated.  The forwards: each <= the bound tests/test_attn_fp8_center_model_gpu.py applies to the recentred shadow mode, against
    the oracle with the centred restatement under the model's centres."""
    wo, cfg, w, lat, ctx = tiny["wo"], tiny["cfg"], tiny["w"], tiny["lat"], tiny["ctx"]
    model, wr = _model(tiny, "codes")
    kv, ca = _kv(model, cfg, 9360, True)
    with pytest.raises(RuntimeError, match="has not run yet"):
        model.fp8_attention_recenter(kv)
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    a, _ = wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    before = _codes(kv)
    amax0 = model.fp8_attention_amax().clone()
    ptrs = (model._fp8_attention.center.data_ptr(), model._fp8_attention.center_new.data_ptr())
    mem = _allocated()
    assert model.fp8_attention_recenter(kv) is model
    assert _allocated() == mem, "the recentre allocated"
    assert ptrs == (model._fp8_attention.center.data_ptr(), model._fp8_attention.center_new.data_ptr())
    centres = model._fp8_attention.center.clone()
    zero = torch.zeros_like(centres[0])
    for l, c in enumerate(kv):
        old = before[l][0]
        x = oc.dequantized(old[:4680], 1.0).double()
        want = x.mean(0)
        bound = 4680 * 2.0 ** -24 * x.abs().mean(0) + 2.0 ** -23 * want.abs()
        assert bool(((centres[l].double() - want).abs() <= bound).all()), l
        moved, t = oc.recentered(old[:4680], zero, centres[l], 1.0)
        assert torch.equal(c["k8"][:4680], moved), l
        assert torch.equal(c["k8"][4680:], old[4680:]) and torch.equal(c["v8t"], before[l][1]), l
        assert float(model.fp8_attention_amax()[l, 0]) == max(float(amax0[l, 0]), float(t.abs().max()))
        assert c["fp8_center"] == model._fp8_attention.center_stamp()
    assert bool(centres.any())

    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    _block_mask(model, True)
    rc, _ = wr(lat[2].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680)
    _block_mask(model, False)
    b, _ = wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    assert torch.equal(model._fp8_attention.center, centres), "a forward wrote the centres"

    orc = CentredOracle(cfg["num_layers"])
    monkeypatch.setattr(wo, "attention_block_causal", orc.block_causal)
    wd, ctx_d, lat_d = _on_dev(dict(w)), ctx.to(DEV), [x.to(DEV) for x in lat]
    sched = wo.FlowMatchScheduler()
    kvc = wo.initialize_kv_cache(cfg["num_layers"], 1, 9360, cfg["num_heads"], 128, BF, DEV)
    cac = wo.initialize_crossattn_cache(cfg["num_layers"], 1, cfg["num_heads"], 128, BF, device=DEV)
    ra, _ = wo.wrapper_forward(wd, cfg, sched, lat_d[0], [ctx_d], T.to(DEV), kvc, cac, 0, attn_fn=orc.attn_fn)
    orc.centers, orc.calls = centres, 0
    wo.reset_kv_cache(kvc)
    rrc, _ = wo.wrapper_forward(wd, cfg, sched, lat_d[2], [ctx_d], T0.to(DEV), kvc, cac, 4680, recompute=True, attn_fn=orc.attn_fn)
    rb, _ = wo.wrapper_forward(wd, cfg, sched, lat_d[3], [ctx_d], T.to(DEV), kvc, cac, 4680, attn_fn=orc.attn_fn)
    errs = [rel_l2(o, r) for o, r in zip((a, rc, b), (ra, rrc, rb))]
    line = "ATTN_FP8_ONLY_CENTER recentred compact mode vs centred oracle (denoise, recompute, denoise): " + " ".join(f"{v:.3e}" for v in errs)
    print(line)
    if os.environ.get("RTV_PROFILE_DIR"):      # behind the kernel figures tests/test_attn_fp8_only_center_gpu.py has written
        with open(os.path.join(os.environ["RTV_PROFILE_DIR"], PROFILE), "a") as f:
            f.write(line + "\n")
    assert all(v <= TOL for v in errs)


def test_recentre_allocates_nothing_and_graph_replay_equals_eager(tiny):
    """fill, recentre, then the same step three times (eager, capture, replay) with a second recentre between the capture and the
    replay: the graph holds the centre buffer's address; outputs, codes and centres equal the eager model's bit for bit."""
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    outs = {}
    for graphs in (False, True):
        model, wr = _model(tiny, "codes")
        model.use_hip_graphs = graphs
        kv, ca = _kv(model, cfg, 9360, True)
        cond = {"prompt_embeds": [ctx.to(DEV)]}
        wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
        model.fp8_attention_recenter(kv)
        ptr = model._fp8_attention.center.data_ptr()
        lats, tt, seq = [x.to(DEV) for x in lat], T.to(DEV), []
        for rep in range(3):
            if rep == 2:
                before = _allocated()
                first = model._fp8_attention.center.clone().cpu()
                model.fp8_attention_recenter(kv)                                # rows [0, 9360) now
                assert not torch.equal(model._fp8_attention.center.cpu(), first) and model._fp8_attention.center.data_ptr() == ptr
                del first
            for c in kv:
                c["global_end_index"] = c["local_end_index"] = 4680
            out, _ = wr(lats[1 + rep], cond, tt, kv, ca, current_start=4680)
            seq.append(out.cpu())
            del out
        assert _allocated() == before, "recentre + forward allocated"
        if graphs:
            assert any(isinstance(e, dict) for e in model._graphs.values()), "no graph was captured"
            assert all(k[-1][:2] == ("only", "codes") for k in model._graphs), "the graph key does not carry the mode"
        outs[graphs] = (seq, _codes(kv), model._fp8_attention.center.cpu())
    assert torch.equal(outs[False][2], outs[True][2])
    assert all(torch.equal(a, b) for a, b in zip(outs[False][0], outs[True][0])) and _same_codes(outs[False][1], outs[True][1])


def test_session_equals_a_shadow_mode_session_under_the_same_centres(tiny):
    """A three-block GenerationSession on the compact cache recentres once, behind block 1; a shadow-mode smooth_k=True session whose
    recentre installs the first session's centres instead computes the same three blocks, bit for bit: the cache is recomputed at
    the start of every block, so only rows written under the new centres are read behind the recentre."""
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    text_dim, ctx = tiny["text_dim"], tiny["ctx"]
    noise = torch.randn(1, 9, 16, 30, 52, generator=torch.Generator().manual_seed(6)).to(BF)
    padded = torch.zeros(1, 512, text_dim, dtype=BF)
    padded[0, :ctx.shape[0]] = ctx
    latents, centres = {}, None
    for mode in ("codes", "smooth"):
        model, wr = _model(tiny, mode)
        recentres = []
        if mode == "codes":
            real = model.fp8_attention_recenter
            model.fp8_attention_recenter = lambda kv, real=real: (recentres.append(1), real(kv))[1]
        else:
            model.fp8_attention_recenter = lambda kv, model=model: (recentres.append(1), model.fp8_attention_set_centers(centres))[1]
        pipe = _pipeline(wr)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(padded.to(DEV)))
        sess = GenerationSession(GenerateParams(seed=9, num_blocks=3, num_denoising_steps=4, keep_first_frame=True, width=416, height=240),
                                 models, device=DEV)
        assert ("k" in pipe.kv_cache1[0]) == (mode == "smooth")
        sess.noise = noise.to(DEV)
        cpu_rnd = torch.Generator().manual_seed(9)
        sess._randn = lambda shape: torch.randn(*shape, generator=cpu_rnd, dtype=BF).to(DEV)
        blocks = []
        for b in range(3):
            blocks.append(sess.generate_block().cpu())
            assert len(recentres) == 1, (mode, b)
        if mode == "codes":
            centres = model._fp8_attention.center.clone()
            assert bool(centres.any()) and model._fp8_attention.center_epoch >= 1
        else:
            assert torch.equal(model._fp8_attention.center, centres)
        latents[mode] = (blocks, sess.all_latents.cpu())
    for b in range(3):
        assert torch.equal(latents["codes"][0][b], latents["smooth"][0][b]), b
    assert torch.equal(latents["codes"][1], latents["smooth"][1]) and bool(torch.isfinite(latents["codes"][1].float()).all())


def _stream(tiny, model, wr, kv, ca, recentre):
    """Three forwards of a stream: denoise at 0, (recentre,) block-causal recompute, second-block denoise."""
    lat, cond = tiny["lat"], {"prompt_embeds": [tiny["ctx"].to(DEV)]}
    wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    if recentre:
        model.fp8_attention_recenter(kv)
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    _block_mask(model, True)
    wr(lat[2].to(DEV), cond, T0.to(DEV), kv, ca, current_start=4680)
    _block_mask(model, False)
    wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)


def _fourth(tiny, wr, kv, ca):
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 4680
    return wr(tiny["lat"][1].to(DEV), {"prompt_embeds": [tiny["ctx"].to(DEV)]}, T.to(DEV), kv, ca, current_start=4680)[0].cpu()


@pytest.mark.parametrize("centred", [False, True], ids=["plain", "centred"])
def test_conversion_of_a_live_cache_takes_the_current_shadow_over(tiny, centred, monkeypatch):
    """Two identical shadow-mode streams of three forwards; one goes on in the shadow mode, the other converts its cache and goes on
    in the compact mode: the fourth forwards, the codes and the maxima are equal.  The current shadow is taken over as it is - no
    quantiser call, the same tensors -, and the allocation falls by exactly the bf16 bytes: what the allocator counted for the K and V
    tensors when they were made (their size, plus under 1 MiB each where a cached block larger than the request served them)."""
    from realtime_video_amd import ops
    cfg = tiny["cfg"]
    mode, to = ("smooth", "codes") if centred else ("shadow", False)
    runs = []
    for convert in (False, True):
        kv = ca = None      # (the caches of the round before go here, not inside the bracket below)
        model, wr = _model(tiny, mode)
        empty = _allocated()
        kv, ca = _caches(cfg, 9360)
        # (the text caches are below 1 MiB each: counted at their size)
        held = _allocated() - empty - sum(c["k"].numel() * 2 + c["v"].numel() * 2 for c in ca)
        _stream(tiny, model, wr, kv, ca, centred)
        if convert:
            model.enable_fp8_attention(bf16_cache=False, smooth_k=to)
            k8_ptrs = [(c["k8"].data_ptr(), c["v8t"].data_ptr()) for c in kv]
            bf16_bytes = sum(c["k"].numel() * 2 + c["v"].numel() * 2 for c in kv)
            assert bf16_bytes <= held < bf16_bytes + 2 * len(kv) * 2 ** 20, (held, bf16_bytes)
            calls = []
            monkeypatch.setattr(ops, "attn_quantize_kv", lambda *a, **k: calls.append(a))
            before = _allocated()
            assert model.convert_kv_cache_to_fp8(kv) is kv
            # (the centred mode makes its second centre buffer here, L x H x 512 bytes: below 1 MiB, counted at its size)
            assert before - _allocated() == held - (model._fp8_attention.center_new.numel() * 4 if centred else 0)
            monkeypatch.undo()
            assert not calls and k8_ptrs == [(c["k8"].data_ptr(), c["v8t"].data_ptr()) for c in kv]
            assert all("k" not in c and "v" not in c and "fp8_filled" not in c and c["rows"] == 9360 for c in kv)
            assert all(c["fp8_scales"] == (1.0, 1.0) and c["fp8_center"] == model._fp8_attention.center_stamp() for c in kv)
        runs.append((_fourth(tiny, wr, kv, ca), _codes(kv), model.fp8_attention_amax().clone(), int(kv[0]["local_end_index"])))
    (o_s, c_s, a_s, n_s), (o_c, c_c, a_c, n_c) = runs
    assert torch.equal(o_c, o_s) and _same_codes(c_c, c_s) and torch.equal(a_c, a_s) and n_c == n_s == 9360
    assert bool(torch.isfinite(o_c).all())


@pytest.mark.parametrize("centred", [False, True], ids=["plain", "centred"])
def test_conversion_of_a_cache_that_never_had_a_shadow(tiny, centred):
    """A bf16 stream (no fp8 attention) converts as well: one quantiser call per layer codes the whole cache, centred when the mode
    is; the next forward equals that of a model which switches the same stream to the shadow mode instead."""
    cfg = tiny["cfg"]
    centres = _given_centres(cfg["num_layers"], cfg["num_heads"], seed=4)
    runs = []
    for convert in (False, True):
        model, wr = _build(cfg, tiny["text_dim"], tiny["w"])
        kv, ca = _caches(cfg, 9360)
        _stream(tiny, model, wr, kv, ca, False)
        assert "k8" not in kv[0]
        if convert:
            model.enable_fp8_attention(bf16_cache=False, smooth_k="codes" if centred else False)
            if centred:
                model.fp8_attention_set_centers(centres)
            k = [c["k"][0].clone() for c in kv]
            model.convert_kv_cache_to_fp8(kv)
            for l, c in enumerate(kv):
                want = fc.codes(k[l].float() - centres[l], 1.0) if centred else fc.codes(k[l], 1.0)
                assert torch.equal(c["k8"], want), l
        else:
            model.enable_fp8_attention(smooth_k=centred)
            if centred:
                model.fp8_attention_set_centers(centres)
        runs.append((_fourth(tiny, wr, kv, ca), _codes(kv)))
    assert torch.equal(runs[0][0], runs[1][0]) and _same_codes(runs[0][1], runs[1][1])


def test_pipeline_converts_its_cache_and_frees_the_arena(tiny):
    cfg = tiny["cfg"]
    L, H = cfg["num_layers"], cfg["num_heads"]
    model, wr = _build(dict(cfg, local_attn_size=6), tiny["text_dim"], tiny["w"])
    pipe = _pipeline(wr)
    pipe._initialize_kv_cache(1, BF, DEV)
    rows = 6 * 1560
    assert "k" in pipe.kv_cache1[0] and pipe.kv_cache1[0]["k"].shape[1] == rows
    with pytest.raises(RuntimeError, match="bf16_cache=False"):
        pipe.convert_kv_cache_to_fp8()
    model.enable_fp8_attention(bf16_cache=False, smooth_k="codes")
    arena = weakref.ref(pipe._kv_arena)
    assert arena().numel() * 2 == L * 2 * rows * H * 128 * 2
    kv = pipe.convert_kv_cache_to_fp8()
    gc.collect()
    assert kv is pipe.kv_cache1 and pipe._kv_arena is None and all("k" not in c and "v" not in c and c["rows"] == rows for c in kv)
    assert arena() is None, "something still holds the bf16 arena"
    assert all(c["k8"].shape == (rows, H, 128) and c["fp8_center"] == model._fp8_attention.center_stamp() for c in kv)
    ptrs = [c["k8"].data_ptr() for c in kv]
    pipe._initialize_kv_cache(1, BF, DEV)                                        # a reset keeps the converted dicts
    assert pipe.kv_cache1 is kv and ptrs == [c["k8"].data_ptr() for c in kv]


def test_python_refusals_leave_the_indices_alone(tiny):
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    model, wr = _model(tiny, "codes")
    kv, ca = _kv(model, cfg, 9360, True)
    other = model.new_fp8_kv_cache(9360, DEV)
    wr(lat[0].to(DEV), cond, T.to(DEV), kv, ca, current_start=0)
    wr(lat[0].to(DEV), cond, T.to(DEV), other, ca, current_start=0)
    model.fp8_attention_recenter(kv)                       # moves the rows of `kv`; `other` stays under the centres of before
    codes = _codes(other)

    def refused(exc, match, caches, call=None):
        before = [(c["global_end_index"], c["local_end_index"]) for c in caches]
        with pytest.raises(exc, match=match):
            (call or (lambda: wr(lat[3].to(DEV), cond, T.to(DEV), caches, ca, current_start=4680)))()
        assert before == [(c["global_end_index"], c["local_end_index"]) for c in caches]

    refused(RuntimeError, "other K centres", other)
    refused(RuntimeError, "other K centres", other, lambda: model.fp8_attention_recenter(other))
    refused(RuntimeError, "other K centres", other, lambda: model.fp8_attention_set_centers(model._fp8_attention.center.clone(), other))
    refused(ValueError, "heads", kv, lambda: model.fp8_attention_set_centers(torch.zeros(cfg["num_layers"], 1, 128, device=DEV)))
    refused(ValueError, r"\[num_layers, H, 128\]", kv, lambda: model.fp8_attention_set_centers(model._fp8_attention.center.double()))
    refused(ValueError, "compact one already", kv, lambda: model.convert_kv_cache_to_fp8(kv))
    refused(ValueError, 'smooth_k="codes"', kv, lambda: model.enable_fp8_attention(smooth_k=True, bf16_cache=False))
    refused(ValueError, "bf16_cache=False", kv, lambda: model.enable_fp8_attention(smooth_k="codes"))
    model.enable_fp8_attention(bf16_cache=False)           # the plain compact mode finds rows coded under centres
    refused(RuntimeError, "other K centres", kv)
    refused(RuntimeError, "smooth_k", kv, lambda: model.fp8_attention_recenter(kv))
    torch.cuda.synchronize()
    assert _same_codes(_codes(other), codes), "a refused call wrote into the cache"
    # back in the mode the stream goes on; `other` after a reset as well
    model.enable_fp8_attention(bf16_cache=False, smooth_k="codes")
    wr(lat[3].to(DEV), cond, T.to(DEV), kv, ca, current_start=4680)
    assert int(kv[0]["local_end_index"]) == 9360
    for c in other:
        c["global_end_index"] = c["local_end_index"] = 0
    wr(lat[0].to(DEV), cond, T.to(DEV), other, ca, current_start=0)
    assert int(other[0]["local_end_index"]) == 4680 and other[0]["fp8_center"] == model._fp8_attention.center_stamp()


def test_native_forward_refusals(tiny, monkeypatch):
    """rtv_dit_forward_attn_fp8_only_centered with the step a real forward has just issued, altered: what either parent refuses is
    refused with its message before any launch - the codes stay as they were."""
    from realtime_video_amd import _lib
    cfg, lat, ctx = tiny["cfg"], tiny["lat"], tiny["ctx"]
    L = cfg["num_layers"]
    model, wr = _model(tiny, "codes")
    kv, ca = _kv(model, cfg, 9360, True)
    seen, real = [], _lib.call

    def spy(name, *args):
        if name.startswith("rtv_dit_forward"):
            seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    wr(lat[0].to(DEV), {"prompt_embeds": [ctx.to(DEV)]}, T.to(DEV), kv, ca, current_start=0)
    monkeypatch.undo()
    assert [n for n, _ in seen] == ["rtv_dit_forward_attn_fp8_only_centered"]
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
    step.row_count, step.attn_kv_splits = 0, 2
    refused("fp8 attention does not support attn_kv_splits")
    step.attn_kv_splits = 1
    refused("needs its shadow", *args[:3], None, *args[4:])
    refused("needs its table of K centres", *args[:4], None, *args[5:])
    table = lambda: (ctypes.c_void_p * L)(*[model._fp8_attention.center[l].data_ptr() for l in range(L)])
    holes = table()
    holes[L - 1] = None
    refused("a layer has no K centre", *args[:4], holes, *args[5:])
    odd = table()
    odd[L - 1] = model._fp8_attention.center[L - 1].data_ptr() + 4
    refused("16-byte aligned", *args[:4], odd, *args[5:])
    shadow.cache_rows = 0
    refused("needs the k8 / v8t shadow arrays and cache_rows")
    shadow.cache_rows = 4679
    refused(r"outside \[0, cache_rows\)")
    shadow.cache_rows, shadow.k_scale = 9360, 0.0
    refused("scales must be finite and positive")
    shadow.k_scale = 1.0
    k8_0 = shadow.k8[0]
    shadow.k8[0] = None
    refused("a layer has no shadow")
    shadow.k8[0] = k8_0
    torch.cuda.synchronize()
    assert _same_codes(_codes(kv), codes), "a refused call wrote into the cache"
    for c in kv:
        c["global_end_index"] = c["local_end_index"] = 0
    real(name, *args)                                        # the unaltered call runs
