"""GPU tests of the TAEHV tiny-VAE encoder (csrc/taehv.hip behind realtime_video_amd/taehv.py TAEHVEncoder): every new
convolution form of rtv_taehv_enc_conv against torch fp32 conv2d, the streamed encode against the reference's goldens,
bit-identical results however a stream is split into calls, the production size against the CPU-pinned restatement
(tests/test_taehv_encoder_cpu.py) evaluated on the GPU, the time contract's errors, the two live streams on one instance
(a dropped stream's arena is recycled), the session's encode sites and a frame-count round trip through the TAEHV decoder."""
import gc

import pytest
import torch
import torch.nn.functional as F

from conftest import max_abs, rel_l2
from test_taehv_encoder_cpu import golden_frames, restate_encode
from test_taehv_gpu import _ptr, lib_call

DEV = "cuda"
pytestmark = pytest.mark.gpu


def _enc_conv(x, w, bias, out, form, T, H, W, kt, n_total, n0):
    zeros = torch.zeros(64, dtype=torch.float16, device=DEV)
    lib_call("rtv_taehv_enc_conv", _ptr(x), _ptr(w), _ptr(bias), _ptr(out), form, T, H, W, kt, n_total, n0, _ptr(zeros))


def _check(name, got, ref):
    assert not torch.isnan(got).any()
    err, mx = rel_l2(got, ref), max_abs(got, ref)
    print(f"{name}: rel-L2 {err:.2e} max-abs {mx:.2e}")
    assert err <= 2e-3 and mx <= 2e-2 * max(1.0, float(ref.abs().max()))


def test_first_layer_matches_torch():
    """conv 3 -> 64 + bias, ReLU on 0.5 * x + 0.5 with a zero border in [0, 1] space; frames 1..3 of a 5-frame planar clip."""
    g = torch.Generator().manual_seed(0)
    Tt, t0, T, H, W = 5, 1, 3, 26, 42            # 3276 pixels: partial 128-pixel block and partial 32-pixel wave tile
    x16 = (torch.rand(3, Tt, H, W, generator=g) * 2 - 1).half()
    w16 = (torch.randn(64, 3, 3, 3, generator=g) * (2 / 27) ** 0.5).half()
    b16 = (torch.randn(64, generator=g) * 0.1).half()
    x01 = (0.5 * x16.float() + 0.5).half().float()          # the kernel rounds the mapped pixel to fp16 for the MFMA
    ref = F.relu(F.conv2d(x01[:, t0:t0 + T].transpose(0, 1), w16.float(), b16.float(), padding=1))
    wd = torch.cat([w16.reshape(64, 27), w16.new_zeros(64, 5)], 1).contiguous().to(DEV)
    out = torch.full((T, H, W, 64), float("nan"), dtype=torch.float16, device=DEV)
    _enc_conv(x16.to(DEV), wd, b16.to(DEV), out, 0, T, H, W, 1, Tt, t0)
    _check("first_layer_3_64", out.float().cpu().permute(0, 3, 1, 2), ref)
    again = torch.empty_like(out)
    _enc_conv(x16.to(DEV), wd, b16.to(DEV), again, 0, T, H, W, 1, Tt, t0)
    assert torch.equal(again, out)


@pytest.mark.parametrize("kt", [1, 2], ids=["stride2", "stride2_two_time_taps"])
def test_stride2_forms_match_torch(kt):
    from realtime_video_amd.vae_decoder import pack_conv_weight
    g = torch.Generator().manual_seed(10 + kt)
    T, H, W = 3, 13, 21                           # 26x42 -> 13x21: 819 output pixels, partial 256-pixel tiles
    x16 = torch.randn(T * kt, 64, 2 * H, 2 * W, generator=g).half()
    w16 = (torch.randn(64, 64, kt, 3, 3, generator=g) / (64 * kt * 9) ** 0.5).half()
    ref = sum(F.conv2d(x16.float()[dt::kt], w16[:, :, dt].float(), stride=2, padding=1) for dt in range(kt))
    xd = x16.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = pack_conv_weight(w16 if kt == 2 else w16[:, :, 0]).to(DEV)
    out = torch.full((T, H, W, 64), float("nan"), dtype=torch.float16, device=DEV)
    _enc_conv(xd, wd, None, out, 1, T, H, W, kt, 0, 0)
    _check(f"stride2_kt{kt}", out.float().cpu().permute(0, 3, 1, 2), ref)
    again = torch.empty_like(out)
    _enc_conv(xd, wd, None, again, 1, T, H, W, kt, 0, 0)
    assert torch.equal(again, out)


def test_latent_head_matches_torch():
    """conv 64 -> 16 + bias, written as frames 2..4 of a planar [16][6][H][W] tensor; the other frames stay untouched."""
    from realtime_video_amd.vae_decoder import pack_conv_weight
    g = torch.Generator().manual_seed(20)
    T, H, W, To, j = 3, 7, 11, 6, 2
    x16 = torch.randn(T, 64, H, W, generator=g).half()
    w16 = (torch.randn(16, 64, 3, 3, generator=g) / 24.0).half()
    b16 = (torch.randn(16, generator=g) * 0.1).half()
    ref = F.conv2d(x16.float(), w16.float(), b16.float(), padding=1)
    xd = x16.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.full((16, To, H, W), 7.0, dtype=torch.float16, device=DEV)
    _enc_conv(xd, pack_conv_weight(w16).to(DEV), b16.to(DEV), out, 2, T, H, W, 1, To, j)
    _check("latent_head_64_16", out[:, j:j + T].float().cpu().transpose(0, 1), ref)
    assert bool((out[:, :j] == 7).all()) and bool((out[:, j + T:] == 7).all())
    again = torch.full_like(out, 7.0)
    _enc_conv(xd, pack_conv_weight(w16).to(DEV), b16.to(DEV), again, 2, T, H, W, 1, To, j)
    assert torch.equal(again, out)


def test_enc_conv_refuses_bad_arguments():
    x = torch.zeros(1, 16, 16, 64, dtype=torch.float16, device=DEV)
    w = torch.zeros(64, 18, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError):
        _enc_conv(x, w, None, x, 3, 1, 8, 8, 1, 0, 0)          # no such form
    with pytest.raises(RuntimeError):
        _enc_conv(x, w, None, x, 2, 1, 8, 8, 1, 1, 1)          # head frame outside the output tensor


def _encoder(seed):
    from realtime_video_amd.taehv import TAEHVEncoder
    return TAEHVEncoder(DEV).init_random_weights(seed)


def _stream(enc, frames01, splits):
    """frames01 [T, 3, H, W] in [0, 1] -> the wrapper's [1, 3, T, H, W] in [-1, 1], streamed in calls of `splits` frames."""
    x = (2 * frames01 - 1).transpose(0, 1)[None].to(DEV).half()
    cache, outs, t = [None] * 55, [], 0
    for i, n in enumerate(splits):
        mu, cache = enc(x[:, :, t:t + n], cache, stream=i > 0)
        outs.append(mu)
        t += n
    torch.cuda.synchronize()
    return torch.cat(outs, 2), cache


@pytest.mark.parametrize("name,splits", [("64x96_12", None), ("56x88_9_fresh", [9]), ("56x88_21_fresh", [9, 12])])
def test_streamed_encode_matches_golden(golden, name, splits):
    g = golden("taehv_encoder.pt")
    H, W, T, fresh = g["cases"][name]
    enc = _encoder(g["seed"])
    fr = golden_frames(H, W, T, g["frame_seed"])
    if fresh:
        mu, _ = _stream(enc, fr, splits)
    else:
        # 12 frames from a zero state without the repeated first frame: a carried cache of nine zero slices
        zero = [torch.zeros(1, 64, H >> s, W >> s, dtype=torch.float16, device=DEV) for s in (1, 1, 1, 2, 2, 2, 3, 3, 3)]
        mu, _ = enc((2 * fr - 1).transpose(0, 1)[None].to(DEV).half(), zero, stream=True)
    ref = g["latents"][name].transpose(0, 1)[None]            # [1, 16, T', h, w]
    assert mu.shape == ref.shape and mu.dtype == torch.float16
    err, mx = rel_l2(mu.float().cpu(), ref), max_abs(mu.float().cpu(), ref)
    print(f"TAEHV encoder {name} vs golden: max-abs {mx:.3e} rel-L2 {err:.3e}")
    assert err <= 5e-3 and mx <= 2e-2 * max(1.0, float(ref.abs().max()))


def test_split_invariance_bit_identical(golden):
    g = golden("taehv_encoder.pt")
    enc = _encoder(g["seed"])
    fr = golden_frames(56, 88, 21, g["frame_seed"])
    a, sa = _stream(enc, fr, [9, 12])
    b, sb = _stream(enc, fr, [9, 4, 4, 4])
    c, sc = _stream(enc, fr, [9, 8, 4])
    assert a.shape == (1, 16, 6, 7, 11)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert len(sa) == len(sb) == len(sc) == 9
    for x, y, u in zip(sa, sb, sc):
        assert x.data_ptr() != y.data_ptr() and torch.equal(x, y) and torch.equal(x, u)


def test_two_live_streams_and_recycle():
    """Streams A (9 frames fresh, then 12 streamed) and B (21 frames fresh: two GROUP calls) interleaved on one instance give
    what each gives alone on a fresh instance, latents and state, bit for bit; a stream started after A's cache list is gone
    runs on A's arena.  (No grow path: the arena is sized by GROUP.)"""
    from realtime_video_amd.taehv import TAEHVEncoder
    sd = TAEHVEncoder.random_state_dict(2)

    def fresh():
        enc = TAEHVEncoder(DEV)
        enc.load_state_dict(sd)
        return enc

    fa, fb, fc = (golden_frames(56, 88, 21, seed) for seed in (31, 32, 33))
    (ra, rsa), (rb, rsb), (rc, rsc) = _stream(fresh(), fa, [9, 12]), _stream(fresh(), fb, [21]), _stream(fresh(), fc[:9], [9])
    enc = fresh()

    def call(fr, t0, t1, cache):
        x = (2 * fr[t0:t1] - 1).transpose(0, 1)[None].to(DEV).half()
        return enc(x, cache, stream=t0 > 0)

    a0, sa = call(fa, 0, 9, [None] * 55)
    b0, sb = call(fb, 0, 21, [None] * 55)
    a1, sa = call(fa, 9, 21, sa)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([a0, a1], 2), ra) and torch.equal(b0, rb)
    assert len(sa) == len(sb) == 9
    assert all(torch.equal(x, y) for x, y in zip(sa, rsa)) and all(torch.equal(x, y) for x, y in zip(sb, rsb))
    arenas, a_ptr = len(enc._arenas._by_ptr), sa[0].data_ptr()
    assert arenas == 2
    del sa
    gc.collect()
    c0, sc = call(fc, 0, 9, [None] * 55)
    torch.cuda.synchronize()
    assert torch.equal(c0, rc) and all(torch.equal(x, y) for x, y in zip(sc, rsc))
    assert len(enc._arenas._by_ptr) == arenas and sc[0].data_ptr() == a_ptr
    assert all(torch.equal(x, y) for x, y in zip(sb, rsb))   # B's state is untouched by C


def test_production_size_matches_restatement():
    from realtime_video_amd.taehv import TAEHVEncoder
    sd = TAEHVEncoder.random_state_dict(5)
    enc = TAEHVEncoder(DEV)
    enc.load_state_dict(sd)
    g = torch.Generator().manual_seed(23)
    fr = torch.rand(21, 3, 480, 832, generator=g)
    mu, state = _stream(enc, fr, [9, 12])
    assert mu.shape == (1, 16, 6, 60, 104)
    sdd = {k: v.to(DEV) for k, v in sd.items()}
    x = (0.5 * (2 * fr - 1).half().float() + 0.5).to(DEV)        # the fp16 frames the wrapper sees, back in [0, 1]
    x = torch.cat([x[:1].expand(3, -1, -1, -1), x])
    with torch.no_grad():
        y0, st = restate_encode(sdd, x[:12])
        y1, st = restate_encode(sdd, x[12:], st)
    ref = torch.cat([y0, y1]).transpose(0, 1)
    err, mx = rel_l2(mu[0].float(), ref), max_abs(mu[0].float(), ref)
    print(f"TAEHV encoder 480x832, 9 + 12 frames vs fp32 restatement: max-abs {mx:.3e} rel-L2 {err:.3e}")
    assert err <= 5e-3 and mx <= 2e-2 * max(1.0, float(ref.abs().max()))
    assert len(state) == 9
    for k, (s, r) in enumerate(zip(state, st)):
        assert tuple(s.shape) == (1,) + tuple(r.shape), k
        e, m = rel_l2(s[0].float(), r), max_abs(s[0].float(), r)
        print(f"  state {k}: max-abs {m:.3e} rel-L2 {e:.3e}")
        assert e <= 5e-3 and m <= 2e-2 * max(1.0, float(r.abs().max())), (k, e, m)


def test_time_contract_errors():
    enc = _encoder(1)
    x = torch.zeros(1, 3, 12, 16, 16, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="1 \\+ 4k"):
        enc(x, [None] * 55, stream=False)                       # fresh cache with T = 12
    with pytest.raises(ValueError, match="1 \\+ 4k"):
        enc(x, None, stream=True)
    _, cache = enc(x[:, :, :9], [None] * 55, stream=False)
    with pytest.raises(ValueError, match="T = 4k"):
        enc(x[:, :, :9], cache, stream=True)                    # carried cache with T = 9
    with pytest.raises(ValueError, match="T = 4k"):
        enc(x, cache, stream=False)                             # carried cache without stream=True
    with pytest.raises(RuntimeError):
        enc(x[:, :, :9].cpu(), [None] * 55)
    with pytest.raises(ValueError):
        enc(torch.zeros(1, 3, 9, 20, 16, dtype=torch.float16, device=DEV), None)     # H not a multiple of 8
    mu, cache2 = enc(x, cache, stream=True)
    assert mu.shape == (1, 16, 3, 2, 2) and cache2[0].data_ptr() == cache[0].data_ptr()


def _session_parts():
    from oracle import wan_oracle as wo
    from oracle.make_golden import TEXT_DIM, TINY
    from realtime_video_amd.causal_model import CausalWanModel
    from realtime_video_amd.session import StaticTextEncoder
    from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
    cfg = dict(TINY)
    w = wo.make_weights(cfg, seed=0, text_dim=TEXT_DIM)
    m = CausalWanModel(dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"],
                       text_dim=TEXT_DIM, freq_dim=cfg.get("freq_dim", 256))
    m.load_state_dict(w)
    wr = WanDiffusionWrapper(m, timestep_shift=5.0)
    g = torch.Generator().manual_seed(5)
    padded = torch.zeros(1, 512, TEXT_DIM, dtype=torch.bfloat16)
    padded[0, :64] = torch.randn(64, TEXT_DIM, generator=g).to(torch.bfloat16)
    return wr, StaticTextEncoder(padded.to(DEV))


class _Recording:
    """Wraps an encoder: same call contract, keeps (frame count, latents) per call."""

    def __init__(self, enc):
        self.enc, self.calls = enc, []

    def __call__(self, frames, cache, stream=False):
        mu, c = self.enc(frames, cache, stream=stream)
        self.calls.append((frames.shape[2], mu.clone()))
        return mu, c


def test_session_webcam_mode_encodes_with_taehv():
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models
    from realtime_video_amd.taehv import TAEHVDecoder
    from realtime_video_amd.vae_decoder import VAEDecoderWrapper
    from realtime_video_amd.vae_encoder import encode_video_latent
    wr, text = _session_parts()
    g = torch.Generator().manual_seed(31)
    frames = (torch.rand(33, 3, 480, 832, generator=g) * 2 - 1).half()
    dec = TAEHVDecoder(DEV).init_random_weights(2)

    def run(use_taehv, **codecs):
        pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 750, 500, 250]),
                                       DEV, generator=wr, text_encoder=None, vae=None)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=text, **codecs)
        sess = GenerationSession(GenerateParams(seed=9, num_blocks=3, num_denoising_steps=4, keep_first_frame=True,
                                                webcam_mode=True, strength=0.8), models, device=DEV, use_taehv=use_taehv)
        seen = []
        inner = sess._randn_like

        def randn_like(t):                       # the session noises the encoded block: t is its latents [1, 3, 16, h, w]
            seen.append(t.clone())
            return inner(t)
        sess._randn_like = randn_like
        outs, t = [], 0
        for n in (9, 12, 12):
            for f in frames[t:t + n]:
                sess.push_frame(f.to(DEV))
            t += n
            outs.append(sess.generate_block())
        return outs, seen

    rec = _Recording(_encoder(4))
    outs, seen = run(True, vae_decoder=None, vae_encoder=None, taehv_decoder=dec, taehv_encoder=rec)
    assert [o.shape[1] for o in outs] == [6, 12, 12] and outs[0].shape[2:] == (3, 480, 832)
    assert [c[0] for c in rec.calls] == [9, 12, 12] and len(seen) == 3
    direct, cache, t = _encoder(4), [None] * 55, 0
    for b, n in enumerate((9, 12, 12)):
        lat, cache = encode_video_latent(direct, cache, frames=frames[t:t + n].to(DEV), height=480, width=832, stream=b > 0)
        t += n
        assert lat.shape == (16, 3, 60, 104)
        assert torch.equal(rec.calls[b][1][0], lat), b
        assert torch.equal(seen[b], lat[None].to(torch.bfloat16).movedim(1, 2)), b
    # no encoder of either kind: the webcam block cannot encode, as without use_taehv
    with pytest.raises((TypeError, RuntimeError)):
        run(True, vae_decoder=None, vae_encoder=None, taehv_decoder=dec)
    # use_taehv=False never touches the TAEHV encoder
    from realtime_video_amd.vae_encoder import VAEEncoderWrapper
    untouched = _Recording(_encoder(4))
    outs2, _ = run(False, vae_decoder=VAEDecoderWrapper(DEV).init_random_weights(), taehv_decoder=dec, taehv_encoder=untouched,
                   vae_encoder=VAEEncoderWrapper(device=DEV).init_random_weights())
    assert untouched.calls == [] and [o.shape[1] for o in outs2] == [6, 12, 12]


def test_session_first_frame_reencode_uses_taehv():
    """keep_first_frame=False: once the window slides (block 2) the oldest context pixel frame is re-encoded as a fresh
    one-frame stream - through the TAEHV encoder under use_taehv."""
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models
    from realtime_video_amd.taehv import TAEHVDecoder
    wr, text = _session_parts()
    rec = _Recording(_encoder(4))
    pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 750, 500, 250]),
                                   DEV, generator=wr, text_encoder=None, vae=None)
    models = Models(transformer=wr, pipeline=pipe, text_encoder=text, vae_decoder=None, vae_encoder=None,
                    taehv_decoder=TAEHVDecoder(DEV).init_random_weights(2), taehv_encoder=rec)
    sess = GenerationSession(GenerateParams(seed=9, num_blocks=3, num_denoising_steps=4, keep_first_frame=False),
                             models, device=DEV, use_taehv=True)
    seen = []
    inner = sess.get_clean_context_frames

    def ctx_frames(models):
        out = inner(models)
        seen.append(out)
        return out
    sess.get_clean_context_frames = ctx_frames
    outs = [sess.generate_block() for _ in range(3)]
    assert [o.shape[1] for o in outs] == [6, 12, 12]
    assert len(rec.calls) == 1 and rec.calls[0][0] == 1
    mu = rec.calls[0][1]
    assert mu.shape == (1, 16, 1, 60, 104) and float(mu.float().std()) > 1e-3
    first = mu.transpose(1, 2)                                   # [1, 1, 16, h, w]
    assert first.shape == (1, 1, 16, 60, 104)
    assert torch.equal(seen[-1][:, :1], first.to(seen[-1].dtype))


def test_round_trip_frame_count():
    """Sanity, not parity: under the 1 + 4k contract TAEHVDecoder(TAEHVEncoder(frames)) has the input's frame count."""
    from realtime_video_amd.taehv import TAEHVDecoder
    enc, dec = _encoder(4), TAEHVDecoder(DEV).init_random_weights(2)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(1, 3, 9, 64, 96, generator=g) * 2 - 1).half().to(DEV)
    mu, _ = enc(x, [None] * 55)
    assert mu.shape == (1, 16, 3, 8, 12)
    px, _ = dec(mu.transpose(1, 2), *([None] * 55))
    assert px.shape == (1, 9, 3, 64, 96)
    assert bool(torch.isfinite(px).all())
