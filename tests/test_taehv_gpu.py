"""GPU tests of the TAEHV tiny-VAE decoder (csrc/taehv.hip behind realtime_video_amd/taehv.py): every convolution form of
rtv_taehv_conv against torch fp32 conv2d, the streamed decode against the reference's golden, bit-identical results however
a stream is split into calls, the production size against the CPU-pinned restatement (tests/test_taehv_cpu.py) evaluated on
the GPU, two live streams on one instance (grow and recycle of a stream's arena), and the session's use_taehv switch."""
import ctypes
import gc

import pytest
import torch
import torch.nn.functional as F

from conftest import max_abs, rel_l2
from test_taehv_cpu import golden_latents, restate_decode

DEV = "cuda"
c_vp = ctypes.c_void_p
pytestmark = pytest.mark.gpu


def _ptr(t):
    return c_vp(t.data_ptr()) if t is not None else None


def lib_call(name, *args):
    """One library call on the current stream, then a device synchronise.  Shared with tests/test_taehv_encoder_gpu.py."""
    from realtime_video_amd import _lib, taehv  # noqa: F401  (registers the signatures)
    _lib.call(name, *args, c_vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def _conv_call(x, w, bias, res, out, T, H, W, Cin, Cout, kt, ups, n_split, relu, head):
    zeros = torch.zeros(64, dtype=torch.float16, device=DEV)
    lib_call("rtv_taehv_conv", _ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(out), T, H, W, Cin, Cout, kt, ups, n_split, relu,
             head, _ptr(zeros))


@pytest.mark.parametrize("T,hw", [(1, 96), (3, 60 * 104), (2, 777)])
def test_prep_kernel_clamp_and_layout(T, hw):
    """taehv_prep_kernel alone: z fp16 [T][16][hw] -> tanh(z / 3) * 3 -> channels-last [T][hw][32], within 1 fp16 ulp of the fp64
    evaluation (the kernel rounds an fp32 tanhf); +-0, +-60, +-65504 and a subnormal among the inputs; channels 16..31 exact
    zeros; nothing written behind the last pixel.  Inputs, reference and acceptance: tests/test_vae_units_cpu.py."""
    import test_vae_units_cpu as U
    z = U.taehv_prep_inputs(T, hw, device=DEV)
    out = torch.full((T * hw + 2, 32), float("nan"), dtype=torch.float16, device=DEV)
    lib_call("rtv_taehv_prep", _ptr(z), T, hw, _ptr(out))
    v = U.taehv_prep_violation(out[:T * hw].view(T, hw, 32), z)
    print(f"taehv_prep T={T} hw={hw}: {v} ulp (bound 1)")
    assert v <= 1
    assert bool(torch.isnan(out[T * hw:]).all())


FORMS = [
    # name, T, H, W, Cin, Cout, kt, ups, n_split, relu, residual, bias, head
    ("plain_relu_64", 2, 13, 21, 64, 64, 1, 0, 0, 1, False, True, False),
    ("memblock_window_zero_state", 3, 11, 9, 128, 128, 2, 0, 0, 1, False, True, False),
    ("memblock_window_state", 3, 11, 9, 128, 128, 2, 0, 0, 1, False, True, False),
    ("residual_relu_256", 2, 7, 11, 256, 256, 1, 0, 0, 1, True, True, False),
    ("upsample_fold_256_128", 2, 14, 22, 256, 128, 1, 1, 0, 0, False, False, False),
    ("upsample_fold_split_128", 2, 14, 18, 128, 128, 1, 1, 64, 0, False, False, False),
    ("upsample_fold_split_64_relu", 1, 26, 30, 64, 128, 1, 1, 64, 1, False, False, False),
    ("head_2y_minus_1", 3, 19, 23, 64, 8, 1, 0, 0, 0, False, True, True),
]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_conv_forms_match_torch(form):
    seed = FORMS.index(form)
    from realtime_video_amd.vae_decoder import pack_conv_weight
    name, T, H, W, Cin, Cout, kt, ups, n_split, relu, use_res, use_bias, head = form
    g = torch.Generator().manual_seed(seed)
    inH, inW = H >> ups, W >> ups
    x = torch.randn(T + kt - 1, Cin, inH, inW, generator=g)
    if name == "memblock_window_zero_state":
        x[0] = 0
    real_out = 3 if head else Cout
    w = torch.randn(real_out, Cin, kt, 3, 3, generator=g) / (Cin * kt * 9) ** 0.5
    b = torch.randn(real_out, generator=g) * 0.1 if use_bias else None
    x16, w16 = x.half(), w.half()
    # reference: fp32 conv of the fp16-rounded operands
    xr = F.interpolate(x16.float(), scale_factor=2, mode="nearest") if ups else x16.float()
    ref = sum(F.conv2d(xr[dt:dt + T], w16[:, :, dt].float(), padding=1) for dt in range(kt))
    if b is not None:
        ref = ref + b.half().float()[None, :, None, None]
    res = None
    if use_res:
        res = torch.randn(T, Cout, H, W, generator=g).half()
        ref = F.relu(ref + res.float())
    elif relu:
        ref = F.relu(ref)
    if head:
        ref = (2 * ref - 1).clamp(-1, 1)
    # device operands: channels-last activations, [Cout][kt * 9][Cin] weights
    xd = x16.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = pack_conv_weight(w16 if kt == 2 else w16[:, :, 0], cout_pad=8 if head else None).to(DEV)
    bd = None
    if b is not None:
        bb = b.half()
        bd = torch.cat([bb, bb.new_zeros(8 - 3)]).to(DEV) if head else bb.to(DEV)
    rd = res.permute(0, 2, 3, 1).contiguous().to(DEV) if res is not None else None
    if head:
        out = torch.full((T, 3, H, W), float("nan"), device=DEV)
    elif n_split:
        out = torch.full((2 * T, H, W, n_split), float("nan"), dtype=torch.float16, device=DEV)
    else:
        out = torch.full((T, H, W, Cout), float("nan"), dtype=torch.float16, device=DEV)
    _conv_call(xd, wd, bd, rd, out, T, H, W, Cin, 8 if head else Cout, kt, ups, n_split, relu, int(head))
    if head:
        got = out.float().cpu()
    elif n_split:
        got = out.float().cpu().permute(0, 3, 1, 2)                       # [2T][n_split][H][W]
        ref = torch.stack([ref[:, :n_split], ref[:, n_split:]], 1).reshape(2 * T, n_split, H, W)
    else:
        got = out.float().cpu().permute(0, 3, 1, 2)
    assert not torch.isnan(got).any()
    err, mx = rel_l2(got, ref), max_abs(got, ref)
    print(f"{name}: rel-L2 {err:.2e} max-abs {mx:.2e}")
    assert err <= 2e-3 and mx <= 2e-2 * max(1.0, float(ref.abs().max()))
    again = torch.empty_like(out)
    _conv_call(xd, wd, bd, rd, again, T, H, W, Cin, 8 if head else Cout, kt, ups, n_split, relu, int(head))
    assert torch.equal(again, out)


def _decoder(seed):
    from realtime_video_amd.taehv import TAEHVDecoder
    return TAEHVDecoder(DEV).init_random_weights(seed)


def _stream(dec, z, splits):
    state, outs, t = [None] * 55, [], 0
    for n in splits:
        px, state = dec(z[:, t:t + n].to(DEV).half(), *state)
        outs.append(px)
        t += n
    torch.cuda.synchronize()
    return torch.cat(outs, 1), state


@pytest.mark.parametrize("name,h,w", [("taehv_decoder.pt", 8, 12), ("taehv_decoder_7x11.pt", 7, 11)])
def test_streamed_decode_matches_golden(golden, name, h, w):
    g = golden(name)
    dec = _decoder(g["seed"])
    z = golden_latents(h, w, g["latent_seed"], g["T"])
    px, _ = _stream(dec, z, [3] * (g["T"] // 3))
    ref = 2 * g["outputs"][f"{h}x{w}"].float() - 1
    assert px.shape == ref.shape and px.dtype == torch.float32
    err, mx = rel_l2(px.cpu(), ref), max_abs(px.cpu(), ref)
    print(f"TAEHV {h}x{w} streamed 3+3 vs golden: max-abs {mx:.3e} rel-L2 {err:.3e}")
    assert mx <= 2e-2 and err <= 5e-3


def test_split_invariance_bit_identical(golden):
    g = golden("taehv_decoder_7x11.pt")
    dec = _decoder(g["seed"])
    z = golden_latents(7, 11, g["latent_seed"], 6)
    a, sa = _stream(dec, z, [3, 3])
    b, sb = _stream(dec, z, [1] * 6)
    c, sc = _stream(dec, z, [2, 4])
    assert a.shape == (1, 21, 3, 56, 88)
    assert torch.equal(a, b) and torch.equal(a, c)
    for x, y, u in zip(sa, sb, sc):
        assert torch.equal(x, y) and torch.equal(x, u)


def test_two_live_streams_grow_and_recycle():
    """Streams A (T = 2, then 4: longer than the arena sized on its first call, so its state moves to a larger one) and B
    (T = 3, 3) interleaved on one instance give what each gives alone on a fresh instance, pixels and state, bit for bit; a
    stream started after A's state list is gone runs on A's arena."""
    from realtime_video_amd.taehv import TAEHVDecoder
    sd = TAEHVDecoder.random_state_dict(2)

    def fresh():
        dec = TAEHVDecoder(DEV)
        dec.load_state_dict(sd)
        return dec

    za, zb, zc = (golden_latents(7, 11, seed, 6) for seed in (11, 12, 13))
    (ra, rsa), (rb, rsb), (rc, rsc) = _stream(fresh(), za, [2, 4]), _stream(fresh(), zb, [3, 3]), _stream(fresh(), zc[:, :3], [3])
    dec = fresh()

    def call(z, t0, t1, state):
        return dec(z[:, t0:t1].to(DEV).half(), *state)

    a0, sa = call(za, 0, 2, [None] * 55)
    small = sa[0].data_ptr()
    b0, sb = call(zb, 0, 3, [None] * 55)
    a1, sa = call(za, 2, 6, sa)
    b1, sb = call(zb, 3, 6, sb)
    torch.cuda.synchronize()
    assert sa[0].data_ptr() != small                      # A has moved
    assert torch.equal(torch.cat([a0, a1], 1), ra) and torch.equal(torch.cat([b0, b1], 1), rb)
    assert len(sa) == len(sb) == 9
    assert all(torch.equal(x, y) for x, y in zip(sa, rsa)) and all(torch.equal(x, y) for x, y in zip(sb, rsb))
    arenas, a_ptr = len(dec._arenas._by_ptr), sa[0].data_ptr()
    assert arenas == 2
    del sa
    gc.collect()
    c0, sc = call(zc, 0, 3, [None] * 55)
    torch.cuda.synchronize()
    assert torch.equal(c0, rc) and all(torch.equal(x, y) for x, y in zip(sc, rsc))
    assert len(dec._arenas._by_ptr) == arenas and sc[0].data_ptr() == a_ptr
    assert all(torch.equal(x, y) for x, y in zip(sb, rsb))   # B's state is untouched by C


def test_production_size_matches_restatement():
    from realtime_video_amd.taehv import TAEHVDecoder
    sd = TAEHVDecoder.random_state_dict(5)
    dec = TAEHVDecoder(DEV)
    dec.load_state_dict(sd)
    g = torch.Generator().manual_seed(21)
    z = torch.randn(1, 6, 16, 60, 104, generator=g)
    px, state = _stream(dec, z, [3, 3])
    assert px.shape == (1, 21, 3, 480, 832)
    sdd = {k: v.to(DEV) for k, v in sd.items()}
    zh = z[0].half().float().to(DEV)
    with torch.no_grad():
        y0, st = restate_decode(sdd, zh[:3])
        y1, st = restate_decode(sdd, zh[3:], st)
    ref = (2 * torch.cat([y0[3:], y1]) - 1).clamp(-1, 1)
    err, mx = rel_l2(px[0], ref), max_abs(px[0], ref)
    print(f"TAEHV 60x104, two 3-latent blocks vs fp32 restatement: max-abs {mx:.3e} rel-L2 {err:.3e}")
    assert mx <= 2e-2 and err <= 5e-3
    assert len(state) == 9
    for k, (s, r) in enumerate(zip(state, st)):
        assert tuple(s.shape) == (1,) + tuple(r.shape), k
        e = rel_l2(s[0].float(), r)
        assert e <= 5e-3, (k, e)


def test_session_use_taehv():
    from oracle import wan_oracle as wo
    from oracle.make_golden import TEXT_DIM, TINY
    from realtime_video_amd.causal_model import CausalWanModel
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    from realtime_video_amd.vae_decoder import VAEDecoderWrapper
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

    def run(use_taehv, **dec):
        pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 750, 500, 250]),
                                       DEV, generator=wr, text_encoder=None, vae=None)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(padded.to(DEV)), **dec)
        sess = GenerationSession(GenerateParams(seed=9, num_blocks=3, num_denoising_steps=4, keep_first_frame=True),
                                 models, device=DEV, use_taehv=use_taehv)
        return sess, [sess.generate_block() for _ in range(3)]

    taehv = _decoder(2)
    sess, outs = run(True, vae_decoder=None, taehv_decoder=taehv)
    assert [o.shape[1] for o in outs] == [6, 12, 12]
    px = torch.cat(outs, 1)
    assert px.dtype == torch.float32 and px.shape[2:] == (3, 480, 832)
    assert float(px.min()) >= -1 and float(px.max()) <= 1 and float(px.std()) > 1e-3
    direct, _ = taehv(sess.all_latents.half(), *([None] * 55))
    assert torch.equal(direct[:, 3:], px)
    with pytest.raises(ValueError):
        run(True, vae_decoder=None)
    sess2, outs2 = run(False, vae_decoder=VAEDecoderWrapper(DEV).init_random_weights(), taehv_decoder=taehv)
    assert [o.shape[1] for o in outs2] == [6, 12, 12] and outs2[0].dtype == torch.float32
    assert not torch.equal(torch.cat(outs2, 1), px)
