"""GPU tests of the pixel input path (csrc/frame_input.hip behind ops.frames_from_rgb8, frames.FrameUploader and the uint8
paths of encode_video_latent / GenerationSession.push_frame).  The numeric reference is the reference's own call,
torch.nn.functional.interpolate(mode="bicubic"), evaluated in float64 on the CPU on the decoded fp16 frames.

Acceptance rule of a resized output element: |got - e| <= 0.5 * ulp16(e) + 2**-15, e the float64 result, ulp16 the fp16 spacing
at |e| (the subnormal spacing 2**-24 below 2**-14).  The half ulp is the final rounding, the 2**-15 covers fp32 accumulation and
fp32 source coordinates: torch's own float32 result exceeds the half ulp by at most 2.1e-6 on the small shapes below and by
7.4e-6 on the smooth 720 x 1280 case (CPU, against float64), a margin of 4x and more.  Every element is checked."""
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
pytestmark = pytest.mark.gpu


def decode(u8):
    """release_server.py:479-481 on bytes [..., H, W, 3] -> fp16 [..., 3, H, W]: to_tensor, half, sub_(0.5).mul_(2.0)."""
    return ((u8.movedim(-1, -3).float() / 255).half() - 0.5) * 2.0


def ulp16(e):
    return 2.0 ** (torch.floor(torch.log2(e.abs().clamp_min(2.0 ** -14))) - 10)


def check_resized(name, got, u8, size):
    """got [3, T, h, w] from the kernel for bytes u8 [T, Hin, Win, 3]."""
    e = F.interpolate(decode(u8).double(), size=size, mode="bicubic").transpose(0, 1)
    got = got.cpu()
    assert got.shape == e.shape and got.dtype == torch.float16 and torch.isfinite(got).all()
    excess = ((got.double() - e).abs() - 0.5 * ulp16(e)).max().item()
    not_bit_equal = (got != e.half()).float().mean().item()
    print(f"{name}: worst excess over the half ulp {excess:.3e} (allowed {2.0 ** -15:.3e}); "
          f"{100 * not_bit_equal:.3f} % of the elements differ from the rounded float64 result (recorded, not gated)")
    assert excess <= 2.0 ** -15, name


def test_decode_only_is_the_table_value_bit_for_bit():
    from realtime_video_amd import ops
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (3, 24, 40, 3), generator=g, dtype=torch.uint8)
    u8.view(-1)[torch.randperm(u8.numel(), generator=g)[:256]] = torch.arange(256, dtype=torch.uint8)
    assert len(torch.unique(u8)) == 256
    expect = (((u8.permute(0, 3, 1, 2).float() / 255).half() - 0.5) * 2.0).transpose(0, 1)
    got = ops.frames_from_rgb8(u8.to(DEV), (24, 40))
    assert got.shape == (3, 3, 24, 40) and got.dtype == torch.float16 and got.is_contiguous()
    assert torch.equal(got.cpu(), expect)
    # frames at byte offsets that are no multiple of 4 (a view into a larger byte buffer) decode the same
    buf = torch.zeros(u8.numel() + 8, dtype=torch.uint8, device=DEV)
    buf[1:1 + u8.numel()] = u8.view(-1).to(DEV)
    assert torch.equal(ops.frames_from_rgb8(buf[1:1 + u8.numel()].view(u8.shape), (24, 40)).cpu(), expect)
    with pytest.raises(ValueError):
        ops.frames_from_rgb8(u8.to(DEV).float(), (24, 40))
    with pytest.raises(ValueError):
        ops.frames_from_rgb8(u8.to(DEV).permute(0, 2, 1, 3), (24, 40))
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.frames_from_rgb8(u8.to(DEV), (20, 40))


@pytest.mark.parametrize("src,dst", [((20, 28), (24, 40)), ((7, 9), (24, 40)), ((36, 50), (24, 40)), ((45, 80), (24, 40)),
                                     ((33, 47), (16, 24))], ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_matches_torch_bicubic(src, dst):
    from realtime_video_amd import ops
    g = torch.Generator().manual_seed(src[0] * 100 + src[1])
    u8 = torch.randint(0, 256, (2,) + src + (3,), generator=g, dtype=torch.uint8)
    got = ops.frames_from_rgb8(u8.to(DEV), dst)
    check_resized(f"{src} -> {dst}", got, u8, dst)
    assert torch.equal(ops.frames_from_rgb8(u8.to(DEV), dst), got)          # deterministic


def test_production_sized_frame():
    """720 x 1280 -> 480 x 832 on a smooth image: 64-bit indexing, every tile shape of the launch and the fp32 coordinates at
    large dst.  (Random noise at this size fails the rule for torch's own float32 result: the fp32 coordinate rounding at large
    dst times a slope of about 1 per pixel exceeds the slack, 1.6e-4.)"""
    from realtime_video_amd import ops
    g = torch.Generator().manual_seed(3)
    img = F.interpolate(torch.rand(1, 3, 45, 80, generator=g), size=(720, 1280), mode="bilinear")
    u8 = (img * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    got = ops.frames_from_rgb8(u8.to(DEV), (480, 832))
    check_resized("720x1280 -> 480x832", got, u8, (480, 832))


def test_out_argument_and_more_frames_than_one_launch_takes():
    """20 frames = two launches (16 + 4) into one output tensor; `slots` picks and repeats frames."""
    from realtime_video_amd import ops
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (20, 9, 13, 3), generator=g, dtype=torch.uint8).to(DEV)
    out = torch.full((3, 20, 16, 24), float("nan"), dtype=torch.float16, device=DEV)
    assert ops.frames_from_rgb8(u8, (16, 24), out=out) is out
    for t in (0, 15, 16, 19):
        assert torch.equal(out[:, t:t + 1], ops.frames_from_rgb8(u8[t:t + 1], (16, 24))), t
    pick = [19, 0, 0, 7]
    assert torch.equal(ops.frames_from_rgb8(u8, (16, 24), slots=pick), out[:, pick])
    with pytest.raises(IndexError):
        ops.frames_from_rgb8(u8, (16, 24), slots=[20])


def test_uploader_ring_gather():
    from realtime_video_amd import ops
    from realtime_video_amd.frames import FrameUploader
    from realtime_video_amd.session import resample_array
    g = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (34, 20, 28, 3), generator=g, dtype=torch.uint8)
    up = FrameUploader(DEV, slots=16)
    tickets = [up.push(f.numpy() if i % 2 else f) for i, f in enumerate(frames[:14])]      # torch and numpy frames
    assert tickets == list(range(14))
    pick = resample_array(tickets, 12)
    assert len(pick) == 12 and len(set(pick)) == 12
    got = up.gather(pick, (24, 40))
    assert torch.equal(got, ops.frames_from_rgb8(frames[pick].to(DEV), (24, 40)))
    for i, f in enumerate(frames[14:34]):                            # 20 more pushes wrap the 16-slot ring
        last = up.push(f.to(DEV) if i % 2 else f)                    # CUDA frames too
    assert last == 33
    with pytest.raises(KeyError):
        up.gather([tickets[3]], (24, 40))
    fresh = [33, 18, 25, 33]
    assert torch.equal(up.gather(fresh, (24, 40)), ops.frames_from_rgb8(frames[fresh].to(DEV), (24, 40)))
    # a frame of another size reallocates the rings: the old tickets are gone, the new one works
    t = up.push(frames[0, :12, :20].contiguous())
    with pytest.raises(KeyError):
        up.gather([33], (24, 40))
    assert torch.equal(up.gather([t], (24, 40)), ops.frames_from_rgb8(frames[:1, :12, :20].contiguous().to(DEV), (24, 40)))
    with pytest.raises(ValueError):
        up.push(torch.zeros(3, 20, 28, dtype=torch.uint8))


class _RecordingEncoder:
    """Wraps an encoder: same call contract, keeps a copy of every input it is given."""

    def __init__(self, enc):
        self.enc, self.inputs = enc, []

    def __call__(self, frames, cache, stream=False):
        self.inputs.append(frames.clone())
        return self.enc(frames, cache, stream=stream)


@pytest.mark.parametrize("use_taehv", [False, True], ids=["wan_vae", "taehv"])
def test_session_takes_camera_frames(use_taehv):
    """uint8 [H, W, 3] frames at the session's size give the latents of the corresponding float [3, H, W] frames, bit for bit,
    over block 0 (9 frames) and block 1 (12 frames, stream=True); half-size frames run, and the encoder's input is
    ops.frames_from_rgb8 of them; a mixed queue is refused."""
    from oracle import wan_oracle as wo
    from test_dit_gpu import _build, _tiny
    from realtime_video_amd import ops
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    cfg, text_dim, _ = _tiny()
    cfg["num_layers"] = 1
    _, wr = _build(cfg, text_dim, wo.make_weights(cfg, seed=0, text_dim=text_dim))
    g = torch.Generator().manual_seed(11)
    prompt = torch.zeros(1, 512, text_dim, dtype=torch.bfloat16)
    prompt[0, :64] = torch.randn(64, text_dim, generator=g).to(torch.bfloat16)
    if use_taehv:
        from realtime_video_amd.taehv import TAEHVDecoder, TAEHVEncoder
        codecs = dict(taehv_decoder=TAEHVDecoder(DEV).init_random_weights(2), taehv_encoder=TAEHVEncoder(DEV).init_random_weights(4))
    else:
        from realtime_video_amd.vae_encoder import VAEEncoderWrapper
        codecs = dict(vae_encoder=VAEEncoderWrapper(device=DEV).init_random_weights(seed=1))
    key = "taehv_encoder" if use_taehv else "vae_encoder"
    u8 = torch.randint(0, 256, (21, 480, 832, 3), generator=g, dtype=torch.uint8)
    half = torch.randint(0, 256, (9, 240, 416, 3), generator=g, dtype=torch.uint8)

    def run(blocks, push):
        rec = _RecordingEncoder(codecs[key])
        pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 500]), DEV, generator=wr)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(prompt.to(DEV)), **dict(codecs, **{key: rec}))
        sess = GenerationSession(GenerateParams(prompt="a", seed=1, num_blocks=2, num_denoising_steps=2, strength=0.7,
                                                webcam_mode=True, keep_first_frame=True), models, device=DEV, use_taehv=use_taehv)
        seen = []
        inner = sess._randn_like

        def randn_like(t):                       # the session noises the encoded block: t is its latents [1, 3, 16, h, w]
            seen.append(t.clone())
            return inner(t)
        sess._randn_like = randn_like
        for b in range(blocks):
            push(sess, b)
            sess.generate_block()
        return sess, rec, seen

    def push_u8(sess, b):
        for i, f in enumerate(u8[:9] if b == 0 else u8[9:21]):
            sess.push_frame(f if i % 3 == 0 else f.numpy() if i % 3 == 1 else f.to(DEV))

    def push_float(sess, b):
        for f in (u8[:9] if b == 0 else u8[9:21]):
            sess.push_frame(decode(f).to(DEV))

    _, rec_f, seen_f = run(2, push_float)
    sess, rec_u, seen_u = run(2, push_u8)
    assert [x.shape for x in rec_u.inputs] == [(1, 3, 9, 480, 832), (1, 3, 12, 480, 832)] and len(seen_u) == 2
    for b in range(2):
        assert torch.equal(rec_u.inputs[b], rec_f.inputs[b]), b
        assert torch.equal(seen_u[b], seen_f[b]), b
    # a mixed queue
    sess.push_frame(u8[0])
    with pytest.raises(ValueError):
        sess.push_frame(decode(u8[1]).to(DEV))

    _, rec_h, seen_h = run(1, lambda sess, b: [sess.push_frame(f) for f in half])
    assert torch.equal(rec_h.inputs[0][0], ops.frames_from_rgb8(half.to(DEV), (480, 832)))
    assert seen_h[0].shape == seen_u[0].shape and torch.isfinite(seen_h[0]).all()


def test_encode_video_latent_takes_a_uint8_clip():
    """uint8 [T, Hin, Win, 3]: max_frames truncation, one launch to (h, w), the encoder - the latents of the float path fed
    with the kernel's own output."""
    from realtime_video_amd import ops
    from realtime_video_amd.taehv import TAEHVEncoder
    from realtime_video_amd.vae_encoder import encode_video_latent
    g = torch.Generator().manual_seed(13)
    clip = torch.randint(0, 256, (11, 30, 44, 3), generator=g, dtype=torch.uint8).to(DEV)
    rec = _RecordingEncoder(TAEHVEncoder(DEV).init_random_weights(4))
    lat, _ = encode_video_latent(rec, [None] * 55, frames=clip, height=68, width=100, stream=False, max_frames=None)
    planar = ops.frames_from_rgb8(clip[:9], (64, 96))                       # 1 + ((11 - 1) // 4) * 4 = 9 frames, sizes floored to 8
    assert torch.equal(rec.inputs[0][0], planar)
    ref, _ = encode_video_latent(TAEHVEncoder(DEV).init_random_weights(4), [None] * 55, frames=planar.transpose(0, 1).contiguous(),
                                 height=64, width=96, stream=False, max_frames=None)
    assert lat.shape == (16, 3, 8, 12) and torch.equal(lat, ref)
