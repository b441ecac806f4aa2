"""GPU tests of the JPEG frame decoder (csrc/jpeg_decode.hip behind ops.jpeg_decode / ops.jpeg_decode_coefficients,
frames.FrameUploader.push_jpeg and GenerationSession.push_frame).  The reference is tests/jpeg_decode_oracle.py, which
tests/test_jpeg_decode_cpu.py pins to PIL byte for byte, so every comparison here is an equality.

Sizes: (8, 8) one block; (16, 16) one 4:2:0 MCU; (17, 23) cropped edges on both axes and, for 4:2:0, a chroma edge that needs
replication; (24, 40); (152, 24) ten MCU rows, so RSTn wraps; one (160, 240) noise image at q 95 whose restart-free scan spans
hundreds of default-length subsequences and takes many rounds."""
import base64
import functools

import numpy as np
import pytest
import torch

import jpeg_decode_oracle as jd
import jpeg_oracle as jo

DEV = "cuda"
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _valid():
    """{name: (file, oracle info, oracle coefficients, oracle pixels)}, computed once."""
    out = {}
    for name, data in jd.valid_files().items():
        info = jd.parse(data)
        coef = jd.entropy_decode(info)
        out[name] = (data, info, coef, jd.pixels(info, coef))
    return out


def _own_files():
    """Files of the native encoder (one restart interval per MCU row), over the sizes that are multiples of 8."""
    from realtime_video_amd import ops
    out = {}
    for H, W in [s for s in jd.SIZES if s[0] % 8 == 0 and s[1] % 8 == 0] + [(48, 64)]:
        rgb = torch.from_numpy(np.stack([jo.image(H, W, "smooth", seed=3), jo.image(H, W, "noise", seed=4)])).to(DEV)
        buf, offs = ops.jpeg_encode(rgb, 90)
        buf, offs = buf.cpu().numpy().tobytes(), offs.tolist()
        for t in range(2):
            out[f"native_{H}x{W}_{t}"] = buf[offs[t]:offs[t + 1]]
    return out


@pytest.mark.parametrize("subseq_bits", [0, 32])
def test_coefficients_equal_the_oracles(subseq_bits):
    """PIL files in every sampling mode, with and without optimised tables and restart markers, and the native encoder's files.
    At 32 bits every subsequence boundary of the small files falls mid-symbol; the 160 x 240 file at the default length has
    hundreds of subsequences.  Two calls give identical output."""
    from realtime_video_amd import ops
    most = 0
    for name, (data, info, coef, _) in _valid().items():
        got, status, rounds = ops.jpeg_decode_coefficients(data, subseq_bits)
        assert int(status) == 0, name
        assert len(got) == len(coef)
        for g, w in zip(got, coef):
            assert g.shape == w.shape and torch.equal(g.cpu(), torch.from_numpy(w)), name
        most = max(most, int(rounds))
        if name.endswith("_opt") or "160x240" in name:
            again = ops.jpeg_decode_coefficients(data, subseq_bits)
            assert all(torch.equal(a, b) for a, b in zip(again[0], got)) and int(again[2]) == int(rounds)
    assert most > 3                                                       # rounds were needed, and the loop ended
    for name, data in _own_files().items():
        want = jd.entropy_decode(jd.parse(data))
        got, status, _ = ops.jpeg_decode_coefficients(data, subseq_bits)
        assert int(status) == 0 and all(torch.equal(g.cpu(), torch.from_numpy(w)) for g, w in zip(got, want)), name


def test_pixels_equal_the_oracles_and_pils():
    from realtime_video_amd import ops
    names = list(_valid())
    for t0 in range(0, len(names), 16):                                   # 16 frames of mixed sizes and sampling per call
        part = names[t0:t0 + 16]
        out, status = ops.jpeg_decode([_valid()[n][0] for n in part])
        assert status.tolist() == [0] * len(part)
        for n, o in zip(part, out):
            want = _valid()[n][3]
            assert o.dtype == torch.uint8 and tuple(o.shape) == want.shape and o.is_cuda
            assert torch.equal(o.cpu(), torch.from_numpy(want)), n
    # T = 3 frames of different sizes and sampling in one call, against PIL itself; more than 16 files take several calls
    three = ["420_17x23_smooth_q90", "444_152x24_noise_q50", "grey_24x40_smooth_q90"]
    out, status = ops.jpeg_decode([_valid()[n][0] for n in three])
    assert status.tolist() == [0, 0, 0]
    for n, o in zip(three, out):
        assert torch.equal(o.cpu(), torch.from_numpy(jd.pil_pixels(_valid()[n][0]))), n
    out, status = ops.jpeg_decode([_valid()[n][0] for n in names[:18]])
    assert len(out) == 18 and status.tolist() == [0] * 18
    assert torch.equal(out[17].cpu(), torch.from_numpy(_valid()[names[17]][3]))


def test_round_trip_with_the_encoder():
    """jpeg_decode(jpeg_encode(rgb8)) equals PIL's decode of the same files."""
    from realtime_video_amd import ops
    files = _own_files()
    out, status = ops.jpeg_decode(list(files.values()))
    assert status.tolist() == [0] * len(files)
    for (name, data), o in zip(files.items(), out):
        assert torch.equal(o.cpu(), torch.from_numpy(jd.pil_pixels(data))), name


# fifteen of the damaged files the sanitised host check has passed on the CPU (tests/test_jpeg_decode_cpu.py), every way of damage
# and every status bit among them; with one clean frame they fill ONE call
DAMAGED = ["420_cut50", "420_flip3", "420_marker0", "420_marker1", "420_huff_00", "444rst_cut10", "444rst_flip0", "444rst_flip1",
           "444rst_marker0", "own_cut90", "own_flip3", "own_marker3", "grey_opt_flip1", "grey_opt_marker2", "grey_opt_huff_00"]


def test_damaged_files_stay_inside_their_bounds(tmp_path):
    from realtime_video_amd import ops
    prog = jd.build_hostcheck(sanitize=False)                             # the plain build: its status words are the expectation
    assert prog is not None
    damaged = jd.damaged_files()
    files = {n: damaged[n] for n in DAMAGED}
    rc, err, host = jd.run_hostcheck(prog, files, 0, str(tmp_path))
    assert rc == 0 and all(host[n][0] != "refused" for n in DAMAGED)
    clean = "420_24x40_smooth_q90"
    batch = [files[n] for n in DAMAGED[:7]] + [_valid()[clean][0]] + [files[n] for n in DAMAGED[7:]]
    infos = [ops.jpeg_parse(f) for f in batch]
    G = 4096                                                              # guard bytes around the arena and every output frame
    need = ops.jpeg_decode_arena_bytes(infos)
    arena = torch.full((need + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    bufs = [torch.full((i.H * i.W * 3 + 2 * G,), 0x5A, dtype=torch.uint8, device=DEV) for i in infos]
    outs = [b[G:G + i.H * i.W * 3].view(i.H, i.W, 3) for b, i in zip(bufs, infos)]
    out, status = ops.jpeg_decode(batch, out=outs, arena=arena[G:G + need])          # returns: the call itself succeeded
    torch.cuda.synchronize()
    want = [host[n][0] for n in DAMAGED[:7]] + [0] + [host[n][0] for n in DAMAGED[7:]]
    assert status.tolist() == want
    assert set(want) >= {0, 1, 2, 8, 16}
    assert torch.equal(out[7].cpu(), torch.from_numpy(_valid()[clean][3]))           # the clean frame is unaffected
    assert bool((arena[:G] == 0xA5).all()) and bool((arena[G + need:] == 0xA5).all())
    for b, i in zip(bufs, infos):
        assert bool((b[:G] == 0x5A).all()) and bool((b[G + i.H * i.W * 3:] == 0x5A).all())
    # the coefficients of a damaged frame are the host check's too: what was reached, and zeros behind it
    for n in ("420_flip3", "444rst_marker0", "grey_opt_huff_00"):
        got, st, _ = ops.jpeg_decode_coefficients(files[n])
        assert int(st) == host[n][0] and np.array_equal(torch.cat([g.reshape(-1) for g in got]).cpu().numpy(), host[n][2]), n


def _frames(n, H, W, seed=0):
    return [jo.image(H, W, "smooth", seed=seed + i) for i in range(n)]


def test_uploader_push_jpeg():
    from realtime_video_amd import ops
    from realtime_video_amd.frames import FrameUploader
    imgs = _frames(14, 48, 64)
    files = [jd.pil_file(im, 80, ("420", "444", "422")[i % 3], **(dict(optimize=True) if i % 4 == 0 else {})) for i, im in enumerate(imgs)]
    px = [jd.pil_pixels(f) for f in files]
    up_j, up_r = FrameUploader(DEV, slots=8), FrameUploader(DEV, slots=8)
    tj = [up_j.push_jpeg(f if i % 3 == 0 else bytearray(f) if i % 3 == 1 else memoryview(f)) for i, f in enumerate(files[:6])]
    tr = [up_r.push(p) for p in px[:6]]
    assert tj == tr == list(range(6))
    assert torch.equal(up_j.gather(tj, (48, 64)), up_r.gather(tr, (48, 64)))          # equal size: bit for bit
    assert torch.equal(up_j.gather(tj, (32, 48)), up_r.gather(tr, (32, 48)))          # and through the resize
    assert [up_j.status(t) for t in tj] == [0] * 6
    # raw and JPEG pushes mixed in one gather, while the ring wraps (8 slots, 14 pushes)
    for i in range(6, 14):
        tj.append(up_j.push_jpeg(files[i]) if i % 2 else up_j.push(px[i]))
        tr.append(up_r.push(px[i]))
    with pytest.raises(KeyError):
        up_j.gather([tj[2]], (48, 64))
    with pytest.raises(KeyError):
        up_j.status(tj[2])
    pick = [13, 6, 9, 12, 7]
    assert torch.equal(up_j.gather(pick, (48, 64)), up_r.gather(pick, (48, 64)))
    assert up_j.status(13) == 0 and up_j.status(12) == 0
    # a refused file raises before anything is queued: the ring is as usable as before
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(imgs[0]).save(b, format="JPEG", progressive=True)
    with pytest.raises(ValueError, match="progressive"):
        up_j.push_jpeg(b.getvalue())
    assert up_j.push_jpeg(files[0]) == 14
    assert torch.equal(up_j.gather([14, 13], (48, 64)), ops.frames_from_rgb8(torch.from_numpy(np.stack([px[0], px[13]])).to(DEV), (48, 64)))
    # a file of another size reallocates the rings: the old tickets are gone, the new one works; then a raw frame of that size
    small = jd.pil_file(jo.image(17, 23, "noise"), 90, "420")
    t = up_j.push_jpeg(small)
    with pytest.raises(KeyError):
        up_j.gather([14], (48, 64))
    t2 = up_j.push(jd.pil_pixels(small))
    got = up_j.gather([t, t2], (24, 40))
    assert torch.equal(got[:, 0], got[:, 1])
    assert torch.equal(got, ops.frames_from_rgb8(torch.from_numpy(np.stack([jd.pil_pixels(small)] * 2)).to(DEV), (24, 40)))
    # a damaged file decodes to a status word, not to an exception
    bad = jd.damaged_files()["420_flip3"]
    assert up_j.status(up_j.push_jpeg(bad)) == 2


class _RecordingEncoder:
    def __init__(self, enc):
        self.enc, self.inputs = enc, []

    def __call__(self, frames, cache, stream=False):
        self.inputs.append(frames.clone())
        return self.enc(frames, cache, stream=stream)


def test_session_push_frame_takes_the_cameras_bytes():
    """bytes, base64 str and a data: URL give the latents of the PIL-decoded uint8 frames, bit for bit, for a webcam block (the
    rig of test_frame_input_gpu.test_session_takes_camera_frames, TAEHV codecs, block 0)."""
    from oracle import wan_oracle as wo
    from test_dit_gpu import _build, _tiny
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    from realtime_video_amd.taehv import TAEHVDecoder, TAEHVEncoder
    cfg, text_dim, _ = _tiny()
    cfg["num_layers"] = 1
    _, wr = _build(cfg, text_dim, wo.make_weights(cfg, seed=0, text_dim=text_dim))
    g = torch.Generator().manual_seed(11)
    prompt = torch.zeros(1, 512, text_dim, dtype=torch.bfloat16)
    prompt[0, :64] = torch.randn(64, text_dim, generator=g).to(torch.bfloat16)
    codecs = dict(taehv_decoder=TAEHVDecoder(DEV).init_random_weights(2), taehv_encoder=TAEHVEncoder(DEV).init_random_weights(4))
    base = jo.image(480 + 16, 832 + 16, "smooth")
    files = [jd.pil_file(np.ascontiguousarray(base[i:i + 480, 2 * i:2 * i + 832]), 80, "420") for i in range(9)]   # the browser case

    def run(push):
        rec = _RecordingEncoder(codecs["taehv_encoder"])
        pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 500]), DEV, generator=wr)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(prompt.to(DEV)), **dict(codecs, taehv_encoder=rec))
        sess = GenerationSession(GenerateParams(prompt="a", seed=1, num_blocks=1, num_denoising_steps=2, strength=0.7,
                                                webcam_mode=True, keep_first_frame=True), models, device=DEV, use_taehv=True)
        seen = []
        inner = sess._randn_like

        def randn_like(t):
            seen.append(t.clone())
            return inner(t)
        sess._randn_like = randn_like
        for i, f in enumerate(files):
            push(sess, i, f)
        sess.generate_block()
        return sess, rec, seen

    def as_kind(i, f):
        text = base64.b64encode(f).decode()
        return (f, text, "data:image/jpeg;base64," + text)[i % 3]

    _, rec_p, seen_p = run(lambda s, i, f: s.push_frame(jd.pil_pixels(f)))
    sess, rec_j, seen_j = run(lambda s, i, f: s.push_frame(as_kind(i, f)))
    assert [x.shape for x in rec_j.inputs] == [(1, 3, 9, 480, 832)] and len(seen_j) == 1
    assert torch.equal(rec_j.inputs[0], rec_p.inputs[0]) and torch.equal(seen_j[0], seen_p[0])
    assert all(sess.uploader.status(t) == 0 for t in range(9))
    # a JPEG file counts as a uint8 frame for the one-kind-per-block rule; a refused file queues nothing
    sess.push_frame(files[0])
    sess.push_frame(jd.pil_pixels(files[1]))
    with pytest.raises(ValueError):
        sess.push_frame(torch.zeros(3, 480, 832, dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="not a JPEG"):
        sess.push_frame(b"not a jpeg file")
    assert len(sess.frame_queue) == 2
