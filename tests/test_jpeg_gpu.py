"""GPU tests of the JPEG frame encoder (csrc/jpeg_encode.hip behind ops.jpeg_coefficients / ops.jpeg_encode and
frames.JpegFrameDownloader) against tests/jpeg_oracle.py, the numpy restatement of the stream that tests/test_jpeg_cpu.py pins
to PIL's encoder.

Coefficients: equal to the oracle's, except where the oracle's float64 value before rounding lies within 1e-3 of a half - there
the kernel's fp32 DCT may round the other way (a difference of 1).  The fp32 error of a coefficient is far below that: samples
below 128 and 16 products per output give about 16 * 128 * 2**-24 = 1.2e-4 before the division by a step >= 1.  Such positions
may be at most 1 % of all coefficients (a uniform fraction puts 0.2 % there).
Entropy coder: exact - the file is header + oracle.entropy_encode(the kernel's own coefficients) + EOI, byte for byte."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_oracle as jo

DEV = "cuda"
pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (24, 40), (48, 64), (152, 24)]          # one MCU; both sides 8 mod 16; several MCUs; 10 MCU rows (RSTn wraps)
CASES = [(size, T, q) for size in SIZES for T in (1, 3) for q in (50, 90, 100)]
ids = lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def frames(size, T):
    """uint8 [T, H, W, 3]: smooth, noise, smooth."""
    return np.stack([jo.image(size[0], size[1], "noise" if t == 1 else "smooth", seed=t) for t in range(T)])


@functools.lru_cache(maxsize=None)
def oracle_coefficients(size, T, q):
    return [jo.coefficients(f, q) for f in frames(size, T)]


def files(out, offsets):
    out, offsets = out.cpu().numpy().tobytes(), offsets.cpu().tolist()
    assert offsets[0] == 0 and all(a < b for a, b in zip(offsets[:-1], offsets[1:]))
    return [out[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def check_file(data, H, W, q):
    """Structure of one file: header, RSTn between the MCU rows in order mod 8, EOI at the end, and PIL decodes all of it."""
    head = jo.header(q, H, W)
    assert data[:len(head)] == head and data.endswith(jo.EOI)
    scan = data[len(head):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0x00]
    rows = -(-H // 16)
    assert marks == [0xD0 + i % 8 for i in range(rows - 1)] + [0xD9]
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (W, H) and im.mode == "RGB"
    return np.asarray(im)


@pytest.mark.parametrize("size,T,q", CASES, ids=ids)
def test_coefficients_match_the_oracle(size, T, q):
    from realtime_video_amd import ops
    rgb8 = torch.from_numpy(frames(size, T)).to(DEV)
    got = ops.jpeg_coefficients(rgb8, q)
    assert got.dtype == torch.int16 and got.shape == (T, -(-size[0] // 16), -(-size[1] // 16), 6, 64)
    assert torch.equal(ops.jpeg_coefficients(rgb8, q), got)                              # deterministic
    got = got.cpu().numpy().astype(np.int64)
    near_total = differ_total = 0
    for t, (ref, pre) in enumerate(oracle_coefficients(size, T, q)):
        frac = np.abs(pre) - np.floor(np.abs(pre))
        near = np.abs(frac - 0.5) < 1e-3
        diff = np.abs(got[t] - ref)
        assert not (diff[~near] != 0).any(), (t, int((diff[~near] != 0).sum()))
        assert diff.max() <= 1
        near_total, differ_total = near_total + int(near.sum()), differ_total + int((diff != 0).sum())
    share = near_total / got.size
    print(f"{size} T={T} q={q}: {100 * share:.3f} % of the coefficients within 1e-3 of a half, {differ_total} rounded the other way")
    assert share <= 0.01


@pytest.mark.parametrize("size,T,q", CASES, ids=ids)
def test_files_are_header_plus_oracle_entropy_coding_of_the_kernels_coefficients(size, T, q):
    from realtime_video_amd import ops
    H, W = size
    rgb8 = torch.from_numpy(frames(size, T)).to(DEV)
    coeffs = ops.jpeg_coefficients(rgb8, q).cpu().numpy()
    out, offsets = ops.jpeg_encode(rgb8, q)
    assert out.dtype == torch.uint8 and offsets.dtype == torch.int64 and offsets.shape == (T + 1,) and int(offsets[-1]) == out.numel()
    got = files(out, offsets)
    for t in range(T):
        assert got[t] == jo.header(q, H, W) + jo.entropy_encode(coeffs[t], W) + jo.EOI, t
        check_file(got[t], H, W, q)
        if T > 1:                                                                        # a frame does not depend on its block
            alone = files(*ops.jpeg_encode(rgb8[t:t + 1], q))
            assert alone == [got[t]], t


def test_entropy_coder_corner_inputs():
    """Flat (EOB only), noise at quality 100 (stuffed 0xFF, AC sizes of 9 and more) and a single (7, 7) basis pattern (a zero run
    beyond 16: ZRL); each input's property is asserted on the kernel's own coefficients and bytes."""
    from realtime_video_amd import ops
    H, W = 48, 64
    k = np.arange(8)
    basis = np.outer(np.cos((2 * k + 1) * 7 * np.pi / 16), np.cos((2 * k + 1) * 7 * np.pi / 16))
    pattern = np.clip(128 + 100 * np.tile(basis, (H // 8, W // 8)), 0, 255).astype(np.uint8)
    # black / white noise: uniform bytes give luma coefficients of sigma 49, which do not reach 256 in a frame of this size
    binary = (np.random.default_rng(5).integers(0, 2, (H, W, 1)) * 255).astype(np.uint8)
    inputs = {"flat": (np.full((H, W, 3), 200, np.uint8), 90), "noise": (np.repeat(binary, 3, axis=2), 100),
              "basis": (np.repeat(pattern[:, :, None], 3, axis=2), 50)}
    for name, (img, q) in inputs.items():
        rgb8 = torch.from_numpy(img[None]).to(DEV)
        coeffs = ops.jpeg_coefficients(rgb8, q).cpu().numpy()[0]
        data, = files(*ops.jpeg_encode(rgb8, q))
        assert data == jo.header(q, H, W) + jo.entropy_encode(coeffs, W) + jo.EOI, name
        check_file(data, H, W, q)
        scan = data[629:-2]
        if name == "flat":
            assert not coeffs[..., 1:].any() and coeffs[..., :4, 0].all()
        elif name == "noise":
            assert b"\xff\x00" in scan and np.abs(coeffs[..., 1:]).max() >= 256
        else:
            luma = coeffs[:, :, :4]
            assert luma[..., 63].all() and not luma[..., 1:63].any()                     # 62 zeros in front of the last: 3 ZRL


def test_float_pixels_and_their_rgb8_give_identical_files():
    from realtime_video_amd import ops
    g = torch.Generator().manual_seed(3)
    px = ((torch.rand(2, 3, 24, 40, generator=g) - 0.5) * 2.4).to(DEV)
    assert px.min() < -1.05 and px.max() > 1.05
    a, ao = ops.jpeg_encode(px, 90)
    b, bo = ops.jpeg_encode(ops.pixels_to_rgb8(px), 90)
    assert torch.equal(ao, bo) and torch.equal(a, b)
    assert torch.equal(ops.jpeg_coefficients(px, 75), ops.jpeg_coefficients(ops.pixels_to_rgb8(px), 75))
    with pytest.raises(ValueError):
        ops.jpeg_encode(px.half())
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.jpeg_encode(px[..., :20, :].contiguous())


def test_small_out_cap_truncates_and_reports_the_true_sizes():
    from realtime_video_amd import ops
    rgb8 = torch.from_numpy(frames((48, 64), 3)).to(DEV)
    full, offsets = ops.jpeg_encode(rgb8, 90)
    total = full.numel()
    for cap in (total // 2 + 1, 700, 1):
        buf = torch.full((total + 256,), 0xAB, dtype=torch.uint8, device=DEV)
        out, got = ops.jpeg_encode(rgb8, 90, out=buf[:cap])
        assert torch.equal(got, offsets)
        assert torch.equal(buf[:cap], full[:cap]) and bool((buf[cap:] == 0xAB).all()), cap


def test_jpeg_frame_downloader():
    from realtime_video_amd import ops
    from realtime_video_amd.frames import JpegFrameDownloader
    H, W, T = 48, 64, 2
    flat = np.full((T, H, W, 3), 200, np.uint8)
    noise = np.stack([jo.image(H, W, "noise", seed=s) for s in (1, 2)])
    blocks = [torch.from_numpy(b).to(DEV).permute(0, 3, 1, 2).float().div(127.5).sub(1.0).contiguous()[None]
              for b in (flat, noise, frames((H, W), T))]
    expect = [files(*ops.jpeg_encode(b[0], 90)) for b in blocks]
    dl = JpegFrameDownloader(DEV, slots=2, quality=90)
    t0 = dl(blocks[0], frame_ids=[10, 11])
    t1 = dl(blocks[1], frame_ids=[12, 13], event=None)
    assert (t0, t1) == (0, 1) and dl.frame_ids(t0) == [10, 11] and dl.frame_ids(t1) == [12, 13]
    got0 = dl.fetch(t0)
    assert dl.topups == 0 and sum(len(f) for f in got0) < H * W * T // 2                 # the first estimate held
    assert [bytes(f) for f in got0] == expect[0] and all(isinstance(f, memoryview) for f in got0)
    got1 = dl.fetch(t1)
    assert dl.topups == 1 and sum(len(f) for f in got1) > H * W * T // 2                 # noise after flat: the rest was fetched
    assert [bytes(f) for f in got1] == expect[1]
    assert [bytes(f) for f in dl.fetch(t1)] == expect[1] and dl.topups == 1              # fetching again copies nothing
    t2 = dl(blocks[2], frame_ids=[14, 15])
    with pytest.raises(KeyError):
        dl.fetch(t0)
    assert [bytes(f) for f in dl.fetch(t2)] == expect[2] and dl.frame_ids(t2) == [14, 15] and dl.topups == 1
    for f in dl.fetch(t2):
        check_file(bytes(f), H, W, 90)
    with pytest.raises(KeyError):
        dl.fetch(t2 + 1)
    with pytest.raises(ValueError):
        dl(blocks[0][0])


def test_workload_shaped_frame_against_pil():
    """One 480 x 832 frame, smooth, quality 90 (no Python oracle at this size): PIL decodes it, and its PSNR and size against PIL's
    own encode of the same image are within the margins the CPU test records for the stream."""
    from realtime_video_amd import ops
    H, W = 480, 832
    src = jo.image(H, W, "smooth", seed=7)
    data, = files(*ops.jpeg_encode(torch.from_numpy(src[None]).to(DEV), 90))
    mine = jo.psnr(src, check_file(data, H, W, 90))
    b = io.BytesIO()
    Image.fromarray(src).save(b, format="JPEG", quality=90)
    pil = jo.psnr(src, np.asarray(Image.open(io.BytesIO(b.getvalue()))))
    ratio = len(data) / len(b.getvalue())
    print(f"480x832 smooth q90: {len(data)} B {mine:.3f} dB, PIL {len(b.getvalue())} B {pil:.3f} dB, deficit {pil - mine:+.3f} dB, ratio {ratio:.4f}")
    assert pil - mine <= jo.PARITY_PSNR_DEFICIT_DB and ratio <= jo.PARITY_SIZE_RATIO
