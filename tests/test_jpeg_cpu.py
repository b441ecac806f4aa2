"""CPU-only tests of the JPEG frame encoder's host side: include/rtv_hip_jpeg.h parses into tables of its own and leaves the
pinned ABI tables alone, the library exports what it declares, rtv_jpeg_header writes what PIL reads as PIL's own stream
parameters, the entry points validate before they touch the device, the Python entry points refuse CPU tensors - and the
numpy oracle the GPU tests compare with (tests/jpeg_oracle.py) is pinned to the reference's encoder, PIL's
`save(format='JPEG', quality=q)` (release_server.py:972).

`PYTHONPATH=. python tests/test_jpeg_cpu.py` prints the parity table kept as profiles/r10_jpeg_parity.txt."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, JpegImagePlugin

import jpeg_oracle as jo
from realtime_video_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(4)]      # never dereferenced: every case returns before a launch


def test_jpeg_header_parses_into_its_own_tables():
    with open(os.path.join(ROOT, "include", _lib.JPEG_HEADER)) as f:
        protos = _lib.parse_header(f.read(), dict(_lib.STRUCTS))
    assert protos == _lib.JPEG_PROTOTYPES
    assert list(protos) == ["rtv_jpeg_header", "rtv_jpeg_arena_bytes", "rtv_jpeg_out_bound", "rtv_jpeg_encode", "rtv_jpeg_coefficients"]
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert protos["rtv_jpeg_header"] == (sz, [i, i, i, vp, sz])
    assert protos["rtv_jpeg_arena_bytes"] == (sz, [i, i, i])
    assert protos["rtv_jpeg_encode"] == (i, [vp, i, i, i, i, i, vp, sz, vp, sz, vp, vp])
    assert protos["rtv_jpeg_coefficients"] == (i, [vp, i, i, i, i, i, vp, sz, vp, vp])
    assert _lib.JPEG_STRUCTS == {}
    # the pinned tables keep their values
    assert len(_lib.PROTOTYPES) == 90 and len(_lib.STRUCTS) == 14 and _lib.HEADERS == ("rtv_hip.h", "rtv_hip_lab.h")
    assert list(_lib.IO_PROTOTYPES) == ["rtv_frames_from_rgb8"] and _lib.IO_STRUCTS == {} and _lib.FRAMES_MAX == 16
    for other in (_lib.PROTOTYPES, _lib.IO_PROTOTYPES, _lib.declared_symbols()):
        assert not set(protos) & set(other)
    with open(os.path.join(ROOT, "include", "rtv_hip.h")) as f:
        assert _lib.ABI_VERSION == int([ln.split()[2] for ln in f if ln.startswith("#define RTV_ABI_VERSION")][0])


def test_library_exports_the_jpeg_functions_with_generated_prototypes():
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.JPEG_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


# ----------------------------------------------------------------------------------------------------------------- the header
def segments(data):
    """A JPEG stream up to SOS -> [(marker, payload)] (T.81 B.1.1.4: 0xFF, marker, 16-bit length that counts itself)."""
    assert data[:2] == b"\xff\xd8"
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out


def huffman_tables(data):
    """{(class, id): (BITS, HUFFVAL)} of every table in the stream's DHT segments (one or several per segment)."""
    out = {}
    for marker, p in segments(data):
        at = 0
        while marker == 0xC4 and at < len(p):
            bits = list(p[at + 1:at + 17])
            out[(p[at] >> 4, p[at] & 15)] = (bits, list(p[at + 17:at + 17 + sum(bits)]))
            at += 17 + sum(bits)
    return out


def pil_jpeg(rgb8, q):
    b = io.BytesIO()
    Image.fromarray(rgb8).save(b, format="JPEG", quality=q)
    return b.getvalue()


def native_header(q, H, W):
    buf = ctypes.create_string_buffer(1024)
    n = _lib.load().rtv_jpeg_header(q, H, W, buf, len(buf))
    assert n > 0, _lib.load().rtv_last_error()
    return buf.raw[:n]


@pytest.mark.parametrize("size", [(24, 40), (480, 832)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("q", [1, 10, 50, 75, 90, 95, 100])
def test_header_is_what_pil_writes_and_reads(q, size):
    from realtime_video_amd import ops
    H, W = size
    head = native_header(q, H, W)
    assert head == jo.header(q, H, W) and head == ops.jpeg_header(q, H, W) and len(head) == 629
    im = Image.open(io.BytesIO(head + jo.EOI))
    assert im.size == (W, H) and im.mode == "RGB" and JpegImagePlugin.get_sampling(im) == 2           # 2 = 4:2:0
    pil = pil_jpeg(np.zeros((H, W, 3), np.uint8), q)
    ref = Image.open(io.BytesIO(pil))
    assert JpegImagePlugin.get_sampling(ref) == 2
    assert {k: list(v) for k, v in im.quantization.items()} == {k: list(v) for k, v in ref.quantization.items()}
    if q == 90:
        ql, _ = jo.quant_tables(90)
        assert list(ql[:8]) == [3, 2, 2, 3, 5, 8, 10, 12]
    mine, theirs = huffman_tables(head), huffman_tables(pil)
    assert sorted(mine) == [(0, 0), (0, 1), (1, 0), (1, 1)] and mine == theirs
    dri = [p for m, p in segments(head) if m == 0xDD]
    assert len(dri) == 1 and int.from_bytes(dri[0], "big") == -(-W // 16)


def test_header_refusals():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1024)
    for args, word in [((0, 24, 40, buf, 1024), "quality"), ((101, 24, 40, buf, 1024), "quality"), ((90, 20, 40, buf, 1024), "multiples of 8"),
                       ((90, 24, 0, buf, 1024), "positive"), ((90, 24, 40, None, 1024), "null"), ((90, 24, 40, buf, 628), "cap")]:
        assert lib.rtv_jpeg_header(*args) == 0 and word in lib.rtv_last_error().decode(), args
    assert lib.rtv_jpeg_header(90, 24, 40, buf, 629) == 629


# ------------------------------------------------------------------------------------------------------------------- refusals
def _encode(pixels=FAKE[0], rgb8=0, T=2, H=24, W=40, quality=90, arena=FAKE[1], arena_bytes=None, out=FAKE[2], out_cap=1 << 20,
            offsets=FAKE[3]):
    lib = _lib.load()
    if arena_bytes is None:
        arena_bytes = lib.rtv_jpeg_arena_bytes(max(T, 1), 24, 40)
    status = lib.rtv_jpeg_encode(pixels, rgb8, T, H, W, quality, arena, arena_bytes, out, out_cap, offsets, None)
    return status, lib.rtv_last_error().decode()


REFUSALS = [
    (dict(pixels=None), "null"), (dict(arena=None), "null"), (dict(out=None), "null"), (dict(offsets=None), "null"),
    (dict(T=-1), "positive"), (dict(H=0), "positive"), (dict(W=-8), "positive"),
    (dict(H=20), "multiples of 8"), (dict(W=36), "multiples of 8"),
    (dict(quality=0), "quality"), (dict(quality=101), "quality"),
    (dict(T=17, arena_bytes=1 << 30), "RTV_FRAMES_MAX"),
    (dict(arena_bytes=1024), "arena"),
    (dict(pixels=ctypes.c_void_p(0x10008)), "aligned"),
]


@pytest.mark.parametrize("kw,word", REFUSALS, ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_encode_refuses_before_any_launch(kw, word):
    status, msg = _encode(**kw)
    assert status != 0 and msg.startswith("jpeg_encode") and word in msg, (status, msg)


@pytest.mark.parametrize("kw,word", [c for c in REFUSALS if "out" not in c[0] and "offsets" not in c[0]] + [(dict(out=None), "null")],
                         ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_coefficients_refuses_before_any_launch(kw, word):
    lib = _lib.load()
    a = dict(pixels=FAKE[0], rgb8=0, T=2, H=24, W=40, quality=90, arena=FAKE[1], arena_bytes=None, out=FAKE[2])
    a.update(kw)
    if a["arena_bytes"] is None:
        a["arena_bytes"] = lib.rtv_jpeg_arena_bytes(max(a["T"], 1), 24, 40)
    status = lib.rtv_jpeg_coefficients(a["pixels"], a["rgb8"], a["T"], a["H"], a["W"], a["quality"], a["arena"], a["arena_bytes"],
                                       a["out"], None)
    msg = lib.rtv_last_error().decode()
    assert status != 0 and msg.startswith("jpeg_coefficients") and word in msg, (status, msg)


def test_misaligned_rgb8_is_not_refused_for_alignment_and_no_frames_is_no_error():
    assert _encode(T=0)[0] == 0
    assert _encode(T=0, pixels=None, arena=None, out=None, offsets=None)[0] == 0
    # rgb8 asks no alignment: the same odd address is refused for the next reason in line, not for alignment
    status, msg = _encode(pixels=ctypes.c_void_p(0x10001), rgb8=1, arena_bytes=1024)
    assert status != 0 and "arena" in msg and "aligned" not in msg


def test_arena_and_bound_sizes():
    lib = _lib.load()
    assert lib.rtv_jpeg_arena_bytes(0, 24, 40) == 0 and lib.rtv_jpeg_arena_bytes(17, 24, 40) == 0
    assert lib.rtv_jpeg_arena_bytes(1, 20, 40) == 0 and lib.rtv_jpeg_out_bound(1, 24, 36) == 0
    one, two = lib.rtv_jpeg_arena_bytes(1, 24, 40), lib.rtv_jpeg_arena_bytes(2, 24, 40)
    blocks = 2 * 3 * 6                                                       # 2 MCU rows of 3 MCUs of 6 blocks
    assert one >= blocks * 128 + blocks * 208 and two == 2 * one
    # every block at 1658 bits, every byte stuffed, plus header, markers and EOI
    assert lib.rtv_jpeg_out_bound(1, 24, 40) >= 629 + 2 * blocks * 208 + 2 + 2
    assert lib.rtv_jpeg_out_bound(3, 24, 40) == 3 * lib.rtv_jpeg_out_bound(1, 24, 40)


def test_python_entry_points_refuse_cpu_tensors():
    from realtime_video_amd import ops
    from realtime_video_amd.frames import JpegFrameDownloader
    for x in (torch.zeros(2, 3, 24, 40), torch.zeros(2, 24, 40, 3, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.jpeg_encode(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.jpeg_coefficients(x)
    with pytest.raises(ValueError):
        JpegFrameDownloader.__call__(object.__new__(JpegFrameDownloader), torch.zeros(3, 24, 40))
    with pytest.raises(ValueError):
        JpegFrameDownloader("cpu", quality=0)


# ---------------------------------------------------------------------------------- the oracle, pinned to the reference's encoder
PARITY_CASES = [(kind, size, q) for kind in ("smooth", "noise") for size in ((24, 40), (48, 64), (152, 24)) for q in (50, 90, 100)]


def parity(kind, size, q):
    """-> (bytes of the oracle's file, its PSNR against the source, bytes of PIL's file, its PSNR), both decoded by PIL."""
    src = jo.image(size[0], size[1], kind)
    mine, theirs = jo.encode(src, q), pil_jpeg(src, q)
    im = Image.open(io.BytesIO(mine))
    im.load()                                                                # raises on a stream PIL cannot decode to the end
    assert im.size == (size[1], size[0]) and im.mode == "RGB"
    return len(mine), jo.psnr(src, np.asarray(im)), len(theirs), jo.psnr(src, np.asarray(Image.open(io.BytesIO(theirs))))


def test_generator_is_the_recorded_one():
    """PIL at quality 90 on the fixed-seed images: the figures the parity table starts from."""
    n, _, pil_n, pil_psnr = parity("smooth", (24, 40), 90)
    assert pil_n == 1076 and round(pil_psnr, 2) == 26.30
    n, _, pil_n, pil_psnr = parity("noise", (48, 64), 90)
    assert pil_n == 3374 and round(pil_psnr, 2) == 12.48


@pytest.mark.parametrize("kind,size,q", PARITY_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_oracle_stream_matches_pil_in_quality_and_size(kind, size, q):
    """The margins are the measured worst case rounded up (0.05 dB, 1 %); beyond 0.5 dB or 1.10 the stream's design would be
    wrong - its expected cost over PIL's is one marker, the padding and one DC re-code per MCU row, and the 6-byte DRI."""
    n, mine, pil_n, pil = parity(kind, size, q)
    print(f"{kind} {size[0]}x{size[1]} q{q}: oracle {n} B {mine:.3f} dB, PIL {pil_n} B {pil:.3f} dB, "
          f"deficit {pil - mine:+.3f} dB, size ratio {n / pil_n:.4f}")
    assert jo.PARITY_PSNR_DEFICIT_DB <= 0.5 and jo.PARITY_SIZE_RATIO <= 1.10
    assert pil - mine <= jo.PARITY_PSNR_DEFICIT_DB
    assert n / pil_n <= jo.PARITY_SIZE_RATIO


def test_restart_markers_wrap_past_seven_and_the_stream_ends_with_eoi():
    data = jo.encode(jo.image(152, 24, "smooth"), 90)
    scan = data[len(jo.header(90, 152, 24)):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0x00]
    assert marks == [0xD0 + i % 8 for i in range(9)] + [0xD9] and data.endswith(jo.EOI)


if __name__ == "__main__":
    print("JPEG stream of include/rtv_hip_jpeg.h (tests/jpeg_oracle.py, float64) against PIL %s save(format='JPEG', quality=q),"
          % Image.__version__)
    print("both decoded by PIL; PSNR against the source image; fixed-seed images jpeg_oracle.image(H, W, kind)\n")
    print("image   size    q    oracle B   oracle dB    PIL B     PIL dB   deficit dB  size ratio")
    worst_db, worst_ratio = -1e9, 0.0
    for kind, size, q in PARITY_CASES:
        n, mine, pil_n, pil = parity(kind, size, q)
        worst_db, worst_ratio = max(worst_db, pil - mine), max(worst_ratio, n / pil_n)
        print(f"{kind:7s} {size[0]:3d}x{size[1]:<3d} {q:3d}  {n:8d}  {mine:10.3f}  {pil_n:7d}  {pil:9.3f}  {pil - mine:+10.3f}  {n / pil_n:10.4f}")
    print(f"\nworst PSNR deficit {worst_db:.3f} dB -> asserted {jo.PARITY_PSNR_DEFICIT_DB} dB; "
          f"worst size ratio {worst_ratio:.4f} -> asserted {jo.PARITY_SIZE_RATIO}")
