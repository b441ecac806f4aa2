"""CPU-only tests of the JPEG frame decoder: include/rtv_hip_jpeg_decode.h parses into tables of its own and leaves the pinned ABI
tables alone, the library exports what it declares, the host parser (rtv_jpeg_parse) agrees with PIL on what it accepts and
refuses the rest with a reason, the numpy oracle the GPU tests compare with (tests/jpeg_decode_oracle.py) is pinned to the
reference's decoder - PIL's `Image.open(...).convert("RGB")` (release_server.py:478), byte for byte - and the entropy kernel's
scheme, emulated serially by the host check program (csrc/jpeg_decode_hostcheck.cpp, built with -fsanitize=address,undefined and
run as a child process), reproduces the oracle's coefficients and stays inside its bounds on damaged files."""
import ctypes
import functools
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, JpegImagePlugin

import jpeg_decode_oracle as jd
import jpeg_oracle as jo
from realtime_video_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ header tables and exports
def test_decode_header_parses_into_its_own_tables():
    with open(os.path.join(ROOT, "include", _lib.JPEGDEC_HEADER)) as f:
        structs = dict(_lib.STRUCTS)
        protos = _lib.parse_header(f.read(), structs)
    assert {k: v[0] for k, v in protos.items()} == {k: v[0] for k, v in _lib.JPEGDEC_PROTOTYPES.items()}
    assert list(protos) == ["rtv_jpeg_parse", "rtv_jpeg_decode_arena_bytes", "rtv_jpeg_decode", "rtv_jpeg_decode_coefficients"]
    assert list(_lib.JPEGDEC_STRUCTS) == ["rtv_jpeg_desc"]
    desc = _lib.JPEGDEC_STRUCTS["rtv_jpeg_desc"]
    i, vp, sz, dp = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(desc)
    P = _lib.JPEGDEC_PROTOTYPES
    assert P["rtv_jpeg_parse"] == (i, [vp, sz, dp])
    assert P["rtv_jpeg_decode_arena_bytes"] == (sz, [dp, i])
    assert P["rtv_jpeg_decode"] == (i, [dp, vp, vp, i, i, vp, sz, vp, vp, vp])
    assert P["rtv_jpeg_decode_coefficients"] == (i, [dp, vp, i, vp, sz, vp, vp, vp, vp])
    assert ctypes.sizeof(desc) == 4496 and ctypes.sizeof(desc) % 16 == 0
    assert [f[0] for f in desc._fields_][:6] == ["height", "width", "components", "hsamp", "vsamp", "restart_interval"]
    # the pinned tables keep their values
    assert len(_lib.PROTOTYPES) == 90 and len(_lib.STRUCTS) == 14 and _lib.HEADERS == ("rtv_hip.h", "rtv_hip_lab.h")
    assert list(_lib.IO_PROTOTYPES) == ["rtv_frames_from_rgb8"] and _lib.IO_STRUCTS == {} and _lib.FRAMES_MAX == 16
    assert list(_lib.JPEG_PROTOTYPES) == ["rtv_jpeg_header", "rtv_jpeg_arena_bytes", "rtv_jpeg_out_bound", "rtv_jpeg_encode",
                                          "rtv_jpeg_coefficients"] and _lib.JPEG_STRUCTS == {}
    for other in (_lib.PROTOTYPES, _lib.IO_PROTOTYPES, _lib.JPEG_PROTOTYPES, _lib.declared_symbols()):
        assert not set(protos) & set(other)
    with open(os.path.join(ROOT, "include", "rtv_hip.h")) as f:
        assert _lib.ABI_VERSION == int([ln.split()[2] for ln in f if ln.startswith("#define RTV_ABI_VERSION")][0])


def test_library_exports_the_decode_functions_with_generated_prototypes():
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.JPEGDEC_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


# ------------------------------------------------------------------------------------------------------------------------ parser
PARSER_CASES = [("444", {}), ("422", {}), ("420", {}), ("grey", {}), ("420", dict(optimize=True)),
                ("422", dict(restart_marker_rows=1)), ("444", dict(restart_marker_blocks=3))]


@pytest.mark.parametrize("mode,kw", PARSER_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(v) or "plain")
def test_parser_agrees_with_pil(mode, kw):
    from realtime_video_amd import ops
    for H, W in jd.SIZES:
        data = jd.pil_file(jo.image(H, W, "smooth"), 90, mode, **kw)
        im = Image.open(io.BytesIO(data))
        info = ops.jpeg_parse(data)
        assert (info.W, info.H) == im.size and info.file_bytes == len(data)
        if mode == "grey":
            assert info.components == 1 and im.mode == "L" and info.sampling == (1, 1)
        else:
            assert info.components == 3 and im.mode == "RGB"
            assert info.sampling == {0: (1, 1), 1: (2, 1), 2: (2, 2)}[JpegImagePlugin.get_sampling(im)]
        hs, vs = info.sampling
        cols = -(-W // (8 * hs))
        want_ri = cols if "restart_marker_rows" in kw else kw.get("restart_marker_blocks", 0)
        assert info.restart_interval == want_ri
        d, o = info.desc, jd.parse(data)
        assert (d.mcu_cols, d.mcu_rows, d.blocks_per_mcu) == (cols, -(-H // (8 * vs)), hs * vs + info.components - 1)
        assert data[d.scan_offset:d.scan_offset + d.scan_bytes] == o["scan"] and data[d.scan_offset + d.scan_bytes:] == b"\xff\xd9"
        for c in range(info.components):
            assert list(d.quant[c]) == list(o["quant"][c])
        assert info.packed() == bytes(d) and len(info.packed()) == ops.JPEG_DESC_BYTES
        assert ops.jpeg_parse(bytearray(data)).packed() == info.packed() == ops.jpeg_parse(memoryview(data)).packed()


def _without_segment(data, marker, which=0):
    at, seen = 2, 0
    while True:
        m, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        if m == marker:
            if seen == which:
                return data[:at] + data[at + 2 + n:]
            seen += 1
        assert m != 0xDA
        at += 2 + n


def _patched_sof(data, offset, value):
    at = data.index(b"\xff\xc0")
    b = bytearray(data)
    b[at + 4 + offset] = value
    return bytes(b)


def test_parser_refusals_carry_a_reason():
    from realtime_video_amd import ops
    img = jo.image(24, 40, "smooth")
    good = jd.pil_file(img, 90, "420")
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=90, progressive=True)
    cmyk = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(cmyk, format="JPEG", quality=90)
    sof = good.index(b"\xff\xc0")
    adobe_rgb = good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + good[2:]
    dqt16 = bytearray(good)
    dqt16[good.index(b"\xff\xdb") + 4] |= 0x10
    cases = [(b.getvalue(), "progressive"), (cmyk.getvalue(), "4 components"), (good[:sof + 6], "truncated"), (good[:3], "not a JPEG"),
             (_without_segment(good, 0xC4), "Huffman table"), (_without_segment(good, 0xDB), "quantisation table"),
             (_patched_sof(good, 0, 12), "12-bit"), (_patched_sof(good, 7, 0x41), "sampling"), (bytes(dqt16), "16-bit"),
             (adobe_rgb, "Adobe"), (b"\x00" * 64, "not a JPEG"),
             (good[:2] + b"\xff\xc9" + good[sof + 2:], "arithmetic"),
             (_patched_sof(good, 1, 0x20), "4096"),                                   # height 0x2018
             (good[:-2] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + b"\x00\xff\xd9", "more than one scan")]
    for data, word in cases:
        with pytest.raises(ValueError, match=word):
            ops.jpeg_parse(data)
    assert ops.jpeg_parse(good).H == 24                                               # and the untouched file parses
    assert ops.jpeg_parse(good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + good[2:]).W == 40   # transform 1 = Y Cb Cr
    lib = _lib.load()
    assert lib.rtv_jpeg_parse(None, 10, None) != 0 and "null" in lib.rtv_last_error().decode()


def test_decode_refuses_before_any_launch():
    """Fake device addresses, never dereferenced: every case returns before a launch."""
    from realtime_video_amd import ops
    lib = _lib.load()
    info = ops.jpeg_parse(jd.pil_file(jo.image(24, 40, "smooth"), 90, "420"))
    D = _lib.JPEGDEC_STRUCTS["rtv_jpeg_desc"]
    need = ops.jpeg_decode_arena_bytes([info])
    assert need >= (4 * 6 + 2 * 6) * 128 and ops.jpeg_decode_arena_bytes([info, info]) == 2 * need
    assert lib.rtv_jpeg_decode_arena_bytes((D * 17)(), 17) == 0 and lib.rtv_jpeg_decode_arena_bytes((D * 1)(), 1) == 0

    def call(desc=info.desc, frame=0x10000, out=0x20000, T=1, subseq=0, arena=0x30000, arena_bytes=need, status=0x40000):
        descs = (D * 1)(desc)
        frames, outs = (ctypes.c_void_p * 1)(frame), (ctypes.c_void_p * 1)(out)
        r = lib.rtv_jpeg_decode(descs, frames, outs, T, subseq, arena, arena_bytes, status, None, None)
        return r, lib.rtv_last_error().decode()

    bad = D.from_buffer_copy(bytes(info.desc))
    bad.scan_bytes = info.file_bytes
    wide = D.from_buffer_copy(bytes(info.desc))
    wide.width = 5000
    for kw, word in [(dict(frame=None), "null"), (dict(out=None), "null"), (dict(arena=None), "null"), (dict(status=None), "null"),
                     (dict(T=17), "RTV_FRAMES_MAX"), (dict(T=-1), "RTV_FRAMES_MAX"), (dict(subseq=48), "subseq_bits"),
                     (dict(subseq=16), "subseq_bits"), (dict(arena_bytes=need - 1), "arena"), (dict(arena=0x30008), "aligned"),
                     (dict(frame=0x10004), "aligned"), (dict(desc=bad), "scan"), (dict(desc=wide), "4096")]:
        r, msg = call(**kw)
        assert r != 0 and msg.startswith("jpeg_decode") and word in msg, (kw, msg)
    assert lib.rtv_jpeg_decode(None, None, None, 0, 0, None, 0, None, None, None) == 0      # no frames is no error


def test_python_entry_points_refuse_cpu_tensors_and_non_bytes():
    from realtime_video_amd import ops
    from realtime_video_amd.frames import FrameUploader
    data = jd.pil_file(jo.image(8, 8, "smooth"), 90, "444")
    cpu = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_decode([cpu])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_decode_coefficients(cpu)
    info = ops.jpeg_parse(data)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.jpeg_decode_frames([info], [cpu], [torch.zeros(8, 8, 3, dtype=torch.uint8)], torch.zeros(1, dtype=torch.int32),
                               torch.zeros(4096, dtype=torch.uint8))
    for bad in (123, "text", None, [1, 2], np.zeros(4, np.uint8)):
        with pytest.raises(TypeError):
            ops.jpeg_parse(bad)
        with pytest.raises(TypeError):
            FrameUploader.push_jpeg(object.__new__(FrameUploader), bad)
    with pytest.raises(TypeError):
        ops.jpeg_decode([123])


# ------------------------------------------------------------------------------------------- the oracle, pinned to the reference
def test_entropy_round_trip_with_the_encoder_oracle():
    """jpeg_oracle.encode -> this oracle's entropy decode returns jpeg_oracle.coefficients exactly: the round trip is lossless."""
    for (H, W), kind, q in [((8, 8), "smooth", 90), ((16, 16), "noise", 50), ((24, 40), "smooth", 100), ((152, 24), "noise", 90)]:
        img = jo.image(H, W, kind)
        info = jd.parse(jo.encode(img, q))
        assert (info["H"], info["W"], info["hs"], info["vs"], info["ri"]) == (H, W, 2, 2, -(-W // 16))
        got, want = jd.entropy_decode(info), jd.from_encoder_layout(jo.coefficients(img, q)[0], H, W)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("size", jd.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", list(jd.MODES))
def test_oracle_pixels_equal_pil_byte_for_byte(mode, size):
    """Every stage is integer arithmetic, so equality is expected - and holds: the maximum absolute difference is 0 in every mode
    (profiles/r11_jpeg_decode_parity.txt)."""
    for kind in ("smooth", "noise"):
        for q in (50, 90, 100):
            data = jd.pil_file(jo.image(size[0], size[1], kind), q, mode)
            got, want = jd.decode(data), jd.pil_pixels(data)
            assert got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (kind, q, int(np.abs(got.astype(int) - want.astype(int)).max()))


def test_oracle_equals_pil_on_the_shared_files_and_fails_on_damage():
    for name, data in jd.valid_files().items():
        assert np.array_equal(jd.decode(data), jd.pil_pixels(data)), name
    fails = [n for n, d in jd.damaged_files().items() if _oracle_fails(d)]
    assert len(fails) >= 20                                               # the damaged set does damage


def _oracle_fails(data):
    try:
        jd.entropy_decode(jd.parse(data))
        return False
    except (jd.ScanError, jd.Refused):
        return True


# -------------------------------------------------------------------------------------------------------------------- host check
@functools.lru_cache(maxsize=None)
def _sanitized():
    return jd.build_hostcheck(sanitize=True)


@pytest.mark.parametrize("subseq_bits", [0, 32])
def test_host_check_emulated_rounds_give_the_oracles_coefficients(subseq_bits, tmp_path):
    """The kernel's rounds, emulated serially by the sanitised program over every valid file of this module, at the default
    subsequence length and at 32 bits (every boundary mid-symbol)."""
    prog = _sanitized()
    if prog is None:
        pytest.skip("no host compiler with -fsanitize=address,undefined")
    files = jd.valid_files()
    rc, err, out = jd.run_hostcheck(prog, files, subseq_bits, str(tmp_path))
    assert rc == 0 and err == "", err[-2000:]
    assert sorted(out) == sorted(files)
    rounds = {}
    for name, data in files.items():
        status, rounds[name], coef = out[name]
        assert status == 0, name
        assert np.array_equal(coef, jd.flat(jd.entropy_decode(jd.parse(data)))), name
    print("rounds:", {k: v for k, v in rounds.items() if v > 8})
    if subseq_bits == 32:
        assert max(rounds.values()) > 3                                   # the rounds were needed


def test_host_check_is_clean_on_the_damaged_set(tmp_path):
    """The fixed damaged set through the sanitised program: exit status 0, no sanitizer report, and a non-zero status word (or a
    refusal by the parser) wherever the oracle's serial decoder fails too."""
    prog = _sanitized()
    if prog is None:
        pytest.skip("no host compiler with -fsanitize=address,undefined")
    files = jd.damaged_files()
    assert len(files) >= 50
    for subseq_bits in (0, 32, 96):
        rc, err, out = jd.run_hostcheck(prog, files, subseq_bits, str(tmp_path))
        assert rc == 0 and err == "", err[-2000:]
        assert sorted(out) == sorted(files)
        for name, data in files.items():
            if _oracle_fails(data):
                assert out[name][0] == "refused" or out[name][0] != 0, name
        if subseq_bits == 0:
            first = {k: v[0] for k, v in out.items()}
        else:                                                             # the status word does not depend on the subsequence length
            assert {k: v[0] for k, v in out.items()} == first
    assert {v for v in first.values() if v != "refused"} >= {0, 1, 2, 8, 16}
