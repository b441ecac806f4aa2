"""CPU-only tests of the pixel input path's plumbing: include/rtv_hip_io.h parses into tables of its own and leaves the pinned
ABI tables alone, the library exports what it declares, rtv_frames_from_rgb8 validates before it touches the device, and the
Python entry points refuse CPU frames (no CPU fallback)."""
import ctypes
import os

import pytest
import torch

from realtime_video_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_IN, FAKE_OUT = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)     # never dereferenced: every case returns before a launch


def test_io_header_parses_into_its_own_tables():
    with open(os.path.join(ROOT, "include", _lib.IO_HEADER)) as f:
        protos = _lib.parse_header(f.read(), dict(_lib.STRUCTS))
    assert protos == _lib.IO_PROTOTYPES and list(protos) == ["rtv_frames_from_rgb8"]
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert protos["rtv_frames_from_rgb8"] == (i, [vp, vp, ctypes.c_int64, i, i, i, vp, i, i, i, i, vp])
    assert _lib.IO_STRUCTS == {} and _lib.FRAMES_MAX == 16
    # the pinned tables of the two ABI headers keep their values
    assert len(_lib.PROTOTYPES) == 90 and len(_lib.STRUCTS) == 14 and _lib.HEADERS == ("rtv_hip.h", "rtv_hip_lab.h")
    assert not set(_lib.IO_PROTOTYPES) & set(_lib.PROTOTYPES)
    assert not set(_lib.IO_PROTOTYPES) & set(_lib.declared_symbols())


def test_library_exports_the_io_functions_with_generated_prototypes():
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.IO_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def _call(rgb8=FAKE_IN, slots=None, stride=20 * 28 * 3, T=2, Hin=20, Win=28, out=FAKE_OUT, out_T=2, out_t0=0, H=24, W=40):
    lib = _lib.load()
    arr = (ctypes.c_int * len(slots))(*slots) if slots is not None else None
    status = lib.rtv_frames_from_rgb8(rgb8, arr, stride, T, Hin, Win, out, out_T, out_t0, H, W, None)
    return status, lib.rtv_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(rgb8=None), "null"), (dict(out=None), "null"),
    (dict(T=-1), "positive"), (dict(Hin=0), "positive"), (dict(Win=-3), "positive"), (dict(H=0), "positive"), (dict(W=0), "positive"),
    (dict(H=20), "multiples of 8"), (dict(W=36), "multiples of 8"),
    (dict(out=ctypes.c_void_p(0x20008)), "16-byte aligned"),
    (dict(T=17, out_T=17), "RTV_FRAMES_MAX"),
    (dict(out_t0=1), "out_T"), (dict(out_t0=-1), "out_T"),
    (dict(stride=-1), "stride"), (dict(slots=[0, -1]), "slot"),
    (dict(Hin=40 * 24, Win=40 * 40, stride=0), "downscale"),
], ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else None)
def test_entry_point_refuses_before_any_launch(kw, word):
    status, msg = _call(**kw)
    assert status != 0 and msg.startswith("frames_from_rgb8") and word in msg, (status, msg)


def test_no_frames_is_not_an_error():
    assert _call(T=0)[0] == 0
    assert _call(T=0, rgb8=None, out=None)[0] == 0


def test_python_entry_points_refuse_cpu_frames():
    from realtime_video_amd import ops
    from realtime_video_amd.vae_encoder import encode_video_latent
    u8 = torch.zeros(2, 20, 28, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frames_from_rgb8(u8, (24, 40))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encode_video_latent(lambda *a, **k: pytest.fail("the encoder must not run"), [None] * 55, frames=u8, height=24, width=40)


def test_session_refuses_a_mixed_queue_without_touching_the_device():
    """The kind of a block's frames is fixed by the first queued one; the check comes before any upload."""
    from collections import deque
    from realtime_video_amd.session import GenerationSession
    sess = object.__new__(GenerationSession)
    sess.frame_queue, sess._queue_is_u8, sess.uploader = deque(), False, None
    sess.push_frame(torch.zeros(3, 8, 8, dtype=torch.float16))
    with pytest.raises(ValueError, match="all uint8"):
        sess.push_frame(torch.zeros(8, 8, 3, dtype=torch.uint8))
