"""CPU tests of the TAEHV tiny-VAE decoder (opt-in fast decode, realtime_video_amd/taehv.py, csrc/taehv.hip): the loader's key
set against the reference module's manifest, the synthetic weights against the golden's checksum, a torch restatement of
demo_utils/taehv.py's decoder against the golden (the restatement the GPU tests evaluate at production size), the library's
new symbols, a scratch-free compile of the kernels and the arena layout of both halves against recorded values."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2
from realtime_video_amd import _lib
from realtime_video_amd.taehv import MEMBLOCKS, TGROWS, TAEHVDecoder

CSRC = os.path.join(os.path.dirname(GOLDEN), "..", "realtime_video_amd", "csrc")


def golden_latents(h, w, seed, T):   # scripts/make_taehv_golden.py latents()
    g = torch.Generator().manual_seed(seed + 1000 * h + w)
    return torch.randn(1, T, 16, h, w, generator=g)


def restate_decode(sd, z, state=None):
    """The TAEHV decoder (taehv.py:159-234) streamed over one call: z [T, 16, h, w] float -> (frames [4T, 3, 8h, 8w] in ~[0, 1],
    new state).  `state` = the nine MemBlock inputs of the previous frame ([C, H, W] each), None on a stream's first call.
    Runs on z's device in z's dtype; the last stage goes one frame at a time (memory of torch's im2col at 480 x 832)."""
    def conv(x, name, bias=True, pad=1):
        return F.conv2d(x, sd[name + ".weight"].to(x), sd[name + ".bias"].to(x) if bias else None, padding=pad)

    x = F.relu(conv(torch.tanh(z / 3) * 3, "decoder.1"))
    new_state = []
    for k, idx in enumerate(MEMBLOCKS):
        prev = torch.zeros_like(x[:1]) if state is None else state[k][None].to(x)
        past = torch.cat([prev, x[:-1]])
        new_state.append(x[-1].clone())
        y = F.relu(conv(torch.cat([x, past], 1), f"decoder.{idx}.conv.0"))
        y = F.relu(conv(y, f"decoder.{idx}.conv.2"))
        x = F.relu(conv(y, f"decoder.{idx}.conv.4") + x)
        if k % 3 == 2:
            tg, cv, cin, _cout, stride = TGROWS[k // 3]

            def grow(x):
                x = F.interpolate(x, scale_factor=2, mode="nearest")
                x = F.conv2d(x, sd[f"decoder.{tg}.conv.weight"].to(x))
                x = x.reshape(-1, cin, x.shape[-2], x.shape[-1])
                return conv(x, f"decoder.{cv}", bias=False)

            if k < 8:
                x = grow(x)
            else:
                x = torch.cat([conv(F.relu(grow(x[i:i + 1])), "decoder.22") for i in range(x.shape[0])])
    return x, new_state


def test_loader_keys_match_reference_manifest():
    with open(os.path.join(GOLDEN, "taehv_manifest.json")) as f:
        man = json.load(f)
    spec = TAEHVDecoder.state_dict_spec()
    assert [[k, list(s)] for k, s in spec] == man["decoder"]
    # a real taew2_1.pth: encoder keys (ignored) + a TGrow weight wider than the module's (patch_tgrow_layers keeps the last rows)
    sd = TAEHVDecoder.random_state_dict(3)
    wide = torch.randn(4 * 64, 64, 1, 1)
    sd["decoder.19.conv.weight"] = wide
    for k in man["encoder_keys"]:
        sd[k] = torch.zeros(1)
    patched = TAEHVDecoder.patch_tgrow_layers({k: v for k, v in sd.items() if not k.startswith("encoder.")})
    assert sorted(patched) == sorted(k for k, _ in spec)
    assert torch.equal(patched["decoder.19.conv.weight"], wide[-128:])
    assert {k: tuple(v.shape) for k, v in patched.items()} == dict(spec)
    dec = TAEHVDecoder("cpu")
    dec.load_state_dict(sd)                                 # encoder.* ignored, wide TGrow trimmed
    assert dec._w is not None and tuple(dec._t["up2"].shape) == (128, 9, 64)
    with pytest.raises(KeyError):
        dec.load_state_dict({k: v for k, v in sd.items() if k != "decoder.22.bias"})
    with pytest.raises(KeyError):
        dec.load_state_dict(dict(sd, **{"decoder.99.weight": torch.zeros(1)}))
    with pytest.raises(NotImplementedError):
        TAEHVDecoder("cpu", decoder_time_upscale=(False, True))
    with pytest.raises(NotImplementedError):
        TAEHVDecoder("cpu", decoder_space_upscale=(True, True, False))


def test_random_weights_reproduce_golden_checksum(golden):
    g = golden("taehv_decoder.pt")
    sd = TAEHVDecoder.random_state_dict(g["seed"])
    assert TAEHVDecoder.checksum(sd) == g["checksum"]
    assert golden("taehv_decoder_7x11.pt")["checksum"] == g["checksum"]


@pytest.mark.parametrize("name,h,w", [("taehv_decoder.pt", 8, 12), ("taehv_decoder_7x11.pt", 7, 11)])
def test_restatement_reproduces_golden(golden, name, h, w):
    g = golden(name)
    sd = TAEHVDecoder.random_state_dict(g["seed"])
    z = golden_latents(h, w, g["latent_seed"], g["T"])
    with torch.no_grad():
        y, _ = restate_decode(sd, z[0])
    ref = g["outputs"][f"{h}x{w}"][0]
    assert y.shape == (4 * g["T"], 3, 8 * h, 8 * w) and ref.shape[0] == 4 * g["T"] - 3
    # the golden is stored in fp16: compare the restatement rounded the same way (values in (0, 1): one fp16 ulp <= 4.9e-4)
    y3 = y[3:].half()
    err = rel_l2(y3.float(), ref.float())
    print(f"restatement vs golden {h}x{w}: rel-L2 {err:.2e}, max-abs {float((y3.float() - ref.float()).abs().max()):.2e}")
    assert err <= 1e-5
    assert float((y3.float() - ref.float()).abs().max()) <= 4.9e-4
    # streaming over calls (state carried) is the same function
    with torch.no_grad():
        a, st = restate_decode(sd, z[0, :2])
        b, _ = restate_decode(sd, z[0, 2:], st)
    assert rel_l2(torch.cat([a, b]), y) <= 1e-6


def test_library_exports_taehv_symbols():
    lib = _lib.load()
    for s in ("rtv_taehv_arena_bytes", "rtv_taehv_state_slot", "rtv_taehv_decode", "rtv_taehv_conv"):
        assert s in _lib.declared_symbols(lab=False) and hasattr(lib, s), s
    n = lib.rtv_taehv_arena_bytes(60, 104, 3)
    assert 0 < n < 1.5e9, n
    assert lib.rtv_taehv_arena_bytes(60, 104, 0) == 0 and lib.rtv_taehv_arena_bytes(0, 104, 3) == 0
    off, C, H, W = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    prev_end = 0
    for slot in range(9):
        assert lib.rtv_taehv_state_slot(60, 104, slot, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)) == 0
        s = slot // 3
        assert (C.value, H.value, W.value) == ((256, 128, 64)[s], 60 << s, 104 << s)
        assert off.value >= prev_end and off.value % 256 == 0
        prev_end = off.value + C.value * H.value * W.value * 2
    assert prev_end < n
    assert lib.rtv_taehv_state_slot(60, 104, 9, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)) != 0


def kernel_scratch_sizes(tmp_path):
    """Compile csrc/taehv.hip with the library's flags -> (function names, scratch bytes per lane, the compiler's remarks), from
    the kernel-resource-usage remarks.  Shared with tests/test_taehv_encoder_cpu.py."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    r = subprocess.run([hipcc, "--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-O3", "-std=c++17", "-fPIC", "-c",
                        os.path.join(CSRC, "taehv.hip"), "-o", str(tmp_path / "taehv.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    return names, scratch, r.stderr


def test_taehv_kernels_use_no_scratch(tmp_path):
    names, scratch, remarks = kernel_scratch_sizes(tmp_path)
    kernels = [n for n in names if "taehv" in n]
    assert len(kernels) >= 4 and len(names) == len(scratch), remarks[-4000:]
    assert all(s == 0 for n, s in zip(names, scratch) if "taehv" in n), list(zip(names, scratch))


# What the four layout functions returned before the decoder's and the encoder's layouts were folded into one: Python holds
# state views at these offsets and sizes its arenas by these totals.  Literals on purpose - not to be regenerated from the library.
DEC_ARENA = {(7, 11, 3): 7860480, (8, 12, 6): 16306432, (60, 104, 3): 636979456}
ENC_ARENA = {(56, 88, 12): 6673408, (64, 96, 12): 8319232, (480, 832, 12): 540733696}
DEC_SLOTS = {
    (7, 11): [(0, 256, 7, 11), (39424, 256, 7, 11), (78848, 256, 7, 11), (118272, 128, 14, 22), (197120, 128, 14, 22),
              (275968, 128, 14, 22), (354816, 64, 28, 44), (512512, 64, 28, 44), (670208, 64, 28, 44)],
    (60, 104): [(0, 256, 60, 104), (3194880, 256, 60, 104), (6389760, 256, 60, 104), (9584640, 128, 120, 208),
                (15974400, 128, 120, 208), (22364160, 128, 120, 208), (28753920, 64, 240, 416), (41533440, 64, 240, 416),
                (54312960, 64, 240, 416)],
}
ENC_SLOTS = {
    (56, 88): [(0, 64, 28, 44), (157696, 64, 28, 44), (315392, 64, 28, 44), (473088, 64, 14, 22), (512512, 64, 14, 22),
               (551936, 64, 14, 22), (591360, 64, 7, 11), (601344, 64, 7, 11), (611328, 64, 7, 11)],
    (480, 832): [(0, 64, 240, 416), (12779520, 64, 240, 416), (25559040, 64, 240, 416), (38338560, 64, 120, 208),
                 (41533440, 64, 120, 208), (44728320, 64, 120, 208), (47923200, 64, 60, 104), (48721920, 64, 60, 104),
                 (49520640, 64, 60, 104)],
}


def test_arena_layout_is_pinned():
    from realtime_video_amd.taehv import arena_bytes, enc_arena_bytes

    def slots(fn, a, b):
        off, C, H, W = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        out = []
        for i in range(9):
            _lib.call(fn, a, b, i, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W))
            out.append((off.value, C.value, H.value, W.value))
        return out

    assert {k: arena_bytes(*k) for k in DEC_ARENA} == DEC_ARENA
    assert {k: enc_arena_bytes(*k) for k in ENC_ARENA} == ENC_ARENA
    assert {k: slots("rtv_taehv_state_slot", *k) for k in DEC_SLOTS} == DEC_SLOTS
    assert {k: slots("rtv_taehv_enc_state_slot", *k) for k in ENC_SLOTS} == ENC_SLOTS
