"""CPU tests of the TAEHV tiny-VAE encoder (realtime_video_amd/taehv.py TAEHVEncoder, csrc/taehv.hip): the loader's key set
against the reference module's manifest, the synthetic weights against the golden's checksum, a torch restatement of
demo_utils/taehv.py's encoder (streamed over calls, TPool folded into the stride-2 conv) against the golden, fold_tpool
against the two-layer form, the library's new symbols and a scratch-free compile of the kernels."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, rel_l2
from realtime_video_amd import _lib
from realtime_video_amd.taehv import ENC_MEMBLOCKS, TPOOLS, TAEHVDecoder, TAEHVEncoder, fold_tpool
from test_taehv_cpu import kernel_scratch_sizes


def golden_frames(H, W, T, seed):   # scripts/make_taehv_encoder_golden.py frames01()
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    return torch.rand(24, 3, H, W, generator=g)[:T]


def restate_encode(sd, x, state=None):
    """The TAEHV encoder (taehv.py:172-178) streamed over one call: x [T, 3, H, W] in [0, 1], T a multiple of 4 ->
    (latents [T / 4, 16, H / 8, W / 8], new state).  `state` = the nine MemBlock inputs of the previous frame ([64, h, w] each),
    None on a stream's first call.  Each TPool is folded into the stride-2 conv behind it (fold_tpool).  Runs on x's device in
    x's dtype; the full-resolution layer goes one frame pair at a time (memory of torch's im2col at 480 x 832)."""
    def conv(x, name, bias=True):
        return F.conv2d(x, sd[name + ".weight"].to(x), sd[name + ".bias"].to(x) if bias else None, padding=1)

    def down(x, s):
        tp, cv, stride = TPOOLS[s]
        wf = fold_tpool(sd[f"encoder.{tp}.conv.weight"], sd[f"encoder.{cv}.weight"], stride).to(x)
        if stride == 1:
            return F.conv2d(x, wf, stride=2, padding=1)
        return sum(F.conv2d(x[dt::2], wf[:, :, dt], stride=2, padding=1) for dt in range(2))

    assert x.shape[0] % 4 == 0
    x = torch.cat([down(F.relu(conv(x[i:i + 2], "encoder.0")), 0) for i in range(0, x.shape[0], 2)])
    new_state = []
    for k, idx in enumerate(ENC_MEMBLOCKS):
        if k in (3, 6):
            x = down(x, k // 3)
        prev = torch.zeros_like(x[:1]) if state is None else state[k][None].to(x)
        past = torch.cat([prev, x[:-1]])
        new_state.append(x[-1].clone())
        y = F.relu(conv(torch.cat([x, past], 1), f"encoder.{idx}.conv.0"))
        y = F.relu(conv(y, f"encoder.{idx}.conv.2"))
        x = F.relu(conv(y, f"encoder.{idx}.conv.4") + x)
    return conv(x, "encoder.17"), new_state


def test_loader_keys_match_reference_manifest():
    with open(os.path.join(GOLDEN, "taehv_encoder_manifest.json")) as f:
        man = json.load(f)
    spec = TAEHVEncoder.state_dict_spec()
    assert [[k, list(s)] for k, s in spec] == man["encoder"]
    with open(os.path.join(GOLDEN, "taehv_manifest.json")) as f:
        assert sorted(k for k, _ in spec) == json.load(f)["encoder_keys"]


def test_one_checkpoint_dict_loads_into_both_classes():
    sd = dict(TAEHVEncoder.random_state_dict(3), **TAEHVDecoder.random_state_dict(3))
    enc, dec = TAEHVEncoder("cpu"), TAEHVDecoder("cpu")
    enc.load_state_dict(sd)
    dec.load_state_dict(sd)
    assert enc._w is not None and dec._w is not None
    assert tuple(enc._t["encoder.0.w"].shape) == (64, 32) and not enc._t["encoder.0.w"][:, 27:].any()
    assert tuple(enc._t["down0"].shape) == (64, 18, 64) and tuple(enc._t["down2"].shape) == (64, 9, 64)
    assert tuple(enc._t["encoder.4.conv.0.w"].shape) == (64, 18, 64) and tuple(enc._t["encoder.17.w"].shape) == (16, 9, 64)
    with pytest.raises(KeyError):
        enc.load_state_dict({k: v for k, v in sd.items() if k != "encoder.17.bias"})
    with pytest.raises(KeyError):
        enc.load_state_dict(dict(sd, **{"encoder.99.weight": torch.zeros(1)}))
    with pytest.raises(ValueError):
        enc.load_state_dict(dict(sd, **{"encoder.3.weight": torch.zeros(64, 64, 1, 1)}))


def test_random_weights_reproduce_golden_checksum(golden):
    g = golden("taehv_encoder.pt")
    assert TAEHVEncoder.checksum(TAEHVEncoder.random_state_dict(g["seed"])) == g["checksum"]


@pytest.mark.parametrize("name", ["64x96_12", "56x88_9_fresh", "56x88_21_fresh"])
def test_restatement_reproduces_golden(golden, name):
    g = golden("taehv_encoder.pt")
    H, W, T, fresh = g["cases"][name]
    sd = TAEHVEncoder.random_state_dict(g["seed"])
    x = golden_frames(H, W, T, g["frame_seed"])
    if fresh:
        x = torch.cat([x[:1].expand(3, -1, -1, -1), x])      # the fresh-stream contract: frame 0 four times
    ref = g["latents"][name]
    with torch.no_grad():
        y, _ = restate_encode(sd, x)
    assert y.shape == ref.shape == (x.shape[0] // 4, 16, H // 8, W // 8)
    err = rel_l2(y, ref)
    print(f"restatement vs golden {name}: rel-L2 {err:.2e}, max-abs {float((y - ref).abs().max()):.2e}")
    assert err <= 1e-5
    # streaming over calls (state carried) is the same function: 12 = 4 + 8
    with torch.no_grad():
        full, _ = restate_encode(sd, x[:12])
        a, st = restate_encode(sd, x[:4])
        b, _ = restate_encode(sd, x[4:12], st)
    assert rel_l2(torch.cat([a, b]), full) <= 1e-6


@pytest.mark.parametrize("stride", [1, 2])
def test_fold_tpool_matches_two_layer_form(stride):
    g = torch.Generator().manual_seed(40 + stride)
    tp = torch.randn(64, 64 * stride, 1, 1, generator=g) / (64 * stride) ** 0.5
    cw = torch.randn(64, 64, 3, 3, generator=g) / 24.0
    x = torch.randn(4, 64, 14, 22, generator=g)
    ref = F.conv2d(F.conv2d(x.reshape(-1, 64 * stride, 14, 22), tp), cw, stride=2, padding=1)
    wf = fold_tpool(tp, cw, stride)
    if stride == 1:
        assert wf.shape == (64, 64, 3, 3)
        got = F.conv2d(x, wf, stride=2, padding=1)
    else:
        assert wf.shape == (64, 64, 2, 3, 3)
        got = sum(F.conv2d(x[dt::2], wf[:, :, dt], stride=2, padding=1) for dt in range(2))
    assert got.shape == ref.shape
    assert rel_l2(got, ref) <= 1e-5


def test_library_exports_taehv_encoder_symbols():
    lib = _lib.load()
    for s in ("rtv_taehv_enc_arena_bytes", "rtv_taehv_enc_state_slot", "rtv_taehv_encode", "rtv_taehv_enc_conv"):
        assert s in _lib.declared_symbols(lab=False) and hasattr(lib, s), s
    n = lib.rtv_taehv_enc_arena_bytes(480, 832, 12)
    print(f"TAEHV encoder arena at 480x832, 12 frames per call: {n / 1e9:.3f} GB (Wan encoder: "
          f"{lib.rtv_vae_enc_arena_bytes(480, 832) / 1e9:.3f} GB)")
    assert 0 < n < lib.rtv_vae_enc_arena_bytes(480, 832)
    assert lib.rtv_taehv_enc_arena_bytes(481, 832, 12) == 0 and lib.rtv_taehv_enc_arena_bytes(480, 836, 12) == 0
    assert lib.rtv_taehv_enc_arena_bytes(480, 832, 0) == 0 and lib.rtv_taehv_enc_arena_bytes(480, 832, 9) == 0
    off, C, H, W = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    slot_fn = lib.rtv_taehv_enc_state_slot
    prev_end = 0
    for slot in range(9):
        assert slot_fn(480, 832, slot, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)) == 0
        s = slot // 3
        assert (C.value, H.value, W.value) == (64, 240 >> s, 416 >> s)
        assert off.value >= prev_end and off.value % 256 == 0
        prev_end = off.value + C.value * H.value * W.value * 2
    assert prev_end < n
    # the carried state: nine 64-channel fp16 frames, three per resolution (50.3 MB at 480 x 832; every slice is a multiple of 256 B)
    assert prev_end == 3 * (240 * 416 + 120 * 208 + 60 * 104) * 64 * 2
    assert slot_fn(480, 832, 9, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)) != 0
    assert slot_fn(481, 832, 0, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W)) != 0


def test_taehv_encoder_kernels_use_no_scratch(tmp_path):
    names, scratch, remarks = kernel_scratch_sizes(tmp_path)
    assert len(names) == len(scratch), remarks[-4000:]
    # the first layer, the stride-2 gather form (..., HEAD 0, DOWN true) and the latent head (HEAD 2) of taehv_conv_kernel
    new = [n for n in names if "taehv_enc_first" in n or n.endswith("ELi0ELb1EEEvNS0_10ConvParamsE")
           or n.endswith("ELi2ELb0EEEvNS0_10ConvParamsE")]
    assert len(new) == 3, names
    assert all(s == 0 for n, s in zip(names, scratch) if n in new), list(zip(names, scratch))
