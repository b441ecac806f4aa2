"""CPU checks of the K smoothing of the fp8 attention shadow (tests/attn_fp8_center_cases.py): a zero centre changes no code, what
subtracting the channel means buys on keys with channel offsets and costs on Gaussian keys (rel-L2 of the restated attention
against the fp64 definition on the bf16 operands), the binding of include/rtv_hip_attn_fp8_center.h, and the refusal under context
parallelism."""
import ctypes

import pytest
import torch

import attn_fp8_cases as fc
import attn_fp8_center_cases as cc
from realtime_video_amd import _lib


def test_zero_centre_changes_no_code():
    k = cc.structured_k(130, 3, 16.0, seed=2)
    zero = torch.zeros(3, 128)
    for s in (1.0, 0.5, 3.0):
        assert torch.equal(cc.centered_codes(k, zero, s), fc.codes(k, s))
    v = cc.structured_k(130, 3, 0.0, seed=3)
    a, b = fc.empty_shadow(130, 3, fill=0xA5), fc.empty_shadow(130, 3, fill=0xA5)
    am_a, am_b = torch.zeros(2), torch.zeros(2)
    cc.quantize_kv_centered(k, v, *a, 5, 65, zero, 0.5, 2.0, am_a)
    fc.quantize_kv(k, v, *b, 5, 65, 0.5, 2.0, am_b)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(am_a, am_b)


def test_centred_codes_are_the_codes_of_the_difference():
    k = cc.structured_k(70, 2, 16.0, seed=4)
    c = cc.column_mean(k)
    got = fc.decode(cc.centered_codes(k, c, 1.0))
    want = (k.float() - c).clamp(-448, 448).to(fc.E4M3).double()
    assert torch.equal(got, want)
    # the offset channels are back on the fine part of the grid: |k - c| stays near N(0, 1)
    assert float((k.float() - c)[:, :, ::8].abs().max()) < 6.0 < float(k.float()[:, :, ::8].abs().min())


def test_mean_subtraction_halves_the_error_on_biased_keys():
    """Offset 16 on every 8th channel: rel-L2 of the smoothed attention <= 0.5 x that of the plain one (measured 0.31 x)."""
    q, k, v = cc.biased_operands(offset=16.0)
    plain, smooth = cc.rel_l2_pair(q, k, v, cc.column_mean(k))
    print(f"ATTN_FP8_CENTER biased offset=16 plain={plain:.4f} smooth={smooth:.4f} ratio={smooth / plain:.3f}")
    assert smooth <= 0.5 * plain


def test_mean_subtraction_is_neutral_on_gaussian_keys():
    """No offsets: <= 1.1 x the plain figure (measured 1.02 x)."""
    q, k, v = cc.biased_operands(offset=0.0)
    plain, smooth = cc.rel_l2_pair(q, k, v, cc.column_mean(k))
    print(f"ATTN_FP8_CENTER gaussian plain={plain:.4f} smooth={smooth:.4f} ratio={smooth / plain:.3f}")
    assert smooth <= 1.1 * plain


def test_a_stale_centre_still_gains():
    """The centre need not be the mean of the window attended: the mean of the first half of the rows gains the same 0.5 x."""
    q, k, v = cc.biased_operands(offset=16.0)
    plain, smooth = cc.rel_l2_pair(q, k, v, cc.column_mean(k[:100]))
    print(f"ATTN_FP8_CENTER biased offset=16 stale centre plain={plain:.4f} smooth={smooth:.4f} ratio={smooth / plain:.3f}")
    assert smooth <= 0.5 * plain


def test_binding_has_the_header_and_the_library_the_symbols():
    i, f, vp, i64, sz = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
    P = _lib.ATTN_FP8_CENTER_PROTOTYPES
    quant = _lib.ATTN_FP8_PROTOTYPES["rtv_attn_quantize_kv"]
    fwd = _lib.ATTN_FP8_PROTOTYPES["rtv_dit_forward_attn_fp8"]
    assert P == {
        "rtv_attn_kv_center_workspace_bytes": (sz, [i, i]),
        "rtv_attn_kv_center": (i, [vp, i64, i, i, i, i, i, vp, vp, sz, vp]),
        "rtv_attn_quantize_kv_centered": (quant[0], quant[1][:-1] + [vp] + quant[1][-1:]),
        "rtv_dit_forward_attn_fp8_centered": (fwd[0], fwd[1][:4] + [vp] + fwd[1][4:])}
    for n in [n for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "ATTN_FP8_CENTER_PROTOTYPES"]:
        assert not set(getattr(_lib, n)) & set(P), n
    # the tables the header stays out of are what they were
    assert len(_lib.PROTOTYPES) == 90 and len(_lib.STRUCTS) == 14 and len(_lib.ATTN_FP8_PROTOTYPES) == 4
    assert list(_lib.ATTN_FP8_STRUCTS) == ["rtv_attn_fp8_shadow"]
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    ws = lib.rtv_attn_kv_center_workspace_bytes
    assert ws(1, 1) == 512 and ws(256, 1) == 512 and ws(257, 5) == 2 * 5 * 512 and ws(32760, 40) == 128 * 40 * 512
    assert ws(0, 4) == 0 and ws(4, 0) == 0 and ws(-1, -1) == 0


P16 = 0x10000          # a 16-byte aligned non-null "device address": refusals never follow it


def test_refusals_need_no_gpu():
    lib = _lib.load()
    good = dict(k=P16, rs=256, row0=0, n0=10, row1=0, n1=0, H=2, center=P16, ws=P16, ws_bytes=1024)
    order = list(good)
    bad = [dict(k=0), dict(center=0), dict(ws=0), dict(k=P16 + 2), dict(center=P16 + 4), dict(ws=P16 + 8), dict(n0=0), dict(n0=-1),
           dict(H=0), dict(n1=-1), dict(row0=-1), dict(row1=-1, n1=3), dict(rs=248), dict(rs=260), dict(H=70000, rs=70000 * 128),
           dict(ws_bytes=1023), dict(n0=200, n1=57, ws_bytes=2047)]
    for kw in bad:
        a = dict(good, **kw)
        assert lib.rtv_attn_kv_center(*[a[n] for n in order], None) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_kv_center:"), kw
    qgood = dict(k=P16, v=P16, rs=256, row0=0, rows=10, H=2, k8=P16, v8t=P16, cache_rows=64, k_scale=1.0, v_scale=1.0, amax=0, center=P16)
    qorder = list(qgood)
    for kw in [dict(center=0), dict(center=P16 + 4), dict(k=0), dict(rows=0), dict(row0=60), dict(rs=250), dict(k_scale=0.0),
               dict(v_scale=float("nan")), dict(amax=P16 + 2)]:
        a = dict(qgood, **kw)
        assert lib.rtv_attn_quantize_kv_centered(*[a[n] for n in qorder], None) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_quantize_kv:"), kw


def test_smooth_k_refuses_context_parallelism():
    """enable_fp8_attention(smooth_k=True) under SimulatedContextParallel: the same refusal as the plain mode, before anything is
    allocated or the cache bookkeeping moves."""
    from realtime_video_amd.causal_model import CausalWanModel
    from realtime_video_amd.parallel import SimulatedContextParallel
    m = CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64)
    m.context_parallel = SimulatedContextParallel(2, "heads")
    assert m.enable_fp8_attention(smooth_k=True) is m and m._fp8_attention.mode.smooth
    kv = [{"k": torch.zeros(1, 64, 2, 128, dtype=torch.bfloat16), "v": torch.zeros(1, 64, 2, 128, dtype=torch.bfloat16),
           "global_end_index": 0, "local_end_index": 0}]
    with pytest.raises(RuntimeError, match="context parallelism"):
        m._fp8_attention.shadow(kv, True)
    assert "k8" not in kv[0] and m._fp8_attention.center is None
    with pytest.raises(RuntimeError, match="has not run yet"):
        m.fp8_attention_recenter(kv)
    m.enable_fp8_attention()
    assert not m._fp8_attention.mode.smooth
    with pytest.raises(RuntimeError, match="smooth_k=True"):
        m.fp8_attention_recenter(kv)
