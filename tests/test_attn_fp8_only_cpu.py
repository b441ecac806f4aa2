"""CPU checks of the e4m3-only KV cache (include/rtv_hip_attn_fp8_only.h): the binding carries the header's three declarations in a
table of its own, the pinned sizes of the other tables are unchanged, the built library exports the symbols, and
enable_fp8_attention(bf16_cache=False) refuses what it cannot run."""
import ctypes

import pytest

from realtime_video_amd import _lib


def test_binding_has_the_header_and_the_library_the_symbols():
    i, f, vp, i64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64
    P = _lib.ATTN_FP8_ONLY_PROTOTYPES
    S = _lib.STRUCTS
    cfg, w, st = (ctypes.POINTER(S[n]) for n in ("rtv_dit_config", "rtv_dit_weights", "rtv_dit_step"))
    sh = ctypes.POINTER(_lib.ATTN_FP8_STRUCTS["rtv_attn_fp8_shadow"])
    assert P == {
        # qkv, q_out, k8, cache_rows, k_scale, amax, cache_row0, M, d, num_heads, eps, wq, wk, rope_cs, F, gh, gw, start_frame,
        # row_offset, ring_lo, ring_size, ring_shift, stream
        "rtv_qk_norm_rope_k8": (i, [vp, vp, vp, i, f, vp, i, i, i, i, f, vp, vp, vp, i, i, i, i, i, i, i, i, vp]),
        # v_src, src_row_stride, rows, H, v8t, cache_rows, dst_row0, v_scale, amax, stream
        "rtv_attn_quantize_v_rows": (i, [vp, i64, i, i, vp, i, i, f, vp, vp]),
        "rtv_dit_forward_attn_fp8_only": (i, [cfg, w, st, sh, vp, ctypes.c_size_t, vp])}
    assert P["rtv_dit_forward_attn_fp8_only"] == _lib.ATTN_FP8_PROTOTYPES["rtv_dit_forward_attn_fp8"]
    for n in [n for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "ATTN_FP8_ONLY_PROTOTYPES"]:
        assert not set(getattr(_lib, n)) & set(P), n
    # nothing was added to the headers whose sizes other tests pin, and no struct came with the new one
    assert len(_lib.PROTOTYPES) == 90 and len(_lib.STRUCTS) == 14 and len(_lib.ATTN_FP8_PROTOTYPES) == 4
    assert list(_lib.ATTN_FP8_STRUCTS) == ["rtv_attn_fp8_shadow"]
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def _model():
    from realtime_video_amd.causal_model import CausalWanModel
    return CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64, device="cpu")


def test_enable_refuses_what_the_compact_cache_cannot_run():
    """smooth_k and context parallelism are ValueErrors at the call, and a refused call leaves the model's mode as it was."""
    m = _model()
    assert m.enable_fp8_attention(bf16_cache=False) is m and m._fp8_attention.only()
    assert m.enable_fp8_attention() is m and not m._fp8_attention.only()          # the default is the shadow mode
    state = (m._fp8_attention.mode, m._fp8_attention.mode.only, m._fp8_attention.mode.smooth, m._fp8_attention.mode.context_parallel)
    with pytest.raises(ValueError, match="smooth_k"):
        m.enable_fp8_attention(smooth_k=True, bf16_cache=False)
    with pytest.raises(ValueError, match="context parallelism"):
        m.enable_fp8_attention(context_parallel=True, bf16_cache=False)
    with pytest.raises(ValueError, match="finite and positive"):
        m.enable_fp8_attention(k_scale=0.0, bf16_cache=False)
    m.context_parallel = object()                                                  # a model with context_parallel set
    with pytest.raises(ValueError, match="context parallelism"):
        m.enable_fp8_attention(bf16_cache=False)
    assert state == (m._fp8_attention.mode, m._fp8_attention.mode.only, m._fp8_attention.mode.smooth, m._fp8_attention.mode.context_parallel)
    m.context_parallel = None
    m.enable_fp8_attention(k_scale=2.0, v_scale=0.5, bf16_cache=False)
    assert m._fp8_attention.mode[:2] == (2.0, 0.5) and m._fp8_attention.only()
    assert m.disable_fp8_attention() is m and not m._fp8_attention.only()


def test_cache_rows_helper_reads_both_kinds_of_dict():
    import torch

    from realtime_video_amd.causal_model import kv_cache_rows
    assert kv_cache_rows({"k": torch.zeros(1, 7, 2, 128), "v": torch.zeros(1, 7, 2, 128)}) == 7
    assert kv_cache_rows({"k8": None, "v8t": None, "rows": 9}) == 9
