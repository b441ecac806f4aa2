"""CPU checks of the code exchange on the e4m3-only KV cache (include/rtv_hip_attn_fp8_only_cp.h): the restated staging layout and
commit of tests/attn_fp8_only_cp_cases.py against the packers tests/attn_fp8_cases.py already restates, the binding table of the
new header, and the enable matrix of enable_fp8_attention(bf16_cache=False, context_parallel="codes")."""
import ctypes

import numpy as np
import pytest
import torch

import attn_fp8_cases as fc
import attn_fp8_only_cp_cases as cc
from realtime_video_amd import _lib


def test_slot_restatement_agrees_with_the_older_one():
    assert [cc.slot(k) for k in range(64)] == [fc.slot(k) for k in range(64)] and sorted(cc.SLOT.tolist()) == list(range(64))


@pytest.mark.parametrize("name", list(cc.COMMIT_CASES))
def test_segments_of_the_cases(name):
    M, world, cache_rows, row0, ring = cc.COMMIT_CASES[name]
    seg = cc.segments(row0, M, ring)
    assert seg == cc.COMMIT_SEGMENTS[name] and sum(n for _, n in seg) == M
    assert all(0 <= p and p + n <= cache_rows for p, n in seg)
    assert len(set(cc.physical_rows(row0, M, ring).tolist())) == M          # no two rows of a block share a physical row


@pytest.mark.parametrize("H", [2, 5])
@pytest.mark.parametrize("name", list(cc.COMMIT_CASES))
def test_commit_of_a_staging_built_shard_by_shard_equals_direct_placement(name, H):
    """bf16 K / V rows -> codes (fc.codes) -> staged shard by shard, later shards first -> restated commit; against the rows placed
    in a bf16 cache at their physical rows and quantised there segment by segment with fc.quantize_kv.  Sentinel bytes included."""
    M, world, cache_rows, row0, ring = cc.COMMIT_CASES[name]
    g = torch.Generator().manual_seed(M + H)
    k, v = (torch.randn(M, H, 128, generator=g) * 3).bfloat16(), (torch.randn(M, H, 128, generator=g) * 3).bfloat16()
    k_scale, v_scale = 2.0, 0.5
    kc, vc = fc.codes(k, k_scale).numpy().reshape(M, -1), fc.codes(v, v_scale).numpy().reshape(M, -1)
    kv8 = cc.empty_staging(M, H, world)
    S = M // world
    for r in reversed(range(world)):
        cc.stage(kv8, kc[r * S:(r + 1) * S], vc[r * S:(r + 1) * S], r * S)
    assert not (kv8 == cc.SENTINEL).all(axis=-1).any(), "a staged row was left out"
    sk, sv = cc.staged_rows(kv8)
    assert np.array_equal(sk, kc) and np.array_equal(sv, vc)
    # a rank's segment is one contiguous message: K rows then V rows
    flat = kv8.reshape(world, -1)
    assert np.array_equal(flat[1, :S * H * 128], kc[S:2 * S].reshape(-1)) and np.array_equal(flat[1, S * H * 128:], vc[S:2 * S].reshape(-1))
    k8, v8t = cc.empty_cache(cache_rows, H)
    cc.commit(kv8, k8, v8t, row0, ring)

    kcache, vcache = (torch.zeros(cache_rows, H, 128, dtype=torch.bfloat16) for _ in range(2))
    k8_ref, v8t_ref = fc.empty_shadow(cache_rows, H, fill=cc.SENTINEL)
    src = 0
    for p0, n in cc.segments(row0, M, ring):
        kcache[p0:p0 + n], vcache[p0:p0 + n] = k[src:src + n], v[src:src + n]
        fc.quantize_kv(kcache, vcache, k8_ref, v8t_ref, p0, n, k_scale, v_scale)
        src += n
    assert np.array_equal(k8, k8_ref.numpy()) and np.array_equal(v8t, v8t_ref.numpy())
    p = cc.physical_rows(row0, M, ring)
    assert np.array_equal(cc.ungather_v(v8t, p).reshape(M, -1), vc)
    outside = np.setdiff1d(np.arange(cache_rows), p)
    assert (k8[outside] == cc.SENTINEL).all() and (cc.ungather_v(v8t, outside) == cc.SENTINEL).all()


def test_binding_has_the_header_and_the_library_the_symbols():
    i, f, vp, sz = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    P = _lib.ATTN_FP8_ONLY_CP_PROTOTYPES
    S = _lib.STRUCTS
    cfg, w, st = (ctypes.POINTER(S[n]) for n in ("rtv_dit_config", "rtv_dit_weights", "rtv_dit_step"))
    sh = ctypes.POINTER(_lib.ATTN_FP8_STRUCTS["rtv_attn_fp8_shadow"])
    assert P == {
        # qkv, kv8, world, row_begin, row_count, k_scale, v_scale, amax, d, num_heads, eps, wk, rope_cs, F, gh, gw, start_frame, stream
        "rtv_attn_fp8_stage_kv8": (i, [vp, vp, i, i, i, f, f, vp, i, i, f, vp, vp, i, i, i, i, vp]),
        # kv8, world, M, H, k8, v8t, cache_rows, cache_row0, ring_lo, ring_size, ring_shift, stream
        "rtv_attn_fp8_commit_kv8": (i, [vp, i, i, i, vp, vp, i, i, i, i, i, vp]),
        # cfg, w, step, layer, parts, world, kv8, shadow, workspace, workspace_bytes, stream
        "rtv_dit_layer_proj_attn_fp8_only": (i, [cfg, w, st, i, i, i, vp, sh, vp, sz, vp]),
        # cfg, step, layer, world, kv8, shadow, stream
        "rtv_dit_commit_block_attn_fp8_only": (i, [cfg, st, i, i, vp, sh, vp]),
        # cfg, w, step, layer, world, kv8, shadow, workspace, workspace_bytes, stream
        "rtv_dit_layer_rest_attn_fp8_only": (i, [cfg, w, st, i, i, vp, sh, vp, sz, vp])}
    for n in [n for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "ATTN_FP8_ONLY_CP_PROTOTYPES"]:
        assert not set(getattr(_lib, n)) & set(P), n
    # nothing was added to the headers whose sizes other tests pin, and no struct came with the new one
    assert len(_lib.PROTOTYPES) == 90 and len(_lib.STRUCTS) == 14 and len(_lib.ATTN_FP8_ONLY_PROTOTYPES) == 3
    assert len(_lib.ATTN_FP8_CP_PROTOTYPES) == 4 and list(_lib.ATTN_FP8_STRUCTS) == ["rtv_attn_fp8_shadow"]
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def _model():
    from realtime_video_amd.causal_model import CausalWanModel
    return CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64, device="cpu")


def _state(m):
    mode = m._fp8_attention.mode
    return (mode, mode.only, mode.smooth, mode.context_parallel)


def test_enable_matrix():
    """"codes" is accepted with bf16_cache=False - with and without a context_parallel object on the model -, is a ValueError without
    it, every refusal of the older modes is what it was, and a refused call leaves the mode as it was."""
    from realtime_video_amd.parallel import SimulatedContextParallel
    m = _model()
    assert m.enable_fp8_attention(bf16_cache=False, context_parallel="codes") is m
    fa = m._fp8_attention
    assert fa.only() and fa.cp_codes() and fa.mode.context_parallel == "codes" and fa.mode.smooth is False
    m.context_parallel = SimulatedContextParallel(2, "rows")
    m.enable_fp8_attention(k_scale=2.0, v_scale=0.5, bf16_cache=False, context_parallel="codes")
    assert fa.cp_codes() and fa.mode[:2] == (2.0, 0.5)
    state = _state(m)
    for kwargs, match in [(dict(context_parallel="codes"), "bf16_cache=False"),                               # the bf16 cache kept
                          (dict(context_parallel="codes", bf16_cache=True), "bf16_cache=False"),
                          (dict(context_parallel="rows", bf16_cache=False), "False, True or \"codes\""),          # not a value
                          (dict(context_parallel="codes", bf16_cache=False, smooth_k="codes"), "smooth_k"),
                          (dict(context_parallel="codes", bf16_cache=False, smooth_k=True), "smooth_k"),
                          (dict(context_parallel=True, bf16_cache=False), "context parallelism"),
                          (dict(bf16_cache=False), "context parallelism"),                                    # a model with context_parallel set
                          (dict(context_parallel=True, smooth_k=True), "smooth_k"),
                          (dict(context_parallel="codes", bf16_cache=False, k_scale=0.0), "finite and positive")]:
        with pytest.raises(ValueError, match=match):
            m.enable_fp8_attention(**kwargs)
        assert _state(m) == state, kwargs
    m.context_parallel = None
    with pytest.raises(ValueError, match="context parallelism"):
        m.enable_fp8_attention(context_parallel=True, bf16_cache=False)
    assert _state(m) == state
    # the older values keep their meaning
    assert m.enable_fp8_attention(context_parallel=True) is m and fa.mode.context_parallel is True and not fa.only() and not fa.cp_codes()
    assert m.enable_fp8_attention(bf16_cache=False) is m and fa.mode.context_parallel is False and fa.only() and not fa.cp_codes()
    assert m.disable_fp8_attention() is m and not fa.cp_codes()


def test_simulated_gather_of_codes_is_a_no_op():
    from realtime_video_amd.parallel import ContextParallel, SimulatedContextParallel
    kv8 = torch.arange(2 * 2 * 3 * 128, dtype=torch.int64).to(torch.uint8).view(2, 2, 3, 128)
    before = kv8.clone()
    cp = SimulatedContextParallel(2, "rows")
    assert cp.gather_codes(kv8) is None
    pend = cp.gather_codes(kv8, async_op=True)
    pend.wait()
    assert torch.equal(kv8, before) and hasattr(ContextParallel, "gather_codes")
