"""CPU checks of K smoothing on the e4m3-only KV cache (include/rtv_hip_attn_fp8_only_center.h): the recentre arithmetic of
tests/attn_fp8_only_center_cases.py on every code, what a centre taken from the codes buys and what the second rounding of the
rows recentred in place costs (rel-L2 of the restated attention against the fp64 definition on the bf16 operands), the binding of
the header, and the refusals that need no GPU."""
import ctypes
import math

import pytest
import torch

import attn_fp8_cases as fc
import attn_fp8_center_cases as cc
import attn_fp8_only_center_cases as oc
from realtime_video_amd import _lib

K_SCALES = [1.0, 2.0, 0.5, 0.3, 1.7, 1.0 / 3.0, 3.1e-3, 97.0, 1e4]
CENTRES = [0.0, 16.0, -3.3]
ALL = torch.arange(256, dtype=torch.uint8).view(256, 1, 1)


@pytest.mark.parametrize("k_scale", K_SCALES)
def test_recentre_arithmetic_on_every_code(k_scale):
    nan = oc.is_nan_code(ALL)
    assert int(nan.sum()) == 2 and bool(nan[0x7F]) and bool(nan[0xFF])
    for c in CENTRES:
        c_old = torch.full((1, 1), c)
        # the same centre: every non-NaN code is kept but -0, which becomes +0; NaN stays NaN
        same, t = oc.recentered(ALL, c_old, c_old, k_scale)
        want = ALL.clone()
        want[0x80] = 0x00
        assert torch.equal(same, want), (k_scale, c)
        assert bool(torch.isnan(t[nan]).all()) and bool(oc.is_nan_code(same[nan]).all())
        for c2 in CENTRES:
            c_new = torch.full((1, 1), c2)
            moved, t = oc.recentered(ALL, c_old, c_new, k_scale)
            assert torch.equal(moved[nan], ALL[nan]) and not bool(oc.is_nan_code(moved[~nan]).any())
            # the distance from x + delta is e4m3's half step at |t| / k_scale (or the clamp)
            s64 = float(torch.tensor(k_scale, dtype=torch.float32))
            y = (t[~nan].double() / s64).clamp(-448, 448)
            got = fc.decode(moved[~nan])
            ulp = torch.maximum(torch.exp2(torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -6))) - 3), torch.tensor(2.0 ** -9, dtype=torch.float64))
            assert bool(((got - y).abs() <= 0.5 * ulp * (1 + 2.0 ** -20)).all()), (k_scale, c, c2)
            # and the amax rule ignores the NaNs
            am = torch.zeros(2)
            oc.recenter_rows(ALL.clone(), 0, 256, c_old, c_new, k_scale, am)
            assert float(am[0]) == float(t[~nan].abs().max()) and float(am[1]) == 0.0


def test_recentre_in_pieces_equals_one_call():
    g = torch.Generator().manual_seed(0)
    k8 = torch.randint(0, 256, (200, 3, 128), generator=g, dtype=torch.uint8)
    c_old, c_new = torch.randn(3, 128, generator=g), torch.randn(3, 128, generator=g) * 4
    one = oc.recenter_rows(k8.clone(), 5, 150, c_old, c_new, 0.5)
    two = oc.recenter_rows(oc.recenter_rows(k8.clone(), 70, 85, c_old, c_new, 0.5), 5, 65, c_old, c_new, 0.5)
    assert torch.equal(one, two) and torch.equal(one[:5], k8[:5]) and torch.equal(one[155:], k8[155:])


def test_centre_from_the_codes_halves_the_error_on_biased_keys():
    """cc.biased_operands(offset=16), seeds 0-2: fresh codes centred under the mean of the plain codes reach at most half the plain
    error - the criterion of test_mean_subtraction_halves_the_error_on_biased_keys (measured ratio 0.32); and the code mean is as
    good a centre as the bf16 mean."""
    for seed in range(3):
        q, k, v = cc.biased_operands(offset=16.0, seed=seed)
        plain, fresh, moved, center = oc.rel_l2_triple(q, k, v)
        _, bf16_mean = cc.rel_l2_pair(q, k, v, cc.column_mean(k))
        print(f"ATTN_FP8_ONLY_CENTER biased offset=16 seed={seed} plain={plain:.4f} fresh={fresh:.4f} (bf16 mean {bf16_mean:.4f}) "
              f"ratio={fresh / plain:.3f}")
        assert fresh <= 0.5 * plain
        # every code lies within e4m3's half step of its key (2^-4 relative, 2^-10 below the normals), and so do the means
        assert bool(((center.double() - k.double().mean(0)).abs() <= 2.0 ** -4 * k.double().abs().mean(0) + 2.0 ** -10).all())


@pytest.mark.parametrize("offset", [16.0, 4.0, 0.0])
def test_rows_recentred_in_place_stay_within_sqrt2_of_the_plain_error(offset):
    """The rows a recentre finds in the cache keep the error of their first rounding and take a second one under the new centre,
    whose step is at most the first one's (|k - c| <= |k| up to the centre's own noise): two roundings of at most the same step
    add at most in quadrature, so at most sqrt(2) x the plain error.  Measured: 1.00 - 1.10."""
    for seed in range(3):
        q, k, v = cc.biased_operands(offset=offset, seed=seed)
        plain, fresh, moved, _ = oc.rel_l2_triple(q, k, v)
        print(f"ATTN_FP8_ONLY_CENTER offset={offset:g} seed={seed} plain={plain:.4f} fresh={fresh:.4f} moved={moved:.4f} "
              f"moved/plain={moved / plain:.3f}")
        assert moved <= math.sqrt(2.0) * plain


def test_binding_has_the_header_and_the_library_the_symbols():
    i, f, vp, sz = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    P = _lib.ATTN_FP8_ONLY_CENTER_PROTOTYPES
    rope = _lib.ATTN_FP8_ONLY_PROTOTYPES["rtv_qk_norm_rope_k8"]
    fwd = _lib.ATTN_FP8_CENTER_PROTOTYPES["rtv_dit_forward_attn_fp8_centered"]
    assert P == {
        "rtv_qk_norm_rope_k8_centered": (rope[0], rope[1][:-1] + [vp] + rope[1][-1:]),
        "rtv_attn_k8_center": (i, [vp, i, i, i, i, i, i, f, vp, vp, vp, sz, vp]),
        "rtv_attn_k8_recenter": (i, [vp, i, i, i, i, f, vp, vp, vp, vp]),
        "rtv_dit_forward_attn_fp8_only_centered": fwd}
    for n in [n for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "ATTN_FP8_ONLY_CENTER_PROTOTYPES"]:
        assert not set(getattr(_lib, n)) & set(P), n
    # the tables the header stays out of are what they were
    assert len(_lib.ATTN_FP8_ONLY_PROTOTYPES) == 3 and len(_lib.ATTN_FP8_CENTER_PROTOTYPES) == 4 and len(_lib.ATTN_FP8_PROTOTYPES) == 4
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


P16 = 0x10000          # a 16-byte aligned non-null "device address": refusals never follow it


def test_native_refusals_need_no_gpu():
    lib = _lib.load()
    good = dict(k8=P16, cache_rows=64, row0=0, n0=10, row1=0, n1=0, H=2, k_scale=1.0, c_old=P16, center=P16, ws=P16, ws_bytes=1024)
    order = list(good)
    for kw in [dict(k8=0), dict(c_old=0), dict(center=0), dict(ws=0), dict(k8=P16 + 8), dict(c_old=P16 + 4), dict(center=P16 + 4),
               dict(ws=P16 + 8), dict(n0=0), dict(n0=-1), dict(H=0), dict(cache_rows=0), dict(n1=-1), dict(row0=-1), dict(row0=55),
               dict(row1=-1, n1=3), dict(row1=62, n1=3), dict(k_scale=0.0), dict(k_scale=float("nan")), dict(k_scale=float("inf")),
               dict(H=70000), dict(ws_bytes=1023), dict(cache_rows=300, n0=200, row1=200, n1=57, ws_bytes=2047)]:
        a = dict(good, **kw)
        assert lib.rtv_attn_k8_center(*[a[n] for n in order], None) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_k8_center:"), (kw, lib.rtv_last_error())
    good = dict(k8=P16, cache_rows=64, row0=0, rows=10, H=2, k_scale=1.0, c_old=P16, c_new=P16, amax=0)
    order = list(good)
    for kw in [dict(k8=0), dict(c_old=0), dict(c_new=0), dict(k8=P16 + 4), dict(c_old=P16 + 8), dict(c_new=P16 + 4), dict(amax=P16 + 2),
               dict(rows=0), dict(rows=-3), dict(H=0), dict(cache_rows=0), dict(row0=-1), dict(row0=55), dict(k_scale=0.0),
               dict(k_scale=-1.0), dict(k_scale=float("nan")), dict(H=65536)]:
        a = dict(good, **kw)
        assert lib.rtv_attn_k8_recenter(*[a[n] for n in order], None) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_k8_recenter:"), (kw, lib.rtv_last_error())
    # the centred cache write: its centre, then the list of rtv_qk_norm_rope_k8 with that entry point's messages
    rope = dict(qkv=P16, q_out=P16, k8=P16, cache_rows=256, k_scale=1.0, amax=0, cache_row0=0, M=105, d=256, heads=2, eps=1e-6, wq=P16,
                wk=P16, cs=P16, F=3, gh=5, gw=7, start=2, row_offset=0, ring_lo=0, ring_size=0, ring_shift=0, center=P16)
    order = list(rope)
    for kw, msg in [(dict(center=0), "center must be"), (dict(center=P16 + 8), "center must be"), (dict(k8=0), "null pointer"),
                    (dict(k8=P16 + 8), "16-byte aligned"), (dict(cache_rows=100), "outside [0, cache_rows)"),
                    (dict(k_scale=float("inf")), "finite and positive"), (dict(heads=4), "head_dim must be 128")]:
        a = dict(rope, **kw)
        assert lib.rtv_qk_norm_rope_k8_centered(*[a[n] for n in order], None) != 0, kw
        err = lib.rtv_last_error().decode()
        assert err.startswith("qk_norm_rope_k8:") and msg in err, (kw, err)
    # the forward: both parents' refusals
    assert lib.rtv_dit_forward_attn_fp8_only_centered(None, None, None, None, None, None, 0, None) != 0
    assert "needs its shadow" in lib.rtv_last_error().decode()


def _model():
    from realtime_video_amd.causal_model import CausalWanModel
    return CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=64, device="cpu")


def test_enable_takes_codes_only_on_the_compact_cache():
    from realtime_video_amd.parallel import SimulatedContextParallel
    m = _model()
    assert m.enable_fp8_attention(bf16_cache=False, smooth_k="codes") is m
    assert m._fp8_attention.only() and m._fp8_attention.codes() and m._fp8_attention.center is None
    state = (m._fp8_attention.mode, m._fp8_attention.mode.smooth, m._fp8_attention.mode.only)
    with pytest.raises(ValueError, match='smooth_k="codes"'):          # True stays the error it was, and names the new value
        m.enable_fp8_attention(smooth_k=True, bf16_cache=False)
    with pytest.raises(ValueError, match="bf16_cache=False"):
        m.enable_fp8_attention(smooth_k="codes")
    with pytest.raises(ValueError, match="context_parallel"):
        m.enable_fp8_attention(smooth_k="codes", bf16_cache=False, context_parallel=True)
    with pytest.raises(ValueError, match="smooth_k is"):
        m.enable_fp8_attention(smooth_k="means", bf16_cache=False)
    m.context_parallel = SimulatedContextParallel(2, "heads")
    with pytest.raises(ValueError, match="context parallelism"):
        m.enable_fp8_attention(smooth_k="codes", bf16_cache=False)
    assert state == (m._fp8_attention.mode, m._fp8_attention.mode.smooth, m._fp8_attention.mode.only), "a refused call changed the mode"
    m.context_parallel = None
    # the plain compact mode and the shadow mode know no codes mode
    m.enable_fp8_attention(bf16_cache=False)
    assert not m._fp8_attention.codes() and m._fp8_attention.center_stamp() is None
    m.enable_fp8_attention(smooth_k=True)
    assert not m._fp8_attention.codes() and m._fp8_attention.mode.smooth is True


def test_python_refusals_need_no_gpu():
    from realtime_video_amd.parallel import SimulatedContextParallel
    m = _model()
    bf16 = [{"k": torch.zeros(1, 64, 2, 128, dtype=torch.bfloat16), "v": torch.zeros(1, 64, 2, 128, dtype=torch.bfloat16),
             "global_end_index": 0, "local_end_index": 0}]
    compact = [{"k8": torch.zeros(64, 2, 128, dtype=torch.uint8), "v8t": torch.zeros(1, 2, 128, 64, dtype=torch.uint8), "rows": 64,
                "global_end_index": 0, "local_end_index": 0}]
    with pytest.raises(RuntimeError, match="bf16_cache=False"):          # a model outside the mode
        m.convert_kv_cache_to_fp8(bf16)
    with pytest.raises(RuntimeError, match="smooth_k"):
        m.fp8_attention_set_centers(torch.zeros(1, 2, 128))
    m.enable_fp8_attention()
    with pytest.raises(RuntimeError, match="bf16_cache=False"):
        m.convert_kv_cache_to_fp8(bf16)
    m.enable_fp8_attention(bf16_cache=False, smooth_k="codes")
    with pytest.raises(ValueError, match="compact one already"):
        m.convert_kv_cache_to_fp8(compact)
    two = [dict(bf16[0], k=torch.zeros(2, 64, 2, 128, dtype=torch.bfloat16), v=torch.zeros(2, 64, 2, 128, dtype=torch.bfloat16))]
    with pytest.raises(ValueError, match="batch size 1"):
        m.convert_kv_cache_to_fp8(two)
    with pytest.raises(ValueError, match="one KV cache entry per layer"):
        m.convert_kv_cache_to_fp8(bf16 + bf16)
    m.context_parallel = SimulatedContextParallel(2, "heads")
    with pytest.raises(RuntimeError, match="context parallelism"):
        m.convert_kv_cache_to_fp8(bf16)
    m.context_parallel = None
    assert "k" in bf16[0] and "k8" not in bf16[0], "a refused conversion touched the dicts"
    with pytest.raises(ValueError, match=r"float32 GPU tensor \[num_layers, H, 128\]"):
        m.fp8_attention_set_centers(torch.zeros(1, 2, 128))             # (a CPU tensor)
    with pytest.raises(RuntimeError, match="has not run yet"):
        m.fp8_attention_recenter(compact)
    # a compact dict whose rows stand under other centres
    m._fp8_attention.center_new = m._fp8_attention.center_ws = torch.zeros(1)     # (as if a forward had allocated them: the check comes first)
    stale = [dict(compact[0], local_end_index=10, fp8_center=None)]
    with pytest.raises(RuntimeError, match="other K centres"):
        m.fp8_attention_recenter(stale)
    with pytest.raises(RuntimeError, match="is empty"):
        m.fp8_attention_recenter(compact)
    with pytest.raises(RuntimeError, match="compact KV cache"):
        m.fp8_attention_recenter(bf16)

