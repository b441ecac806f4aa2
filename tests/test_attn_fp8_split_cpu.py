"""CPU checks of the restated KV split of the fp8 attention (tests/attn_fp8_split_cases.py): on every input of
tests/test_attn_fp8_split_gpu.py the split emulation stays inside the UNCHANGED bar of tests/attn_fp8_cases.py (a range's e4m3
rounding floor, taken relative to its own reference point, enters the merge scaled by w_s <= 1), one range is the unsplit emulation
bit for bit, each of three mutants breaks the bar somewhere, and the binding carries the header's declarations."""
import ctypes

import torch

import attn_cases as ac
import attn_fp8_cases as fc
import attn_fp8_split_cases as sc
from realtime_video_amd import _lib

BF16 = torch.bfloat16


def _ratio(spec, S, launch_kw=None, **mutant):
    launch = fc.Launch(spec, **(launch_kw or {}))
    k8, v8t = launch.shadow()
    ref, E = fc.reference(launch, k8, v8t)
    return fc.bound_ratio(sc.emulate_split(launch, k8, v8t, S, **mutant), ref, E)


def test_tile_rule():
    assert sc.tile_list((37, 200), (0, 0)) == [(0, 37, 64, 0), (1, 64, 128, 27), (2, 128, 192, 91), (3, 192, 237, 155)]
    assert sc.tile_list((1000, 1), (10, 130)) == [(15, 1000, 1001, 0), (0, 10, 64, 1), (1, 64, 128, 55), (2, 128, 140, 119)]
    assert sc.tile_list((0, 1100), (0, 0), limit=96) == [(0, 0, 64, 0), (1, 64, 96, 64)]
    assert [sc.split_tile_range(4, s, 5) for s in range(5)] == [(0, 0), (0, 1), (1, 2), (2, 3), (3, 4)]
    assert [sc.split_tile_range(18, s, 4) for s in range(4)] == [(0, 4), (4, 9), (9, 13), (13, 18)]
    assert sc.clamp_splits((37, 200), (0, 0), 16) == 4 and sc.clamp_splits((3, 1100), (0, 0), 16) == 16
    assert sc.key_ranges((37, 200), (0, 0), 2) == [(0, 90), (91, 199)]
    assert sc.key_ranges((1000, 1), (10, 130), 16) == [(0, 0), (1, 54), (55, 118), (119, 130)]


def test_one_range_is_the_unsplit_emulation():
    for spec in (ac.spec_two_ranges((600, 500), (2, 300), dtype=BF16), ac.spec_causal(520, 1100, 96, 37, BF16)):
        launch = fc.Launch(spec)
        k8, v8t = launch.shadow()
        assert torch.equal(sc.emulate_split(launch, k8, v8t, 1), fc.emulate(launch, k8, v8t))


def test_split_emulation_passes_the_unchanged_bound():
    worst, n = 0.0, 0
    for spec, S in sc.all_cases():
        ok, ratio = _ratio(spec, S)
        assert ok, f"{spec.name}: S {S}, ratio {ratio:.3f}"
        worst, n = max(worst, ratio), n + 1
    print(f"{n} split launches, largest err / (E + 2^-8 |ref| + 5e-7): {worst:.3f}")
    assert worst <= 1.0 and n >= 60          # the factor 2 of the bound is margin the emulation does not use


def test_block_causal_workgroups_have_empty_and_masked_ranges():
    """What the block-causal family is there for: with cb = 96 at offset 0 the first workgroup (rows 0..255, largest limit 288) owns 5 of the 18
    tiles (S = 16: eleven empty ranges), and a row of the first block sees nothing of the ranges behind tile 1."""
    launch = fc.Launch(ac.spec_causal(520, 1100, 96, 0, BF16))
    lim = launch.limits()
    tiles = sc.tile_list(launch.seg0, launch.seg1, int(lim[:256].max()))
    assert len(tiles) == 5 and sum(lo == hi for lo, hi in (sc.split_tile_range(5, s, 16) for s in range(16))) == 11
    k8, v8t = launch.shadow()
    m, l, o = sc.emulate_partial(launch, k8, v8t, slice(0, 256), tiles[2:5])
    assert bool((m[:, :96] == -1e30).all()) and bool((l[:, :96] == 0).all()) and bool((o[:96] == 0).all())
    assert bool((l[:, 200:] > 0).all())


def test_mutant_unit_weights():
    assert any(not _ratio(sc.spec_window("one_hot", s0, s1, S), S, unit_weights=True)[0] for s0, s1 in sc.WINDOWS for S in (2, 5))


def test_mutant_boundary_tile():
    """A dropped tile loses one_hot targets; a doubled one leaves a one_hot answer alone (numerator and denominator double) and
    shows in the ties, whose keys in the doubled tile get twice the weight of their copies."""
    for d_hi, family in ((-1, "one_hot"), (1, "tie2")):
        assert any(not _ratio(sc.spec_window(family, s0, s1, S), S, d_hi=d_hi)[0] for s0, s1 in sc.WINDOWS for S in (2, 3)), d_hi


def test_mutant_merge_without_v_scale():
    spec = sc.spec_window("one_hot", (37, 200), (0, 0), 2)
    assert _ratio(spec, 2, dict(v_scale=2.0))[0] and not _ratio(spec, 2, dict(v_scale=2.0), apply_v_scale=False)[0]


def test_binding_has_the_header_and_the_library_the_symbols():
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    P = _lib.ATTN_FP8_CP_PROTOTYPES
    fwd = _lib.ATTN_FP8_PROTOTYPES["rtv_attn_fwd_fp8"]
    S = _lib.STRUCTS
    cfg, w, st = (ctypes.POINTER(S[n]) for n in ("rtv_dit_config", "rtv_dit_weights", "rtv_dit_step"))
    sh = ctypes.POINTER(_lib.ATTN_FP8_STRUCTS["rtv_attn_fp8_shadow"])
    assert P == {
        "rtv_attn_fwd_fp8_split": (fwd[0], fwd[1][:-1] + [i, vp, sz] + fwd[1][-1:]),
        "rtv_dit_quantize_block_attn_fp8": (i, [cfg, st, i, i, sh, vp]),
        "rtv_dit_layer_rest_attn_fp8": (i, [cfg, w, st, i, sh, vp, sz, vp]),
        "rtv_dit_layer_attn_hp_attn_fp8": (i, [cfg, w, st, i, i, vp, vp, sh, vp, sz, vp])}
    for n in [n for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "ATTN_FP8_CP_PROTOTYPES"]:
        assert not set(getattr(_lib, n)) & set(P), n
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
