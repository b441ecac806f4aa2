"""CPU checks of the fp8 attention restatements (tests/attn_fp8_cases.py): the emulation of the kernel's arithmetic passes the
derived bound on every input family of tests/test_attn_fp8_gpu.py, each mutant of it fails on at least one input, the slot map is
a permutation, and the binding carries the header's declarations."""
import ctypes
import os
import re

import pytest
import torch

import attn_cases as ac
import attn_fp8_cases as fc
from realtime_video_amd import _lib

BF16 = torch.bfloat16


def _specs():
    for Lq, Lkv, B, off in ac.EVERY_KEY:
        yield ac.spec_every_key(Lq, Lkv, BF16, B, off)
    for Lq, Lkv, cb, off in ac.CAUSAL:
        for far in (False, True):
            yield ac.spec_causal(Lq, Lkv, cb, off, BF16, far)
    for Lq, Lkv in ac.OUTSIDE:
        yield ac.spec_outside(Lq, Lkv, BF16)
    for seg0, seg1 in ac.TWO_RANGE_WINDOWS:
        yield ac.spec_two_ranges(seg0, seg1, dtype=BF16)
    for Lq, Lkv in ac.STAIRCASE:
        yield ac.spec_staircase(Lq, Lkv, BF16)
    yield ac.spec_gaussian()


def _launches(spec, **kw):
    return [fc.Launch(spec, b, **kw) for b in range(spec.q.shape[0])]


def _fails(launch, shadow=None, ref_shadow=None, **mutant):
    """Does the mutant of the emulation miss the bound?  The reference always comes from the clean shadow."""
    clean = launch.shadow()
    ref, E = fc.reference(launch, *(ref_shadow or clean))
    ok, _ = fc.bound_ratio(fc.emulate(launch, *(shadow or clean), **mutant), ref, E)
    return not ok


def test_slot_map_is_a_permutation_and_matches_the_header():
    assert sorted(fc.SLOT_MAP.tolist()) == list(range(64))
    # the operand argument of the header: register (kb, r = 4 i + j) of lane group g holds key 32 kb + 8 i + 4 g + j and must be the
    # lane's k-byte 16 kb + r of its 32 consecutive bytes 32 g ..
    for kb in range(2):
        for r in range(16):
            for g in range(2):
                assert fc.slot(32 * kb + 8 * (r >> 2) + 4 * g + (r & 3)) == 32 * g + 16 * kb + r
    with open(os.path.join(_lib._INCLUDE, _lib.ATTN_FP8_HEADER)) as f:
        text = f.read()
    m = re.search(r"#define\s+RTV_ATTN_FP8_SLOT\(key\)\s+(.*)", text)
    expr = m.group(1).replace("(key)", "(k)")
    assert [eval(expr, {"k": k}) for k in range(64)] == fc.SLOT_MAP.tolist()
    assert "32 g + 16 kb + 4 i + j" in text


def test_binding_has_the_header():
    i, f, vp, i64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64
    P = _lib.ATTN_FP8_PROTOTYPES
    assert P["rtv_attn_quantize_kv"] == (i, [vp, vp, i64, i, i, i, vp, vp, i, f, f, vp, vp])
    assert P["rtv_attn_fwd_fp8"] == (i, [vp, vp, vp, vp, i, i, i, i, i, i, i, i64, i64, f, f, f, i, i, vp])
    assert P["rtv_dit_lab_capture_self_attn"] == (i, [vp, vp]) and len(P) == 4
    sh = _lib.ATTN_FP8_STRUCTS["rtv_attn_fp8_shadow"]
    pp = ctypes.POINTER(vp)
    assert [(n, t) for n, t in sh._fields_] == [("k8", pp), ("v8t", pp), ("cache_rows", i), ("k_scale", f), ("v_scale", f), ("amax", pp)]
    assert "rtv_attn_fp8_shadow" not in _lib.STRUCTS
    # the DiT forward takes the shadows as an argument: rtv_dit_forward's signature with one struct pointer behind the step
    S = _lib.STRUCTS
    fwd = _lib.PROTOTYPES["rtv_dit_forward"]
    assert P["rtv_dit_forward_attn_fp8"] == (fwd[0], fwd[1][:3] + [ctypes.POINTER(sh)] + fwd[1][3:])
    assert fwd[1][:3] == [ctypes.POINTER(S[n]) for n in ("rtv_dit_config", "rtv_dit_weights", "rtv_dit_step")]
    assert S["rtv_dit_step"]._fields_[-1][0] == "ca_vo_ld"                     # rtv_hip.h is untouched: no new field, no new revision
    assert not set(P) & set(_lib.PROTOTYPES)
    with open(os.path.join(_lib._INCLUDE, "rtv_hip.h")) as fh:
        assert _lib.ABI_VERSION == int(re.search(r"^#define\s+RTV_ABI_VERSION\s+(\d+)", fh.read(), flags=re.M).group(1))


def test_quantiser_restatement_layout():
    g = torch.Generator().manual_seed(5)
    kc, vc = (torch.randn(130, 2, 128, generator=g).to(BF16) * 3 for _ in range(2))
    k8, v8t = fc.empty_shadow(130, 2, fill=0xAA)
    amax = torch.zeros(2)
    fc.quantize_kv(kc, vc, k8, v8t, 63, 2, 0.5, 2.0, amax)
    assert bool((k8[:63] == 0xAA).all()) and bool((k8[65:] == 0xAA).all())
    assert torch.equal(k8[63:65].view(fc.E4M3).float(), (kc[63:65].float() / 0.5).clamp(-448, 448).to(fc.E4M3).float())
    assert torch.equal(v8t[0, :, :, fc.slot(63)], fc.codes(vc[63], 2.0)) and torch.equal(v8t[1, :, :, fc.slot(0)], fc.codes(vc[64], 2.0))
    assert int((v8t != 0xAA).sum()) <= 2 * 2 * 128 and float(amax[0]) == float(kc[63:65].float().abs().max())
    rows = torch.tensor([63, 64])
    assert torch.equal(fc.gather_v(v8t, rows), fc.codes(vc[rows], 2.0))


@pytest.mark.parametrize("slack", [0.0, 8.0])
def test_emulation_passes_the_bound(slack):
    worst = 0.0
    for spec in _specs():
        for launch in _launches(spec):
            k8, v8t = launch.shadow()
            ref, E = fc.reference(launch, k8, v8t)
            ok, ratio = fc.bound_ratio(fc.emulate(launch, k8, v8t, slack=slack), ref, E)
            assert ok, f"{launch.name}: slack {slack}, ratio {ratio:.3f}"
            worst = max(worst, ratio)
    print(f"largest err / (E + 2^-8 |ref| + 5e-7) at slack {slack}: {worst:.3f}")
    assert worst <= 1.0          # the factor 2 of the bound is margin the emulation does not use


def test_scales_cancel_in_the_emulation():
    """k_scale = 2, v_scale = 0.5 against scale 1 on inputs that both grids hold exactly (fc.on_both_grids)."""
    for spec in (fc.on_both_grids(ac.spec_every_key(300, 129, BF16)), fc.on_both_grids(ac.spec_staircase(300, 200, BF16))):
        one, two = fc.Launch(spec), fc.Launch(spec, k_scale=2.0, v_scale=0.5)
        ref1, E1 = fc.reference(one, *one.shadow())
        ref2, E2 = fc.reference(two, *two.shadow())
        assert torch.equal(ref1, ref2) and torch.equal(E1, E2)
        out1, out2 = fc.emulate(one, *one.shadow()), fc.emulate(two, *two.shadow())
        assert fc.bound_ratio(out2, ref1, E1)[0] and torch.equal(out1, out2)


def test_mutant_swapped_v_slots():
    swapped = fc.SLOT_MAP.clone()
    swapped[[3, 40]] = swapped[[40, 3]]
    assert _fails(fc.Launch(ac.spec_every_key(300, 129, BF16)), slot_map=swapped)


WINDOW_SPECS = [ac.spec_two_ranges(s0, s1, dtype=BF16) for s0, s1 in ac.TWO_RANGE_WINDOWS] + [ac.spec_outside(257, 129, BF16)]


@pytest.mark.parametrize("which", ["d_seg0", "d_seg1"])
@pytest.mark.parametrize("delta", [(-1, 0), (1, 0), (0, -1), (0, 1)])
def test_mutant_window_off_by_one(which, delta):
    hit = []
    for spec in WINDOW_SPECS:
        launch = fc.Launch(spec)
        first, n = launch.seg0 if which == "d_seg0" else launch.seg1
        if n == 0 or n + delta[1] - delta[0] <= 0 or first + delta[0] < 0 or first + n + delta[1] > launch.cache_rows:
            continue
        if _fails(launch, **{which: delta}):
            hit.append(spec.name)
    assert hit, f"no window spec notices {which} moved by {delta}"


@pytest.mark.parametrize("d_lim", [-1, 1])
def test_mutant_causal_limit_off_by_one(d_lim):
    assert any(_fails(fc.Launch(ac.spec_causal(300, 520, cb, off, BF16)), d_lim=d_lim) for cb, off in ((8, 37), (96, 0), (96, 220)))


def test_mutant_k_scale_not_applied():
    specs = [ac.spec_staircase(300, 200, BF16), ac.spec_every_key(520, 1100, BF16), ac.spec_gaussian()]
    assert any(_fails(fc.Launch(s, k_scale=2.0), apply_k_scale=False) for s in specs)


def test_mutant_v_scale_not_applied():
    assert _fails(fc.Launch(ac.spec_every_key(300, 129, BF16), v_scale=2.0), apply_v_scale=False)


def test_mutant_masked_v_not_zeroed():
    """Rows outside the window may hold anything: NaN codes there must not reach the output."""
    hit = 0
    for spec in (ac.spec_outside(257, 129, BF16), ac.spec_two_ranges((3, 77), (200, 1003), dtype=BF16)):
        launch = fc.Launch(spec)
        clean = launch.shadow()
        k8, v8t = fc.empty_shadow(launch.cache_rows, 2, fill=fc.NAN_CODE)
        for first, n in (launch.seg0, launch.seg1):
            if n:
                fc.quantize_kv(launch.kc, launch.vc, k8, v8t, first, n)
        assert not _fails(launch, shadow=(k8, v8t), ref_shadow=clean), "the emulation itself must shrug the poison off"
        hit += _fails(launch, shadow=(k8, v8t), ref_shadow=clean, zero_masked_v=False)
    assert hit == 2


def test_truncating_p_shows_in_rel_l2_but_not_in_the_bound():
    """Why the GPU file also compares rel-L2 with the emulation on the diffuse input."""
    launch = fc.Launch(ac.spec_gaussian())
    k8, v8t = launch.shadow()
    ref, E = fc.reference(launch, k8, v8t)
    good, bad = fc.emulate(launch, k8, v8t), fc.emulate(launch, k8, v8t, truncate_p=True)
    r_good, r_bad = fc.rel_l2(good, ref), fc.rel_l2(bad, ref)
    print(f"rel-L2 vs reference: rounding {r_good:.3e}, truncating {r_bad:.3e}")
    assert fc.bound_ratio(bad, ref, E)[0] and r_bad > 1.25 * r_good
