"""The attention kernels on peaked inputs (tests/attn_cases.py): every query's answer hangs on one or two known keys, so a key
masked, dropped, read twice or read from outside the window is an O(1) error, not the O(1 / Lkv) one it is on Gaussian data.

Every case goes through realtime_video_amd.ops, pins its kernel with ops.attn_set_waves, asserts from ops.dispatch_counts which
kernel really ran - where the launcher hands a case to another kernel by design, that kernel by name - and compares with the
fp64 definition by the one rule `attn_cases.within_bound`: |out - ref| <= 4 u (P @ |V|) + 1e-6.  The inputs, the bound and
mutants that fail it are checked on the CPU in tests/test_attention_cases_cpu.py.

Each case prints `ATTN_RATIO family=... kernel=... ratio=...` (pytest -s): the share of the bound it used, in units of
u * ref_abs; profiles/attn_peaked_bound_ratios.txt is the per-family, per-kernel maximum of one run.
"""
import functools

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
W4 = 840 + 600               # ops.attn_set_waves: the one-wave-per-SIMD kernel, product variant
L128 = "attn_fwd_kernel<lockstep, 128 rows>"
L256 = "attn_fwd_kernel<lockstep, 256 rows>"
PP = "attn_fwd_pp_kernel<four-phase>"
ONE = "attn_fwd_w4_kernel<one wave per SIMD>"
COMBINE = "attn_combine_kernel<kv split>"
KERNELS = [4, 81, 82, W4]
KERNEL_IDS = {0: "default", 4: "lockstep128", 81: "lockstep256", 82: "four_phase", W4: "one_wave"}


def _kid(w):
    return KERNEL_IDS[w]


def _did(dt):
    return "bf16" if dt == BF16 else "f16"


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


def expected_kernel(waves, spec, splits=1):
    """The kernel the launcher's rules give this case (csrc/attn_fwd.hip, attn_fwd_impl).  The one-wave-per-SIMD kernel is bf16,
    one key range, no counted key: everything else that asks for it falls to the four-phase kernel from 1024 keys on and to the
    256-row lockstep kernel below; a counted key always runs on a lockstep kernel.  waves = 0 is the production dispatch: 128-row
    workgroups while the 256-row grid cannot fill 5/8 of the chip or the window has at most 512 keys - every grid of this file."""
    B, Lq, H, _ = spec.q.shape
    dup = spec.dup_key >= 0 and spec.dup_count > 1
    two, f16, Lkv = spec.seg1[1] > 0, spec.dtype == F16, spec.Lkv
    if waves == 0:
        assert B * H * ((Lq + 255) // 256) * splits < 100, "grid too large for the default-dispatch expectation of this file"
        return L128
    if waves == 4:
        return L128
    if waves == 81 or dup:
        return L256
    if waves == W4 and not f16 and not two:
        return ONE
    return PP if (waves == 82 or Lkv >= 1024) else L256


def launch(ops, waves, spec, splits=1, out=None, win=False):
    """One launch under ops.attn_set_waves(waves) -> (output, name of the kernel that ran); asserts the dispatch counters."""
    kc, vc = spec.caches()
    (r0, n0), (r1, n1) = spec.seg0, spec.seg1
    ops.attn_set_waves(waves)
    try:
        ops.dispatch_counts(reset=True)
        if splits > 1:
            got = ops.attn_fwd_split(spec.q, kc, vc, spec.seg0, spec.seg1, kv_splits=splits, out=out,
                                     causal_block=spec.causal_block, q_offset=spec.q_offset)
        elif spec.dup_key >= 0:
            got = ops.attn_fwd_dup(spec.q, kc[:, r0:r0 + n0], vc[:, r0:r0 + n0], spec.dup_key, spec.dup_count, out=out)
        elif n1 > 0 or win:
            got = ops.attn_fwd_win(spec.q, kc, vc, spec.seg0, spec.seg1, out=out)
        else:
            got = ops.attn_fwd(spec.q, kc[:, r0:r0 + n0], vc[:, r0:r0 + n0], out=out, causal_block=spec.causal_block,
                               q_offset=spec.q_offset)
        torch.cuda.synchronize()
        counts = {n: c for n, c in ops.dispatch_counts(reset=True).items() if n.startswith("attn_")}
    finally:
        ops.attn_set_waves(0)
    want = expected_kernel(waves, spec, splits)
    want_counts = {want: 1}
    if min(splits, (spec.Lkv + ac.KT - 1) // ac.KT) > 1:
        want_counts[COMBINE] = 1
    assert counts == want_counts, f"{spec.name}: attn_set_waves({waves}), kv_splits {splits} ran {counts}, expected {want_counts}"
    return got, want + (" + " + COMBINE if COMBINE in want_counts else "")


@functools.lru_cache(maxsize=None)
def _on_device(factory, *args):
    """(spec on the GPU, fp64 reference, fp64 P @ |V|): built once per input, shared by the kernels that run on it, never changed."""
    spec = factory(*args).to(DEV)
    ref, ref_abs = spec.reference(DEV)
    return spec, ref, ref_abs


def check(family, kernel, spec, out, ref, ref_abs, splits=1):
    ok, ratio, (b, row, head, dim) = ac.within_bound(out, ref, ref_abs, spec.dtype)
    print(f"ATTN_RATIO family={family} kernel={kernel} dtype={_did(spec.dtype)} splits={splits} case={spec.name} ratio={ratio:.3f}")
    keys = [int(t) for t in spec.targets[row, head]]
    assert ok, (f"family {family}, {kernel}, {_did(spec.dtype)}, {spec.name}, kv_splits {splits}: |out - ref| = {ratio:.2f} u ref_abs "
                f"(bar {ac.BOUND_FACTOR}) at batch {b}, query row {row}, head {head}, dim {dim}: out {float(out[b, row, head, dim])}, "
                f"ref {float(ref[b, row, head, dim])}; the row was built to retrieve key(s) {keys}; decoy rows (cache row, key): "
                f"{spec.decoy_rows[:6]}")
    return ratio


def run(ops, family, waves, factory, *args, splits=1, win=False):
    spec, ref, ref_abs = _on_device(factory, *args)
    out, kernel = launch(ops, waves, spec, splits, win=win)
    check(family, kernel, spec, out, ref, ref_abs, splits)
    return out


# ------------------------------------------------------------------------------------------------ a. every key position
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_did)
@pytest.mark.parametrize("waves", KERNELS, ids=_kid)
@pytest.mark.parametrize("Lq,Lkv,B,offset", ac.EVERY_KEY)
def test_a_every_key_position_is_retrieved(ops, Lq, Lkv, B, offset, waves, dtype):
    """Dense one_hot: each key of each tile (with Lq >= Lkv, or over the three offsets of the 1100-key window) is the sole answer
    of some row.  K and V are the two planes of an interleaved arena and start at its row 5; B = 2 once.  f16 has no
    one-wave-per-SIMD form: the launcher's fallback is asserted by name."""
    run(ops, "a", waves, ac.spec_every_key, Lq, Lkv, dtype, B, offset)


# ------------------------------------------------------------------------------------------------ b. block-causal boundary
@pytest.mark.parametrize("far", [False, True], ids=["last_key", "far_key"])
@pytest.mark.parametrize("waves,splits", [(4, 1), (81, 1), (82, 1), (W4, 1), (4, 2), (W4, 5), (0, 5), (82, 2)],
                         ids=lambda v: KERNEL_IDS.get(v, f"S{v}"))
@pytest.mark.parametrize("Lq,Lkv,cb,q_offset", ac.CAUSAL)
def test_b_block_causal_limit_is_exact(ops, Lq, Lkv, cb, q_offset, waves, splits, far):
    """Every row's answer is its last allowed key lim - 1 (far_key: the far end of its own key block) and key lim, where it exists,
    would win the row's softmax if the mask let it through; through attn_fwd_split each workgroup splits its own tile count."""
    run(ops, "b", waves, ac.spec_causal, Lq, Lkv, cb, q_offset, BF16, far, splits=splits)


# ------------------------------------------------------------------------------------------------ c. nothing outside the window
@pytest.mark.parametrize("poison", [False, True], ids=["decoys", "nan_inf"])
@pytest.mark.parametrize("waves", KERNELS, ids=_kid)
@pytest.mark.parametrize("Lq,Lkv", ac.OUTSIDE)
def test_c_rows_outside_the_window_are_never_used(ops, Lq, Lkv, waves, poison):
    """The window is rows [3, 3 + Lkv) of a larger cache; the row in front of it and the 64 rows behind it - the reach of the
    ragged last tile - hold rows that would win the softmax, or NaN in V and +Inf in K.  Pins what the kernels say about those
    rows: the lockstep and four-phase kernels clamp them to the window's last row, the one-wave-per-SIMD kernel reads zeros."""
    out = run(ops, "c", waves, ac.spec_outside, Lq, Lkv, BF16, poison)
    assert bool(torch.isfinite(out.float()).all())


def test_c_rows_outside_the_window_f16(ops):
    for waves in (4, 81, 82):
        for poison in (False, True):
            run(ops, "c", waves, ac.spec_outside, 257, 129, F16, poison)


# ------------------------------------------------------------------------------------------------ d. two-range windows
@pytest.mark.parametrize("waves,splits", [(4, 1), (81, 1), (82, 1), (W4, 1), (0, 1), (4, 2), (82, 5), (W4, 2)],
                         ids=lambda v: KERNEL_IDS.get(v, f"S{v}"))
@pytest.mark.parametrize("seg0,seg1", ac.TWO_RANGE_WINDOWS, ids=lambda s: f"{s[0]}+{s[1]}")
def test_d_two_range_window_reads_its_two_ranges_only(ops, seg0, seg1, waves, splits):
    """one_hot over the concatenated window of attn_fwd_win, decoys on the cache rows next to each end of each range.  The
    one-wave-per-SIMD kernel takes one range: with two the launcher falls back, which is asserted by name."""
    run(ops, "d", waves, ac.spec_two_ranges, seg0, seg1, 300, BF16, splits=splits, win=True)


def test_d_two_range_window_f16(ops):
    for waves in (4, 82):
        run(ops, "d", waves, ac.spec_two_ranges, (3, 77), (200, 1003), 300, F16, win=True)


# ------------------------------------------------------------------------------------------------ e. counted key
@pytest.mark.parametrize("waves", [0, 4, 81, 82, W4], ids=_kid)
@pytest.mark.parametrize("kind,n_real,dup_key,count", ac.COUNTED)
def test_e_counted_key_counts_exactly(ops, kind, n_real, dup_key, count, waves):
    """attn_fwd_dup against the fp64 definition with bias = log(count) on that key: a tie with a real key answers
    (v_a + n v_dup) / (n + 1).  A counted key runs on the lockstep kernels whatever is asked for (asserted by name)."""
    run(ops, "e", waves, ac.spec_counted, kind, n_real, dup_key, count, 257, BF16)


def test_e_counted_key_f16(ops):
    for count in (2, 7):
        run(ops, "e", 0, ac.spec_counted, "tie", 200, 200, count, 257, F16)


# ------------------------------------------------------------------------------------------------ f. split and combine
@pytest.mark.parametrize("waves", [0, 4, W4], ids=_kid)
@pytest.mark.parametrize("kind,Lkv,splits", ac.SPLIT)
def test_f_split_and_combine(ops, kind, Lkv, splits, waves):
    """one_hot with targets in every range (one range's maximum about 40 log2 units above the others: the underflow side of
    2^(m_s - m)), ties between keys of two and three ranges (equal maxima: equal weights), the staircase; more splits than key
    tiles at 200 keys x 5 and 16."""
    run(ops, "f", waves, ac.spec_split, kind, Lkv, splits, 300, BF16, splits=splits)


def test_f_split_and_combine_f16(ops):
    for kind in ("one_hot", "tie3", "staircase"):
        run(ops, "f", 4, ac.spec_split, kind, 1100, 5, 300, F16, splits=5)


# ------------------------------------------------------------------------------------------------ g. rescale path
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_did)
@pytest.mark.parametrize("waves", KERNELS, ids=_kid)
@pytest.mark.parametrize("Lq,Lkv", ac.STAIRCASE)
def test_g_lazy_rescale_on_a_staircase_of_maxima(ops, Lq, Lkv, waves, dtype):
    run(ops, "g", waves, ac.spec_staircase, Lq, Lkv, dtype)


# ------------------------------------------------------------------------------------------------ h. output rows
@pytest.mark.parametrize("waves,splits", [(4, 1), (81, 1), (82, 1), (W4, 1), (4, 3), (W4, 2)],
                         ids=lambda v: KERNEL_IDS.get(v, f"S{v}"))
@pytest.mark.parametrize("Lq", [1, 257, 300])
def test_h_only_the_output_rows_are_written(ops, Lq, waves, splits):
    """out= is rows [7, 7 + Lq) of a larger buffer pre-filled with a sentinel bit pattern: the guard rows on both sides are
    bit-identical afterwards, and the rows between are the answer."""
    spec, ref, ref_abs = _on_device(ac.spec_every_key, Lq, 129, BF16, 1, 0)
    H = spec.q.shape[2]
    buf = torch.full((1, Lq + 14, H, ac.D), 0x5A5A, dtype=torch.int16, device=DEV)
    out = buf.view(BF16)[:, 7:7 + Lq]
    got, kernel = launch(ops, waves, spec, splits, out=out)
    assert got.data_ptr() == out.data_ptr()
    check("h", kernel, spec, out, ref, ref_abs, splits)
    assert bool((buf[:, :7] == 0x5A5A).all()) and bool((buf[:, 7 + Lq:] == 0x5A5A).all()), f"{kernel} wrote outside its {Lq} output rows"


# ------------------------------------------------------------------------------------------------ i. the bound on diffuse data
@pytest.mark.parametrize("waves", [0] + KERNELS, ids=_kid)
def test_i_gaussian_data_within_the_same_bound(ops, waves):
    """The data of the older attention tests (tests/test_kernels_gpu.py) under the bound that follows from the arithmetic."""
    run(ops, "i", waves, ac.spec_gaussian, 520, 1100, BF16)
    run(ops, "i", waves, ac.spec_gaussian, 520, 1100, F16)
