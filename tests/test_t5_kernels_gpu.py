"""The five kernels of the text encoder (realtime_video_amd/csrc/t5_encoder.hip), each on its own through the unit entry points of
include/rtv_hip_t5_units.h - the launches rtv_t5_encode makes - on the inputs of tests/t5_cases.py: peaked and structured attention
inputs against the fp64 definition under attn_cases.within_bound, RMSNorm (both output forms) and GEGLU per element under bars
derived from the kernels' rounding points at the widths where their loops repeat, embed and add bit for bit.  The inputs, the bars
and mutants that fail them are checked on the CPU in tests/test_t5_cases_cpu.py.

Every input is a view into a buffer whose surroundings are NaN - the bias table too, with more than a table's length on each side, so
that an index that leaves the table lands in memory this file owns and poisons the row; every output is a view into a buffer
prefilled with a sentinel, and everything outside the written window must still hold it.  Every launch runs twice and the bits must
agree.  No model is built here.

Each launch prints `T5_RATIO kernel=... family=... shape=... ratio=...` (pytest -s): for attention the largest
|out - ref| / (u P|V| + 2.5e-7) (the bar is 4), for the row kernels the largest |out - ref| over the worst case (the bar is 2);
profiles/t5_kernel_bound_ratios.txt holds the per-family maxima of one run.
"""
import ctypes
import math

import pytest
import torch

import attn_cases as ac
import row_cases as rc
import t5_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64                     # guard elements on each side of a buffer: a multiple of 16 bytes in every dtype used here
SENTINEL = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A)}     # 1.5e16 in both: no output comes near


@pytest.fixture(scope="module")
def call():
    from realtime_video_amd import _lib
    _lib.load()

    def _call(name, *args):
        args = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        _lib.call(name, *args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return _call


def _guarded(t, pad=PAD):
    """t on the device as a view into a buffer with `pad` NaN elements in front and behind (int32: INT_MAX)."""
    fill = tc.INT_MAX if t.dtype == torch.int32 else math.nan
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _sentinel(shape, dtype):
    """(buffer, window): a window of `shape` inside a sentinel-filled buffer."""
    bits, value = SENTINEL[dtype]
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), value, dtype=bits, device=DEV).view(dtype)
    return buf, buf[PAD:PAD + n].view(shape)


def _untouched(buf):
    bits, value = SENTINEL[buf.dtype]
    b = buf.view(bits)
    return bool((b[:PAD] == value).all()) and bool((b[-PAD:] == value).all())


def _same_bits(a, b):
    bits = SENTINEL[a.dtype][0]
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


# ------------------------------------------------------------------------------------------------ attention
def _attend(call, case):
    """Two launches of rtv_t5_attention on `case` (already on the device) -> out [rows, H, 64]."""
    rows, H, da = case.rows, case.H, case.H * tc.HD
    qk, vt = _guarded(case.qk()), _guarded(case.vt())
    table = _guarded(case.table, pad=2 * case.max_len + 2 * rows + PAD)          # whatever a wrong index reaches is NaN and owned
    outs = []
    for _ in range(2):
        buf, o = _sentinel((rows, da), torch.bfloat16)
        call("rtv_t5_attention", qk, vt, o, table, rows, case.valid, H, case.max_len)
        assert _untouched(buf), f"{case.name}: written outside the output"
        outs.append(o)
    assert _same_bits(*outs), f"{case.name}: two launches differ"
    return outs[0].view(rows, H, tc.HD)


def _check(call, case):
    case = case.to(DEV)
    out = _attend(call, case)
    ok, ratio, idx = case.within(out)
    print(f"T5_RATIO kernel=attention family={case.family} shape={case.valid}/{case.rows},H{case.H},L{case.max_len} ratio={ratio:.3f}")
    assert bool(torch.isfinite(out.float()).all()), f"{case.name}: a padding query row is not finite"
    assert ok, (f"{case.name}: |out - ref| = {ratio:.2f} u P|V| (bar {ac.BOUND_FACTOR}) at (batch, row, head, dim) {idx}" +
                (f", targets {case.targets[idx[1], idx[2]].tolist()}" if case.targets is not None else ""))
    return out


_CASES = {}


def _family(name):
    if not _CASES:
        for c in tc.attention_cases():
            _CASES.setdefault(c.family, []).append(c)
    return _CASES[name]


@pytest.mark.parametrize("family", ["one_hot", "content_vs_bias", "mask_edge", "running_max", "gaussian"])
def test_attention_family_against_fp64(call, family):
    for case in _family(family):
        _check(call, case)


@pytest.mark.parametrize("valid,H,max_len", tc.SWEEP_SHAPES)
def test_attention_bias_distance_sweep(call, valid, H, max_len):
    """One spike per head, every distance -(valid - 1) .. valid - 1 in turn: the sign, the offset, the head stride and the
    max_len - 1 centre of the table index."""
    for case in tc.bias_sweep(valid, H, max_len):
        _check(call, case)


def test_attention_wide_launch_is_the_tight_launch(call):
    """rows two blocks larger than needed (vt's row stride and the grid grow, the key loop does not): the valid rows are
    bit-identical with the launch at rows = roundup32(valid)."""
    valid, H, L, rows = tc.WIDE
    for build in (tc.one_hot, tc.mask_edge, tc.gaussian):
        wide = build(valid, H, L, rows, seed=valid)
        tight = tc.AttnCase(wide.name + "tight", wide.family, wide.q[:valid], wide.k[:valid], wide.v[:valid], wide.table, valid, L,
                            wide.targets)
        a, b = _check(call, wide), _check(call, tight)
        assert _same_bits(a[:valid], b[:valid]), wide.name


# ------------------------------------------------------------------------------------------------ RMSNorm
def _report(kernel, family, shape, out, ref, worst):
    ok, ratio, (row, col) = rc.within(out, ref, worst)
    print(f"T5_RATIO kernel={kernel} family={family} shape={shape} ratio={ratio:.3f}")
    assert ok, (f"{kernel}, {family}, {shape}: |out - ref| = {ratio:.2f} x the worst case (bar {tc.MARGIN}) at row {row}, column {col}: "
                f"out {float(out[row, col])}, ref {float(ref[row, col])}")


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("d", tc.RMS_WIDTHS)
def test_rmsnorm_rows_against_fp64(call, d, out_f32):
    w = _guarded(rc.gains(d, 1)[0])
    dtype = torch.float32 if out_f32 else torch.bfloat16
    for family, rows in tc.rms_families(d).items():
        x = _guarded(rows)
        M = x.shape[0]
        outs = []
        for _ in range(2):
            buf, o = _sentinel((M, d), dtype)
            call("rtv_t5_rmsnorm", x, w, o, M, d, ctypes.c_float(tc.EPS), int(out_f32))
            assert _untouched(buf), f"rmsnorm, {family}, d = {d}: written outside the output"
            outs.append(o)
        assert _same_bits(*outs), (family, d)
        ref, worst = tc.rms64(x, w, tc.EPS, out_f32)
        _report("rmsnorm_f32" if out_f32 else "rmsnorm_bf16", family, f"{M}x{d}", outs[0], ref, worst)
        if family == "constant":
            assert float(outs[0][0].float().abs().max()) == 0                   # the zero row


# ------------------------------------------------------------------------------------------------ GEGLU
@pytest.mark.parametrize("rows,dff", tc.GEGLU_SHAPES)
def test_geglu_against_fp64(call, rows, dff):
    gf = _guarded(tc.geglu_rows(rows, dff))
    outs = []
    for _ in range(2):
        buf, h = _sentinel((rows, dff), torch.bfloat16)
        call("rtv_t5_geglu", gf, h, rows, dff)
        assert _untouched(buf), f"geglu {rows}x{dff}: written outside the output"
        outs.append(h)
    assert _same_bits(*outs)
    ref, worst = tc.geglu64(gf)
    _report("geglu", "gate_sweep", f"{rows}x{dff}", outs[0], ref, worst)


# ------------------------------------------------------------------------------------------------ embed, add
@pytest.mark.parametrize("d", tc.EMBED_WIDTHS)
def test_embed_is_exact_and_clamps(call, d):
    vocab, rows, valid = 50, 64, 41
    ids, table, want = tc.embed_case(d, vocab, rows, valid)
    ids_d, table_d = _guarded(ids), _guarded(table)
    outs = []
    for _ in range(2):
        buf, x = _sentinel((rows, d), torch.float32)
        call("rtv_t5_embed", ids_d, table_d, x, rows, valid, d, vocab)
        assert _untouched(buf), f"embed d = {d}: written outside the output"
        outs.append(x)
    assert _same_bits(*outs)
    assert _same_bits(outs[0], want.to(DEV)), f"embed d = {d}: {int((outs[0] != want.to(DEV)).sum())} elements differ"
    print(f"T5_RATIO kernel=embed family=clamped_ids shape={rows}x{d} ratio=0.000")


@pytest.mark.parametrize("n", tc.ADD_SIZES)
def test_add_is_the_single_fp32_addition(call, n):
    x0, y, want = tc.add_case(n)
    y_d = _guarded(y)
    outs = []
    for _ in range(2):
        buf, x = _sentinel((n,), torch.float32)
        x.copy_(x0)
        call("rtv_t5_add", x, y_d, ctypes.c_size_t(n))
        assert _untouched(buf), f"add n = {n}: written outside the output"
        outs.append(x)
    assert _same_bits(*outs)
    assert _same_bits(outs[0], want.to(DEV)), f"add n = {n}: {int((outs[0] != want.to(DEV)).sum())} elements differ"
    print(f"T5_RATIO kernel=add family=gaussian shape={n} ratio=0.000")
