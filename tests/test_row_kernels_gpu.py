"""The DiT row kernels on structured rows (tests/row_cases.py): layernorm_modulate_kernel, rmsnorm_kernel and both forms of the
RMSNorm(q, k) + RoPE + KV-cache kernel, each element against the fp64 definition under the bar derived from the kernel's own
rounding points, at the widths where the chunk loops change path (8 ... 8192).

Every launch goes through realtime_video_amd.ops.  Inputs are views into buffers whose neighbouring rows (for rtv_rmsnorm: pad
columns as well) are NaN, so a chunk read past d or past M poisons a row; outputs are views into buffers prefilled with a
sentinel, and every element outside the written window must still hold it.  The bit equalities - a second launch, a token
shard against the unsharded launch, the fused fp8 quantiser against quantize_fp8_rows(layernorm_modulate(...)), the two RoPE
forms - run on every family, not only on Gaussian rows.  The inputs, the bars and mutants that fail them are checked on the CPU
in tests/test_row_cases_cpu.py.

Each launch prints `ROW_RATIO kernel=... form=... family=... d=... ratio=...` (pytest -s): the largest |out - ref| over the WORST
CASE of the arithmetic (the bar is 2); profiles/row_kernel_bound_ratios.txt is the per-family maximum of one run.
"""
import functools
import math

import pytest
import torch

import row_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x5A5A            # bf16 1.5e16: no kernel output comes near it
ROW_OFFSET, ROWS_PER_FRAME = 5, 7   # the modulated launches: rows_per_frame divides no row count here, frame boundaries from row 2 on


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _untouched(buf, *windows):
    """Every element of `buf` outside the windows (views of it) still holds the sentinel."""
    bits = buf.view(torch.int16).clone()
    for w in windows:
        start = (w.data_ptr() - buf.data_ptr()) // 2
        torch.as_strided(bits, w.shape, w.stride(), start).fill_(SENTINEL)
    return bool((bits == SENTINEL).all())


def _guarded_rows(x):
    """x on the device as rows 1 .. M of a buffer whose rows 0 and M + 1 are NaN."""
    M, d = x.shape
    buf = torch.full((M + 2, d), math.nan, dtype=torch.bfloat16, device=DEV)
    buf[1:M + 1] = x.to(DEV)
    return buf[1:M + 1]


def _report(kernel, form, family, d, out, ref, worst, extra=""):
    ok, ratio, (row, col) = rc.within(out, ref, worst)
    print(f"ROW_RATIO kernel={kernel} form={form} family={family} d={d} ratio={ratio:.3f}")
    assert ok, (f"{kernel}, {form}, family {family}, d = {d}{extra}: |out - ref| = {ratio:.2f} x the worst case (bar {rc.MARGIN}) at row "
                f"{row}, column {col}: out {float(out[row, col])}, ref {float(ref[row, col])}")
    return ratio


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_forms(d, M):
    """form -> (keyword arguments of ops.layernorm_modulate, keyword arguments of rc.ln64)."""
    w, b = (t.to(DEV) for t in rc.gains(d))
    F = (ROW_OFFSET + M - 1) // ROWS_PER_FRAME + 1
    forms = {"plain": ({}, {}), "affine": (dict(weight=w, bias=b), dict(weight=w, bias=b))}
    for name, J, seed in (("mod6", 6, 0), ("mod2", 2, 1)):       # frame_stride 6 d: a block's table; 2 d: the head's
        t = rc.frame_tables(F, d, J, seed).to(DEV)
        geo = dict(rows_per_frame=ROWS_PER_FRAME, row_offset=ROW_OFFSET)
        forms[name] = (dict(shift=t[0, 0], scale=t[0, 1], frame_stride=J * d, **geo), dict(shift=t[:, 0], scale=t[:, 1], **geo))
    return forms


@pytest.mark.parametrize("d", rc.LN_WIDTHS)
def test_layernorm_rows_against_fp64(ops, d):
    worst_ratio = 0.0
    for family, rows in rc.ln_families(d).items():
        x = _guarded_rows(rows)
        M = x.shape[0]
        for form, (kw, ref_kw) in _ln_forms(d, M).items():
            buf = _sentinel(M + 2, d)
            out = ops.layernorm_modulate(x, rc.EPS, out=buf[1:M + 1], **kw)
            assert _untouched(buf, out), f"layernorm {form}, {family}, d = {d}: a row outside the launch was written"
            ref, worst = rc.ln64(x, rc.EPS, **ref_kw)
            worst_ratio = max(worst_ratio, _report("layernorm", form, family, d, out, ref, worst))
            if family == "constant":                                    # exact: 0, the bias, the frame's shift
                want = {"plain": torch.zeros_like(ref), "affine": ref_kw.get("bias", ref).double().expand_as(ref)}.get(form, ref)
                assert torch.equal(out.double(), want), f"layernorm {form}, constant rows, d = {d}: not bit-exact"
            # the same launch again, and rows 3 .. M - 2 as a shard of their own
            assert torch.equal(ops.layernorm_modulate(x, rc.EPS, **kw), out), (form, family, d)
            lo, hi = 3, M - 2
            if hi > lo:
                skw = dict(kw, row_offset=ROW_OFFSET + lo) if "row_offset" in kw else kw
                assert torch.equal(ops.layernorm_modulate(x[lo:hi], rc.EPS, **skw), out[lo:hi]), (form, family, d)
            if d in rc.FP8_WIDTHS:
                q, s = ops.layernorm_modulate_fp8_rows(x, rc.EPS, **kw)
                q2, s2 = ops.quantize_fp8_rows(out)
                assert torch.equal(q.view(torch.uint8), q2.view(torch.uint8)) and torch.equal(s, s2), \
                    f"fused fp8 quantiser differs from quantize_fp8_rows(layernorm_modulate), {form}, {family}, d = {d}"
    print(f"ROW_WORST kernel=layernorm d={d} ratio={worst_ratio:.3f}")


# ------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("d", rc.LN_WIDTHS)
def test_rmsnorm_rows_against_fp64(ops, d):
    """x and out are column slices of wider buffers, ldx = d + 24 != ldo = d + 40 != d; the pad columns of x are NaN."""
    w = rc.gains(d, 1)[0].to(DEV)
    worst_ratio = 0.0
    for family, rows in rc.rms_families(d).items():
        M = rows.shape[0]
        xb = torch.full((M + 2, d + 24), math.nan, dtype=torch.bfloat16, device=DEV)
        x = xb[1:M + 1, 8:8 + d]
        x.copy_(rows.to(DEV))
        ob = _sentinel(M + 2, d + 40)
        out = ops.rmsnorm(x, w, rc.EPS, out=ob[1:M + 1, 16:16 + d])
        assert _untouched(ob, out), f"rmsnorm, {family}, d = {d}: an element outside the output window was written"
        ref, worst = rc.rms64(x, w)
        worst_ratio = max(worst_ratio, _report("rmsnorm", "strided", family, d, out, ref, worst))
        if family == "constant":
            assert float(out[0].float().abs().max()) == 0                # the zero row
        dense = ops.rmsnorm(x.contiguous(), w, rc.EPS)
        assert torch.equal(dense, out) and torch.equal(ops.rmsnorm(x[3:M - 2], w, rc.EPS), out[3:M - 2]), (family, d)
    print(f"ROW_WORST kernel=rmsnorm d={d} ratio={worst_ratio:.3f}")


# ------------------------------------------------------------------------------------------------ RMSNorm(q, k) + RoPE + cache write
FORMS = {0: "workgroup_per_row", 1: "two_waves_per_row", -1: "default"}


@functools.lru_cache(maxsize=None)
def _table(hd):
    from realtime_video_amd.rope import rope_cos_sin_table
    return rope_cos_sin_table(hd).to(DEV)


def _rope_launch(ops, form, qkv, wq, wk, H, g, rows=None):
    """One launch under rtv_rope_set_wave(form) of the rows [lo, hi) of the geometry's shard (all of them by default), into fresh
    sentinel-filled buffers.  -> (q, k rows written, v rows written): the guards are asserted here."""
    from realtime_video_amd import _lib
    M, d = qkv.shape[0], qkv.shape[1] // 3
    lo, hi = rows or (0, M)
    qbuf = _sentinel(hi - lo + 2, d)
    kc, vc = _sentinel(g.cache_rows, H, d // H), _sentinel(g.cache_rows, H, d // H)
    _lib.load().rtv_rope_set_wave(form)
    try:
        q = ops.qk_norm_rope_cache(qkv[lo:hi], kc, vc, g.cache_row0, H, wq, wk, _table(d // H), g.grid, g.start_frame, rc.EPS,
                                   q_out=qbuf[1:hi - lo + 1], row_offset=g.row_offset + lo, ring=g.ring)
    finally:
        _lib.load().rtv_rope_set_wave(-1)
    idx = g.cache_index()[lo:hi].to(DEV)
    kc2, vc2 = kc.view(g.cache_rows, d), vc.view(g.cache_rows, d)
    written = torch.zeros(g.cache_rows, dtype=torch.bool, device=DEV)
    written[idx] = True
    where = f"RoPE {FORMS[form]}, d = {d}, {H} heads, rows {lo} .. {hi}"
    assert _untouched(qbuf, q), f"{where}: a q row outside the launch was written"
    for name, c in (("K", kc2), ("V", vc2)):
        assert bool((c[~written].view(torch.int16) == SENTINEL).all()), f"{where}: a {name} cache row outside the window was written"
    return q, kc2[idx], vc2[idx]


@pytest.mark.parametrize("d,H", rc.ROPE_SHAPES)
def test_rope_rows_against_fp64_in_both_forms(ops, d, H):
    wq, wk = rc.gains(d, 2)[0].to(DEV), rc.gains(d, 3)[0].to(DEV)
    worst_ratio = 0.0
    for family, rows in rc.rope_families(d).items():
        qkv = _guarded_rows(rc.rope_qkv(rows))
        M = qkv.shape[0]
        g = rc.rope_geom(M, ring=family in ("gaussian", "spike"))          # the ring write together with row_offset > 0
        rq, bq = rc.rope64(qkv[:, :d], wq, H, g.grid, g.start_frame, g.row_offset)
        rk, bk = rc.rope64(qkv[:, d:2 * d], wk, H, g.grid, g.start_frame, g.row_offset)
        got = {}
        for form in (0, 1):
            q, k, v = got[form] = _rope_launch(ops, form, qkv, wq, wk, H, g)
            extra = f", grid {g.grid}, start_frame {g.start_frame}, row_offset {g.row_offset}, ring {g.ring}"
            worst_ratio = max(worst_ratio, _report("rope_q", FORMS[form], family, d, q, rq, bq, extra),
                              _report("rope_k", FORMS[form], family, d, k, rk, bk, extra))
            assert torch.equal(v, qkv[:, 2 * d:]), f"V is not a bit-exact copy: {FORMS[form]}, {family}, d = {d}"
            if family == "constant":
                assert float(q[0].float().abs().max()) == 0 and float(k[M - 1].float().abs().max()) == 0     # the zero row (k: reversed)
            again = _rope_launch(ops, form, qkv, wq, wk, H, g)
            shard = _rope_launch(ops, form, qkv, wq, wk, H, g, rows=(3, M - 2))
            for a, b, c in zip(got[form], again, shard):
                assert torch.equal(a, b), f"two launches differ: {FORMS[form]}, {family}, d = {d}"
                assert torch.equal(a[3:M - 2], c), f"a token shard differs from the unsharded launch: {FORMS[form]}, {family}, d = {d}"
        for a, b in zip(got[0], got[1]):
            assert torch.equal(a, b), f"the two forms differ: {family}, d = {d}, {H} heads"
    print(f"ROW_WORST kernel=rope d={d} H={H} ratio={worst_ratio:.3f}")


def test_rope_default_dispatch_equals_both_forms(ops):
    """M = 2049 rows, one over the threshold from which the launcher takes the two-waves-per-row form; d = 256."""
    d, H, M = 256, 2, 2049
    wq, wk = rc.gains(d, 2)[0].to(DEV), rc.gains(d, 3)[0].to(DEV)
    qkv = _guarded_rows(rc.rope_qkv(rc.mixed(M, d, 2)))
    g = rc.rope_geom(M)
    got = {form: _rope_launch(ops, form, qkv, wq, wk, H, g) for form in (-1, 0, 1)}
    for form in (0, 1):
        for a, b in zip(got[-1], got[form]):
            assert torch.equal(a, b), f"default dispatch differs from the {FORMS[form]} form"
    rq, bq = rc.rope64(qkv[:, :d], wq, H, g.grid, g.start_frame, g.row_offset)
    _report("rope_q", "default", "mixed", d, got[-1][0], rq, bq)
