"""The fp8 Linear path on the integer operands of tests/gemm_fp8_cases.py: both e4m3 GEMM kernels (ops.gemm_fp8_rows with scales
that change with every row and column, ops.gemm_fp8 with constant ones) through the K pipeline at every depth that takes another
path, through every split-K plan, the direct and the LDS store, strided operands between NaN guards and the fused epilogues; and the
per-tensor activation quantiser on every bf16 value e4m3 can hold.  The expected output is known bit for bit, so every comparison is
equality of bit patterns.  tests/test_gemm_fp8_cases_cpu.py proves that each named slip of gemm_fp8_cases.SLIPS would break that
equality on the cases used here.

RTV_GEMM_FP8_EXACT_RECORD=<path> writes one line per case (kernels, plan, largest |integer| sum, launches, mismatches, guards,
seconds)."""
import os
import time

import pytest
import torch

import gemm_fp8_cases as K
from fp8_rows_oracle import fp8_rows_quantize

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNELS = (K.ROWS, K.TENSOR)
RECORD = []


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("RTV_GEMM_FP8_EXACT_RECORD")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("# case | kernels | plan (R, S, split_first) | largest |integer| sum | launches | mismatches | guards | seconds\n")
            f.write("".join(line + "\n" for line in RECORD))


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    _ops.ensure_gemm_workspace(torch.device(DEV))             # one workspace for every launch of this module
    return _ops


class Tally:
    """Per-test record: every launch's acceptance is asserted at once; the totals go to the record line."""

    def __init__(self, name, plan):
        self.name, self.plan, self.kernels, self.launches, self.max_int, self.guards = name, plan, [], 0, 0, "none"
        self.t0 = time.perf_counter()

    def accept(self, kernel, out, ref, guard_buf=None, offset=0):
        torch.cuda.synchronize()
        self.launches += 1
        if kernel not in self.kernels:
            self.kernels.append(kernel)
        bad = K.mismatches(out, ref)
        msg = ""
        if bad:
            first = (K.bits(out) != K.bits(ref)).reshape(-1).nonzero()[0].item()
            m, n = divmod(first, out.shape[1])
            msg = (f"{bad} of {out.numel()} outputs differ; first at row {m}, column {n} (row {m % K.BM}, column {n % K.BN} of tile "
                   f"({m // K.BM}, {n // K.BN})): got {float(out[m, n])}, expected {float(ref[m, n])}")
        assert bad == 0, f"{self.name} [{kernel}, launch {self.launches}]: {msg}"
        if guard_buf is not None:
            self.guards = "untouched"
            changed = K.guards_changed(guard_buf, out.shape[1], offset)
            assert changed == 0, f"{self.name} [{kernel}]: {changed} guard elements overwritten"

    def done(self, extra=""):
        secs = time.perf_counter() - self.t0
        names = ", ".join("gemm_fp8_rows" if k == K.ROWS else "gemm_fp8" if k == K.TENSOR else k for k in self.kernels)
        RECORD.append(f"{self.name} | {names} | {self.plan} | {self.max_int} | {self.launches} | 0 | {self.guards} | {secs:.2f}{extra}")
        print(RECORD[-1])


def _s_x():
    return torch.full((1,), K.S_X, dtype=torch.float32, device=DEV)


def _gemm(ops, kernel, aq, wq, sa, sw, **kw):
    if kernel == K.ROWS:
        return ops.gemm_fp8_rows(aq, sa, wq, sw, **kw)
    return ops.gemm_fp8(aq, _s_x(), wq, K.S_W, **kw)


def _nan_out(M, N):
    """an output nobody has written: a tile whose reducer never ran stays NaN"""
    return torch.full((M, N), float("nan"), dtype=K.BF, device=DEV)


def _check_plan(c):
    """The case takes its recorded plan on this device, or says why it cannot."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if c.needs_g_plan and cus != K.G_PLAN:
        pytest.skip(f"{c.name}: the recorded plan {c.plan} holds at {K.G_PLAN} compute units, this device has {cus}")
    assert K.plan(c.tiles, c.nk, cus) == c.plan, (c.name, cus)


# ------------------------------------------------------------------------------------------------ depth and tile map
@pytest.mark.parametrize("c", K.GEMM_CASES, ids=lambda c: c.name)
def test_case_is_exact_through_both_kernels_twice(ops, c):
    """Every depth (1, 2, 3, 5 K-tiles unsplit; S = 2, 3, 8), the one-row problems and the tile maps (short last supertile group,
    more tiles than compute units with the split units first / last), each launched on two different operand sets with one
    workspace: a stale slab, an arrival counter not back at zero (the output stays NaN) or a dropped, doubled or stale K-tile
    changes most of a tile.  The two large cases build their fp64 reference on the device."""
    _check_plan(c)
    tally = Tally(c.name, c.plan)
    t_ref = 0.0
    for launch in (0, 1):
        t0 = time.perf_counter()
        o = K.build(c, launch, DEV)                           # asserts the exactness condition
        refs = {k: K.reference(c, o, k) for k in KERNELS}
        torch.cuda.synchronize()
        t_ref += time.perf_counter() - t0
        tally.max_int = max(tally.max_int, o.max_int)
        for kernel in KERNELS:
            out = _gemm(ops, kernel, o.aq, o.wq, o.sa, o.sw, out=_nan_out(c.M, c.N))
            tally.accept(kernel, out, refs[kernel])
    tally.done(f" (references on the device: {t_ref:.2f} s)" if c.big else "")


@pytest.mark.parametrize("c", [c for c in K.DEPTH_CASES if c.K in (384, 1024, 1664)], ids=lambda c: c.name)
def test_device_output_differs_from_every_slipped_reference(ops, c):
    """The other half of the CPU proof, on the device's own output: it equals the reference and differs from what each named slip
    would have produced (unsplit, S = 2 and S = 3)."""
    _check_plan(c)
    prev, o = K.build(c, 0, DEV), K.build(c, 1, DEV)
    for kernel in KERNELS:
        out = _gemm(ops, kernel, o.aq, o.wq, o.sa, o.sw, out=_nan_out(c.M, c.N))
        torch.cuda.synchronize()
        assert K.mismatches(out, K.reference(c, o, kernel)) == 0
        for slip in K.covering_slips(c, kernel):
            assert K.mismatches(out, K.reference(c, o, kernel, slip=slip, previous=prev)) >= out.numel() // 4, (c.name, kernel, slip)


# ------------------------------------------------------------------------------------------------ direct store
@pytest.mark.parametrize("c", K.DIRECT_STORE_CASES, ids=lambda c: c.name)
def test_direct_store_path_is_exact_and_stays_inside_its_columns(ops, c):
    """An output whose rows are 8 bytes off 16-byte alignment takes store_tile (registers to memory, no LDS image): unsplit with
    a steady-state trip and behind the S = 3 reduction, with and without a bias; the columns beside the slice are untouched."""
    _check_plan(c)
    tally = Tally(c.name + " [direct store]", c.plan)
    for launch in (0, 1):
        o = K.build(c, launch, DEV)
        tally.max_int = max(tally.max_int, o.max_int)
        for kernel in KERNELS:
            for use_bias in (False, True):
                buf, out = K.guarded_output(c.M, c.N, DEV, offset=4)
                assert out.data_ptr() % 16 == 8 and (out.stride(0) * 2) % 16 == 0
                out.fill_(float("nan"))
                _gemm(ops, kernel, o.aq, o.wq, o.sa, o.sw, bias=o.bias if use_bias else None, out=out)
                tally.accept(kernel, out, K.reference(c, o, kernel, use_bias), buf, 4)
    tally.done()


# ------------------------------------------------------------------------------------------------ strided operands
@pytest.mark.parametrize("c", K.STRIDED_CASES, ids=lambda c: c.name)
def test_strided_operands_between_nan_guards(ops, c):
    """lda = K + 16, ldw = K + 32, the padding columns and 64 rows in front of and behind each operand hold the e4m3 NaN code: a
    read outside the K range or outside the rows (the clamped rows of the ragged tiles included) makes outputs NaN.  The output is
    a column slice between guard columns."""
    _check_plan(c)
    tally = Tally(c.name + " [lda = K + 16, ldw = K + 32]", c.plan)
    for launch in (0, 1):
        o = K.build(c, launch, DEV)
        tally.max_int = max(tally.max_int, o.max_int)
        a_buf, a = K.guarded_operand(o.aq, K.PAD_A, DEV)
        w_buf, w = K.guarded_operand(o.wq, K.PAD_W, DEV)
        assert a.stride(0) == c.K + K.PAD_A and w.stride(0) == c.K + K.PAD_W and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
        for kernel in KERNELS:
            ref = K.reference(c, o, kernel)
            for offset in (8, 4):                             # the store through LDS and the direct store
                buf, out = K.guarded_output(c.M, c.N, DEV, offset)
                out.fill_(float("nan"))
                _gemm(ops, kernel, a, w, o.sa, o.sw, out=out)
                assert bool(torch.isfinite(out).all()), f"{c.name} [{kernel}]: {int((~torch.isfinite(out)).sum())} outputs not finite"
                tally.accept(kernel, out, ref, buf, offset)
        assert bool((K.bits(a_buf)[:K.GUARD_ROWS] == K.NAN_CODE).all()) and bool((K.bits(w_buf)[:, c.K:] == K.NAN_CODE).all())
    tally.done()


# ------------------------------------------------------------------------------------------------ epilogue mapping
@pytest.mark.parametrize("direct", [False, True], ids=["lds_store", "direct_store"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_epilogue_mapping_exact(ops, kernel, direct):
    """A = 0, so the output is the epilogue of a zero accumulator: every element depends on its own (row, column) only through
    bias, gate row (frame of row_offset + row) and residual, and the chain y = bf16(acc + bias); y = bf16(act(y));
    t = bf16(y * gate); out = bf16(res + t) restated in torch must come back bit for bit - for store_tile_lds<false, 4> and for
    store_tile<false, Cfg>."""
    p = K.epilogue_problem(DEV)
    M, N, rpf = p["M"], p["N"], p["rpf"]
    offset = 4 if direct else 8
    tally = Tally(f"epilogue_{M}_{N}_rpf{rpf} [{'direct store' if direct else 'LDS store'}]", K.plan(4, 1))

    def run(name, ref, rows=M, residual=None, in_place=False, **kw):
        buf, out = K.guarded_output(rows, N, DEV, offset)
        assert (out.data_ptr() % 16 == 8) == direct
        if in_place:
            out.copy_(residual)
            residual = out
        else:
            out.fill_(float("nan"))
        _gemm(ops, kernel, p["aq"][:rows], p["wq"], p["sa"][:rows].contiguous(), p["sw"], out=out, residual=residual, **kw)
        tally.accept(f"{kernel}: {name}", out, ref, buf, offset)

    gbias, gexp = K.gelu_safe_bias(N, 7)
    run("bias + gelu", gexp[None, :].expand(M, N).contiguous(), bias=gbias, act=1)
    gated = dict(bias=p["bias"], gate=p["gate"], gate_stride=N, rows_per_frame=rpf)
    whole = K.epilogue_reference(p)
    run("bias + gate + residual", whole, residual=p["res"], **gated)
    run("in place", whole, residual=p["res"], in_place=True, **gated)
    run("none", torch.zeros(M, N, dtype=K.BF, device=DEV))
    shifted = K.epilogue_reference(p, 2 * rpf, rpf)
    assert K.mismatches(shifted, whole[:2 * rpf]) > rpf * N   # the next frame's gate is another gate
    run("row_offset", shifted, rows=2 * rpf, residual=p["res"][:2 * rpf], row_offset=rpf, **gated)
    tally.kernels = [kernel]
    tally.done(" (bias + gelu, bias + gate + residual, in place, none, row_offset)")


# ------------------------------------------------------------------------------------------------ per-tensor quantiser
def _quantize_checked(ops, x, d, what):
    """ops.quantize_fp8 of the first d columns of the host matrix x [M][ld] into a strided output: codes and scale bits equal the
    restatement evaluated on the host, the output padding bytes are untouched."""
    M, ld = x.shape
    rq, rs = K.quantize_tensor_restated(x[:, :d])
    xd = x.to(DEV)
    qbuf = torch.full((M, ld), K.QUANT_PAD_OUT, dtype=torch.uint8, device=DEV)
    q, s = ops.quantize_fp8(xd[:, :d], out=qbuf.view(K.E4)[:, :d])
    torch.cuda.synchronize()
    assert s.dtype == torch.float32 and s.shape == (1,)
    assert torch.equal(K.bits(s).cpu(), K.bits(rs)), f"{what}: scale {float(s)} != {float(rs)}"
    bad = K.mismatches(q.cpu(), rq)
    assert bad == 0, f"{what}: {bad} of {M * d} codes differ"
    assert bool((qbuf[:, d:] == K.QUANT_PAD_OUT).all()), f"{what}: output padding bytes written"
    return rs


@pytest.mark.parametrize("M,d,ld", K.QUANT_SHAPES)
def test_quantize_fp8_shapes_strides_and_the_place_of_the_maximum(ops, M, d, ld):
    """One chunk; the widest row; more rows than the 1024 workgroups (second and third trip of both row loops); strided input and
    output.  The maximum is one element +-448 * 2^e at the first element, the last one, the first of row 1024: the scale is
    2^e exactly if both passes see every element once.  Input padding holds 3e38, output padding must stay."""
    for name, r, col in K.quant_peaks(M, d):
        for e, sign in ((0, 1.0), (-9, -1.0)):
            x = K.quant_shape_data(M, d, ld, r, col, e, sign)
            rs = _quantize_checked(ops, x, d, f"({M}, {d}) ld {ld}, maximum at {name}, e = {e}")
            assert float(rs) == 2.0 ** e


@pytest.mark.parametrize("e", [0, -9])
def test_quantisers_round_every_bf16_value_like_torch(ops, e):
    """Every finite bf16 value of magnitude <= 448, times 2^e: the scale is exactly 2^e, x / s is exact, and the codes are torch's
    round-to-nearest-even cast - ties, subnormals, flushes to zero, both zeros, +-448.  Through the per-tensor quantiser and (one
    448 * 2^e in every row) the per-row quantiser."""
    x = K.quant_all_values(e)
    rs = _quantize_checked(ops, x, x.shape[1], f"all values, e = {e}")
    assert float(rs) == 2.0 ** e
    expect = (x.float() / 2.0 ** e).to(K.E4)
    q, s = ops.quantize_fp8_rows(x.to(DEV))
    torch.cuda.synchronize()
    rq, rrs = fp8_rows_quantize(x)
    assert torch.equal(K.bits(rq), K.bits(expect)) and bool((rrs == 2.0 ** e).all())
    assert torch.equal(K.bits(s).cpu(), K.bits(rrs.reshape(-1)))
    assert K.mismatches(q.cpu(), expect) == 0
    if e == 0:
        assert torch.unique(K.bits(q)).numel() == 254
