"""CPU proof that tests/test_gemm_fp8_exact_gpu.py would notice: for every case of tests/gemm_fp8_cases.py the exactness
condition holds (lossless e4m3 operands, every partial sum below 2^24, the scaled sum representable in fp32), plan() gives the
recorded split-K plan at 256 compute units, every named slip changes the reference of every case listed as covering it, every
slip is covered, and the quantiser's data set meets its conditions."""
import functools

import pytest
import torch

import gemm_fp8_cases as K

SMALL_CASES = [c for c in K.GEMM_CASES if not c.big]
KERNELS = (K.ROWS, K.TENSOR)


@functools.lru_cache(maxsize=None)
def _built(c, launch=0):
    return K.build(c, launch)


@pytest.mark.parametrize("c", K.GEMM_CASES, ids=lambda c: c.name)
def test_plan_gives_the_recorded_plan(c):
    assert c.K % K.BK == 0 and c.N % 8 == 0
    assert K.plan(c.tiles, c.nk, K.G_PLAN) == c.plan
    R, S, _ = c.plan
    if S > 1:
        segs = K.segments(c.nk, S)
        assert segs[0][0] == 0 and segs[-1][1] == c.nk and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert min(e - b for b, e in segs) >= 4 and R * S <= K.SPLIT_MAX_UNITS


def test_plans_the_cases_are_named_for():
    """The depth table: 1, 2, 3 and 5 K-tiles unsplit, then S = 2, S = 3 with segments of 4, 4 and 5 K-tiles, S = 8; a single
    split tile; a short last supertile group; more tiles than compute units with the split units first and last; ragged last
    row and column tiles throughout."""
    assert [(c.nk, c.plan[1]) for c in K.DEPTH_CASES] == [(1, 1), (2, 1), (3, 1), (5, 1), (8, 2), (13, 3), (32, 8)]
    assert K.segments(13, 3) == [(0, 4), (4, 8), (8, 13)]
    assert all(c.tiles == 4 and c.M % K.BM == 1 and c.N % K.BN == 8 for c in K.DEPTH_CASES)
    assert [(c.tiles, c.plan) for c in K.MIN_CASES] == [(1, (0, 1, 0)), (1, (1, 2, 1))]
    short, first, last = K.TILE_MAP_CASES
    assert (short.tiles_m, short.tiles_n) == (9, 3) and short.tiles_m % K.GROUP_M == 1
    assert (first.tiles, first.plan) == (285, (29, 2, 1)) and (last.tiles, last.plan) == (296, (40, 2, 0))
    assert all(c.M % K.BM and c.N % K.BN and c.needs_g_plan == (c is not short) for c in K.TILE_MAP_CASES)
    assert [c.needs_g_plan for c in K.DEPTH_CASES] == [False] * 4 + [True] * 3
    assert [c.K for c in K.DIRECT_STORE_CASES] == [384, 1664] and [c.plan[1] for c in K.STRIDED_CASES] == [1, 2]


def test_plan_follows_the_compute_unit_count():
    """Why a split case checks the count before it runs: the same problem takes other plans on other chips."""
    assert K.plan(285, 8, 256) == (29, 2, 1) and K.plan(285, 8, 304) == (0, 1, 0) and K.plan(285, 8, 128) == (29, 2, 0)
    assert K.plan(4, 32, 256) == (4, 8, 1) and K.plan(4, 32, 64) == (4, 8, 0) and K.plan(256, 32, 256) == (0, 1, 0)
    assert K.plan(200, 32, 256) == (0, 1, 0)                  # G / R = 1: nothing to gain
    assert K.plan(100, 2048, 256) == (100, 2, 0) and K.plan(129, 2048, 256) == (0, 1, 0)


@pytest.mark.parametrize("c", SMALL_CASES, ids=lambda c: c.name)
def test_case_is_exact_and_every_covering_slip_shows(c):
    o, prev = _built(c, 1), _built(c, 0)                      # the second launch of the GPU test and the one before it
    assert 0 < o.max_int < K.EXACT_MAX and not torch.equal(o.a, prev.a)
    assert torch.equal(o.isum.float().double(), o.isum)
    for kernel in KERNELS:
        for use_bias in (False, True):
            good = K.reference(c, o, kernel, use_bias)        # asserts: representable in fp32
            assert good.dtype == K.BF and bool(torch.isfinite(good).all())
            for slip in K.covering_slips(c, kernel):
                bad = K.reference(c, o, kernel, use_bias, slip=slip, previous=prev)
                changed = K.mismatches(bad, good)
                print(f"{c.name} [{kernel}{', bias' if use_bias else ''}]: {slip}: {changed} of {good.numel()} outputs change")
                # (under the per-row scales a bias of order 1 hides the sums of the rows and columns with the smallest scales)
                assert changed >= (1 if use_bias else max(1, good.numel() // 4)), (c.name, kernel, slip, changed)


def test_bound_at_the_deepest_case():
    """K = 4096 with |a|, |w| <= 8: no sum of products can pass 4096 * 64 = 2^18."""
    c = K.by_name("depth_257_264_4096")
    assert c.K * 8 * 8 == 262144 < K.EXACT_MAX and _built(c).max_int <= 262144


def test_every_slip_is_covered_by_a_case():
    seen = {"gate_without_row_offset"}                        # the epilogue case: test_epilogue_case_and_its_slip
    for c in SMALL_CASES:
        for kernel in KERNELS:
            seen.update(K.covering_slips(c, kernel))
    assert seen == set(K.SLIPS)


def test_big_cases_are_listed_with_the_slips_of_a_small_twin():
    """The two cases with more tiles than compute units are too large for a CPU slip proof; they are depth_257_264_1024 at other
    sizes (same K, same S = 2), so the slips proven there are the ones they cover, and their exactness is asserted where their
    reference is evaluated."""
    small = K.by_name("depth_257_264_1024")
    for big in (c for c in K.GEMM_CASES if c.big):
        assert (big.K, big.plan[1]) == (small.K, small.plan[1])
        assert all(set(K.covering_slips(big, k)) == set(K.covering_slips(small, k)) - {"padding_column_read"} for k in KERNELS)
        assert big.K * 64 < K.EXACT_MAX


def test_epilogue_case_and_its_slip():
    p = K.epilogue_problem()
    M, N, rpf = p["M"], p["N"], p["rpf"]
    assert (M, N, rpf) == (300, 264, 101) and int(p["aq"].view(torch.uint8).max()) == 0
    wc = p["wq"].view(torch.uint8)
    assert not bool(((wc & 0x7F) == K.NAN_CODE).any()) and bool(torch.isfinite(p["wq"].float()).all())
    assert torch.unique(wc).numel() >= 250
    whole = K.epilogue_reference(p)
    by_hand = torch.stack([(p["res"][m].float() + (p["bias"].float() * p["gate"][m // rpf].float()).to(K.BF).float()).to(K.BF)
                           for m in range(M)])
    assert torch.equal(K.bits(whole), K.bits(by_hand))
    rows = 2 * rpf
    good = K.epilogue_reference(p, rows, rpf)
    bad = K.epilogue_reference(p, rows, rpf, slip="gate_without_row_offset")
    assert torch.equal(K.bits(bad), K.bits(whole[:rows])) and K.mismatches(bad, good) >= rows * N // 2


def test_guarded_layouts_on_the_cpu():
    c = K.STRIDED_CASES[0]
    o = _built(c)
    buf, a = K.guarded_operand(o.aq, K.PAD_A, "cpu")
    assert a.stride(0) == c.K + 16 and a.stride(1) == 1 and torch.equal(K.bits(a), K.bits(o.aq))
    raw = buf.view(torch.uint8)
    assert raw.shape == (c.M + 128, c.K + 16) and bool((raw[:64] == 0x7F).all()) and bool((raw[-64:] == 0x7F).all())
    assert bool((raw[64:-64, c.K:] == 0x7F).all()) and bool(torch.isnan(buf[0, 0].float()))
    _, w = K.guarded_operand(o.wq, K.PAD_W, "cpu")
    assert w.stride(0) == c.K + 32
    for offset, row_rest in ((8, 0), (4, 8)):
        ob, out = K.guarded_output(c.M, c.N, "cpu", offset)
        assert out.shape == (c.M, c.N) and (out.data_ptr() - ob.data_ptr()) % 16 == row_rest and (out.stride(0) * 2) % 16 == 0
        assert K.guards_changed(ob, c.N, offset) == 0
        out.zero_()
        assert K.guards_changed(ob, c.N, offset) == 0
        ob[3, offset - 1] = 0
        ob[5, offset + c.N] = 0
        assert K.guards_changed(ob, c.N, offset) == 2
    assert K.mismatches(torch.tensor([0.0, 1.0]).to(K.BF), torch.tensor([-0.0, 1.0]).to(K.BF)) == 1     # bit patterns, not values


def test_quantiser_data_set():
    vals = K.all_bf16_values()
    assert vals.numel() == 34754 == 2 * (135 * 128 + 97)
    x = K.quant_all_values(0)                                 # asserts: 448 * fp32(1 / 448) == 1, all 254 non-NaN codes occur
    assert x.shape == (129, K.QUANT_WIDTH) and K.QUANT_WIDTH % 16 == 0 and bool((x[:, 0] == 448).all())
    q, s = K.quantize_tensor_restated(x)
    assert float(s) == 1.0 and torch.equal(K.bits(q), K.bits(x.float().to(K.E4)))
    f = x.float()
    codes = K.bits(q)
    assert int(((f == 0) & (codes == 0x80)).sum()) >= 1 and int(((f == 0) & (codes == 0)).sum()) >= 1       # both zeros
    assert int(((f != 0) & ((codes & 0x7F) == 0)).sum()) > 1000                                             # flushes to zero
    assert int((((codes & 0x78) == 0) & ((codes & 0x07) != 0)).sum()) > 100                                 # subnormal codes
    back = q.float()
    ties = (back != f) & ((f - back).abs() == (q.view(torch.uint8) ^ 1).view(K.E4).float().sub(f).abs())
    assert int(ties.sum()) > 100                                                                            # ties (halfway values)
    assert int((codes == 0x7E).sum()) >= 129 and int((codes == 0xFE).sum()) >= 1                            # +-448
    for e in (-9,):
        xe = K.quant_all_values(e)
        qe, se = K.quantize_tensor_restated(xe)
        assert float(se) == 2.0 ** e and torch.unique(K.bits(qe)).numel() == 254
        rq = (xe.float() / 2.0 ** e).to(K.E4)
        assert torch.equal(K.bits(qe), K.bits(rq))


@pytest.mark.parametrize("M,d,ld", K.QUANT_SHAPES)
def test_quantiser_shape_data(M, d, ld):
    assert d % 16 == 0 and ld % 8 == 0
    for name, r, col in K.quant_peaks(M, d):
        for e, sign in ((0, 1.0), (-9, -1.0)):
            x = K.quant_shape_data(M, d, ld, r, col, e, sign)
            q, s = K.quantize_tensor_restated(x[:, :d])
            assert float(s) == 2.0 ** e and int(K.bits(q)[r, col]) == (0x7E if sign > 0 else 0xFE)
            assert int(((K.bits(q) & 0x7F) == 0x7E).sum()) == 1
            if ld > d:                                        # a read of the padding would move the scale
                assert float(K.quantize_tensor_restated(x)[1]) > 1e30
    assert [n for n, _, _ in K.quant_peaks(M, d)] == ["first", "last"] + (["row_1024"] if M > 1024 else [])
