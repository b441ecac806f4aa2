"""The kernels of K smoothing on the e4m3-only KV cache (csrc/kv_fp8_center.hip, include/rtv_hip_attn_fp8_only_center.h):
the centred cache write bit for bit against the path it replaces (rtv_qk_norm_rope_cache_ring into a bf16 cache, then
rtv_attn_quantize_kv_centered on the physical segments of the write) on the placements of tests/test_attn_fp8_only_gpu.py, the
mean of the codes against fp64 within the fp32 summation bound and bit for bit against itself, the recentre bit for bit against
tests/attn_fp8_only_center_cases.py, and the refusals, which launch nothing."""
import ctypes
import os

import pytest
import torch

import attn_fp8_cases as fc
import attn_fp8_only_center_cases as oc
from test_attn_fp8_center_gpu import _windows
from test_attn_fp8_only_gpu import GRID, M, PLACEMENTS, RING, ROWS, SCALES, SENTINEL, START, WIDTHS, _inputs, _segments

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
PROFILE = "r25_attn_fp8_only_center_parity.txt"      # under profiles/; a run with RTV_PROFILE_DIR set writes it there
_lines = []


def _note(line):
    print(line)
    _lines.append(line)
    d = os.environ.get("RTV_PROFILE_DIR")
    if d:
        with open(os.path.join(d, PROFILE), "w") as f:
            f.write("\n".join(_lines) + "\n")


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as o
    return o


def _centres(H, which):
    """zero; +-16 on every 8th channel; one that saturates the codes (|k - c| beyond 448 x both k_scales)."""
    g = torch.Generator().manual_seed(H)
    c = torch.zeros(H, 128)
    if which == "offsets":
        c[:, ::8] = 16.0 * torch.where(torch.rand(H, 16, generator=g) < 0.5, -1.0, 1.0)
    elif which == "saturating":
        c = torch.randn(H, 128, generator=g)
        c[:, 5::16] = 1000.0
        c[:, 11::16] = -950.0
    return c.to(DEV)


@pytest.fixture(scope="module")
def bf16_side(ops):
    """(d, H, placement) -> the inputs, the q rows and the bf16 K / V cache of rtv_qk_norm_rope_cache_ring: computed once."""
    memo = {}

    def get(d, H, place):
        if (d, H, place) not in memo:
            row0, ring = PLACEMENTS[place]
            if (d, H) not in memo:
                memo[(d, H)] = _inputs(d, H)
            qkv, wq, wk, cs = memo[(d, H)]
            kc, vc = (torch.zeros(ROWS, H, 128, dtype=BF, device=DEV) for _ in range(2))
            q = ops.qk_norm_rope_cache(qkv, kc, vc, row0, H, wq, wk, cs, GRID, START, ring=ring)
            memo[(d, H, place)] = (qkv, wq, wk, cs, q, kc, vc)
        return memo[(d, H, place)]
    return get


@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("d,H", WIDTHS)
def test_centred_cache_write_equals_the_cache_write_then_the_centred_quantiser(ops, bf16_side, d, H, place):
    row0, ring = PLACEMENTS[place]
    qkv, wq, wk, cs, q_ref, kc, vc = bf16_side(d, H, place)
    segs = _segments(row0, M, ring)
    for which in ("zero", "offsets", "saturating"):
        center = _centres(H, which)
        for k_scale, v_scale in SCALES:
            k8_ref, v8t_ref = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)
            amax_ref = torch.zeros(2, dtype=torch.float32, device=DEV)
            for p0, n in segs:
                ops.attn_quantize_kv(kc, vc, k8_ref, v8t_ref, p0, n, k_scale, v_scale, amax=amax_ref, center=center)
            amax_ref[1] = 0          # (the K kernel leaves V's maximum alone)
            k8 = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)[0]
            amax = torch.zeros(2, dtype=torch.float32, device=DEV)
            q = ops.qk_norm_rope_k8_centered(qkv, k8, row0, H, wq, wk, cs, GRID, START, center, ring=ring, k_scale=k_scale, amax=amax)
            assert torch.equal(q, q_ref), "q_out"
            assert torch.equal(k8, k8_ref), ("k8", which, k_scale)
            assert torch.equal(amax, amax_ref), (amax.tolist(), amax_ref.tolist())
            assert int((k8 != SENTINEL).any(1).any(1).sum()) <= M      # no row beyond the M written
            if which == "zero":      # ... which must also be the plain kernel's bytes
                k8p = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)[0]
                amaxp = torch.zeros(2, dtype=torch.float32, device=DEV)
                qp = ops.qk_norm_rope_k8(qkv, k8p, row0, H, wq, wk, cs, GRID, START, ring=ring, k_scale=k_scale, amax=amaxp)
                assert torch.equal(k8, k8p) and torch.equal(q, qp) and torch.equal(amax, amaxp)
            if which == "saturating":
                written = k8[k8_ref != SENTINEL]
                assert bool(((written & 0x7F) == 0x7E).any()) and float(amax[0]) > 448 * k_scale      # +-448 is there, no NaN code
                assert not bool(oc.is_nan_code(k8).any())
        # without q role and without maxima (the kv_only pass): the same codes
        k8n = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)[0]
        assert ops.qk_norm_rope_k8_centered(qkv, k8n, row0, H, wq, wk, cs, GRID, START, center, ring=ring, k_scale=SCALES[-1][0],
                                            want_q=False) is None
        assert torch.equal(k8n, k8)


# ------------------------------------------------------------------------------------------------ the mean of the codes
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 200, 4680])
def test_mean_of_the_codes(ops, rows, H):
    """Within rows 2^-24 mean|x| + 2^-23 |want| of the fp64 mean: the bound of the bf16 mean kernel's test plus the final addition of
    c_old (its rounding and that of the mean it is added to)."""
    for cache_rows, seg0, seg1 in _windows(rows):
        g = torch.Generator().manual_seed(rows + H)
        k8 = torch.randint(0, 256, (cache_rows, H, 128), generator=g, dtype=torch.uint8)
        k8[:, :, ::8] = (k8[:, :, ::8] & 0x7F) | 0x48     # channels with an offset: positive, >= 4
        k8[oc.is_nan_code(k8)] = 0x7E                     # no NaN code: the quantisers write none
        k8 = k8.to(DEV)
        for k_scale, c_old in ((1.0, None), (2.0, torch.randn(H, 128, generator=g).mul(3).to(DEV))):
            got = ops.attn_k8_center(k8, seg0, seg1, k_scale=k_scale, c_old=c_old)
            again = ops.attn_k8_center(k8, seg0, seg1, k_scale=k_scale, c_old=c_old)
            sel = torch.cat([k8[seg0[0]:seg0[0] + seg0[1]], k8[seg1[0]:seg1[0] + seg1[1]]])
            assert sel.shape[0] == rows
            x = oc.dequantized(sel, k_scale).double()
            want = oc.code_mean(sel, k_scale, c_old)
            bound = rows * 2.0 ** -24 * x.abs().mean(0) + 2.0 ** -23 * want.abs()
            err = (got.double() - want).abs()
            worst = float((err / bound.clamp(min=1e-300)).max())
            _note(f"ATTN_K8_CENTER rows={rows} H={H} k_scale={k_scale:g} c_old={'0' if c_old is None else 'set'} seg0={seg0} seg1={seg1} "
                  f"err/bound={worst:.3f}")
            assert bool((err <= bound).all()), (seg0, seg1, worst)
            assert torch.equal(got, again), "two calls on the same input differ"


def test_mean_of_the_codes_in_place_and_with_a_nan_code(ops):
    """center_new may be c_old; a NaN code makes its own column's mean NaN and no other."""
    H, rows = 2, 300
    g = torch.Generator().manual_seed(3)
    k8 = (torch.randint(0, 0x7E, (rows, H, 128), generator=g, dtype=torch.uint8)).to(DEV)
    c = torch.randn(H, 128, generator=g).to(DEV)
    want = ops.attn_k8_center(k8, (10, 280), k_scale=0.5, c_old=c)
    inplace = c.clone()
    ops.attn_k8_center(k8, (10, 280), k_scale=0.5, c_old=inplace, out=inplace)
    assert torch.equal(inplace, want)
    k8[100, 1, 77] = 0xFF
    got = ops.attn_k8_center(k8, (10, 280), k_scale=0.5, c_old=c)
    nan = torch.isnan(got)
    assert int(nan.sum()) == 1 and bool(nan[1, 77]) and torch.equal(got[~nan], want[~nan])


# ------------------------------------------------------------------------------------------------ the recentre
QH, QROWS = 3, 200
QRANGES = [(0, 64), (5, 70), (63, 65), (130, 200)]


def _recentre_case(seed=11):
    g = torch.Generator().manual_seed(seed)
    k8 = torch.randint(0, 256, (QROWS, QH, 128), generator=g, dtype=torch.uint8)
    k8[:, 0, :] = torch.arange(QROWS * 128, dtype=torch.int64).remainder(256).to(torch.uint8).view(QROWS, 128)      # every code value, NaNs included
    c_old = torch.randn(QH, 128, generator=g)
    c_new = torch.randn(QH, 128, generator=g) * 3
    c_new[:, ::8] += 16.0
    c_new[1, 5] = -2000.0                                                           # saturates
    return k8.to(DEV), c_old.to(DEV), c_new.to(DEV)


@pytest.mark.parametrize("k_scale", [1.0, 0.3])
@pytest.mark.parametrize("a,b", QRANGES)
def test_recentre_equals_the_restatement(ops, a, b, k_scale):
    k8, c_old, c_new = _recentre_case()
    assert all(bool((k8[a:b] == v).any()) for v in range(256)), "a code value is missing from the range"
    want, am_want = k8.clone(), torch.zeros(2, device=DEV)
    oc.recenter_rows(want, a, b - a, c_old, c_new, k_scale, am_want)
    got, am = k8.clone(), torch.zeros(2, device=DEV)
    assert ops.attn_k8_recenter(got, c_old, c_new, a, b - a, k_scale, amax=am) is got
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(got[:a], k8[:a]) and torch.equal(got[b:], k8[b:]), "bytes outside the range"
    assert torch.equal(am, am_want) and float(am[0]) > 448 * k_scale and float(am[1]) == 0.0
    # the same centre: every code stays but -0
    same = k8.clone()
    ops.attn_k8_recenter(same, c_new, c_new, a, b - a, k_scale)
    keep = k8.clone()
    keep[a:b][keep[a:b] == 0x80] = 0
    assert torch.equal(same, keep)


def test_recentre_in_two_calls_equals_one_call(ops):
    """[a, b) then [b, c) equals [a, c), and a second workgroup is reached (rows beyond 256)."""
    g = torch.Generator().manual_seed(5)
    rows, H = 700, 2
    k8 = torch.randint(0, 0x7F, (rows, H, 128), generator=g, dtype=torch.uint8).to(DEV)
    c_old, c_new = torch.randn(H, 128, generator=g).to(DEV), torch.randn(H, 128, generator=g).mul(4).to(DEV)
    a, b, c = 30, 333, 650
    one, two = k8.clone(), k8.clone()
    am1, am2 = (torch.zeros(2, device=DEV) for _ in range(2))
    ops.attn_k8_recenter(one, c_old, c_new, a, c - a, 2.0, amax=am1)
    ops.attn_k8_recenter(two, c_old, c_new, b, c - b, 2.0, amax=am2)      # the later rows first
    ops.attn_k8_recenter(two, c_old, c_new, a, b - a, 2.0, amax=am2)
    want = oc.recenter_rows(k8.clone(), a, c - a, c_old, c_new, 2.0)
    assert torch.equal(one, two) and torch.equal(one, want) and torch.equal(am1, am2)
    assert torch.equal(one[:a], k8[:a]) and torch.equal(one[c:], k8[c:])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(ops):
    from realtime_video_amd import _lib
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, rows = 2, 300
    k8 = torch.full((rows, H, 128), SENTINEL, dtype=torch.uint8, device=DEV)
    c_old = torch.full((H, 128), 1.0, device=DEV)
    center = torch.full((H, 128), 7.0, device=DEV)
    amax = torch.zeros(2, device=DEV)
    ws = torch.full((ops.attn_kv_center_workspace_bytes(rows, H) // 4,), 7.0, device=DEV)

    good = dict(k8=k8.data_ptr(), cache_rows=rows, row0=5, n0=200, row1=250, n1=50, H=H, k_scale=1.0, c_old=c_old.data_ptr(),
                center=center.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() * 4)
    order = list(good)

    def mean(**kw):
        a = dict(good, **kw)
        return lib.rtv_attn_k8_center(*[a[n] for n in order], stream)

    for kw in [dict(k8=0), dict(c_old=0), dict(center=0), dict(ws=0), dict(k8=k8.data_ptr() + 8), dict(c_old=c_old.data_ptr() + 4),
               dict(center=center.data_ptr() + 4), dict(ws=ws.data_ptr() + 8), dict(n0=0), dict(n0=-5), dict(H=0), dict(cache_rows=0),
               dict(n1=-1), dict(row0=-1), dict(row0=101), dict(row1=-1), dict(row1=251), dict(k_scale=0.0), dict(k_scale=float("nan")),
               dict(H=65536), dict(ws_bytes=H * 512 - 4)]:
        assert mean(**kw) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_k8_center:"), kw

    rgood = dict(k8=k8.data_ptr(), cache_rows=rows, row0=5, rows=200, H=H, k_scale=1.0, c_old=c_old.data_ptr(), c_new=center.data_ptr(),
                 amax=amax.data_ptr())
    rorder = list(rgood)

    def move(**kw):
        a = dict(rgood, **kw)
        return lib.rtv_attn_k8_recenter(*[a[n] for n in rorder], stream)

    for kw in [dict(k8=0), dict(c_old=0), dict(c_new=0), dict(k8=k8.data_ptr() + 4), dict(c_old=c_old.data_ptr() + 8),
               dict(c_new=center.data_ptr() + 4), dict(amax=amax.data_ptr() + 2), dict(rows=0), dict(H=0), dict(cache_rows=0), dict(row0=-1),
               dict(row0=101), dict(k_scale=0.0), dict(k_scale=float("inf")), dict(H=65536)]:
        assert move(**kw) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_k8_recenter:"), kw

    # the centred cache write: the list of rtv_qk_norm_rope_k8 and its centre
    d, Hw = WIDTHS[0]
    qkv, wq, wk, cs = _inputs(d, Hw)
    kw8 = torch.full((ROWS, Hw, 128), SENTINEL, dtype=torch.uint8, device=DEV)
    q_out = torch.full((M, d), 7.0, dtype=BF, device=DEV)
    cw = torch.zeros(Hw, 128, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    F, gh, gw = GRID

    def k_call(qkv_p=p(qkv), q_p=p(q_out), k8_p=p(kw8), rows=ROWS, k_scale=1.0, amax_p=p(amax), row0=0, m=M, heads=Hw, ring=(0, 0, 0),
               center_p=p(cw)):
        _lib.call("rtv_qk_norm_rope_k8_centered", qkv_p, q_p, k8_p, rows, k_scale, amax_p, row0, m, d, heads, 1e-6, p(wq), p(wk), p(cs), F, gh,
                  gw, START, 0, *ring, center_p, stream)

    for kw, msg in [(dict(center_p=None), "center must be"), (dict(center_p=ctypes.c_void_p(cw.data_ptr() + 4)), "center must be"),
                    (dict(qkv_p=None), "null pointer"), (dict(k8_p=None), "null pointer"),
                    (dict(k8_p=ctypes.c_void_p(kw8.data_ptr() + 8)), "16-byte aligned"), (dict(amax_p=ctypes.c_void_p(amax.data_ptr() + 2)), "4-byte aligned"),
                    (dict(rows=0), "cache_rows must be positive"), (dict(row0=ROWS - M + 1), r"outside \[0, cache_rows\)"),
                    (dict(rows=244, row0=140, ring=RING), r"outside \[0, cache_rows\)"), (dict(row0=-1), "negative cache row"),
                    (dict(ring=(35, 210, 210)), "bad ring"), (dict(heads=4), "head_dim must be 128"), (dict(m=M + 1), "token grid"),
                    (dict(k_scale=0.0), "finite and positive"), (dict(k_scale=float("nan")), "finite and positive")]:
        with pytest.raises(RuntimeError, match=msg):
            k_call(**kw)

    torch.cuda.synchronize()
    assert bool((k8 == SENTINEL).all()) and bool((center == 7.0).all()) and bool((ws == 7.0).all()) and bool((amax == 0).all())
    assert bool((kw8 == SENTINEL).all()) and bool((q_out == 7.0).all())
    with pytest.raises(ValueError):
        ops.attn_k8_center(k8[:, :, :64], (0, 10))
    with pytest.raises(ValueError):
        ops.attn_k8_recenter(k8, c_old[:1], center)
    assert mean() == 0 and move() == 0          # the unaltered calls run
    k_call()
    torch.cuda.synchronize()
    assert not bool((center == 7.0).any()) and bool((k8[5:205] != SENTINEL).any()) and bool((k8[:5] == SENTINEL).all()) \
        and bool((k8[205:] == SENTINEL).all()) and bool((kw8[:M] != SENTINEL).any()) and bool((kw8[M:] == SENTINEL).all())
