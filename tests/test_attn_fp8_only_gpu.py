"""The two kernels of the e4m3-only KV cache (include/rtv_hip_attn_fp8_only.h) against the path they replace, bit for bit:
rtv_qk_norm_rope_cache_ring into a bf16 cache, then rtv_attn_quantize_kv on the physical segments of the write - and, on the same
bf16 cache, the restatement tests/attn_fp8_cases.quantize_kv.  Both sides' shadows start from a sentinel byte, so bytes that must
stay untouched are compared as well."""
import ctypes

import pytest
import torch

import attn_fp8_cases as fc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
SENTINEL = 0x5A
GRID, START = (3, 5, 7), 2            # F, gh, gw: M = 105 token rows
M = GRID[0] * GRID[1] * GRID[2]
ROWS = 256                            # cache rows: four storage tiles
WIDTHS = [(256, 2), (1536, 12), (5120, 40)]        # the three row-dispatch instantiations the model widths reach (2, 4, 10 chunks per lane)
RING = (35, 210, 70)
# (cache_row0, ring): (a) from row 0; (b) starts and ends inside a storage tile; (c) the write wraps: physical 210..244, then 35..104;
# (d) sink rows 0..34 and ring rows (physical 105..174) in one call
PLACEMENTS = {"a": (0, (0, 0, 0)), "b": (30, (0, 0, 0)), "c": (140, RING), "d": (0, RING)}
SCALES = [(1.0, 1.0), (2.0, 0.5)]


def _segments(row0, n, ring):
    """Physical (first row, rows) of the logical rows [row0, row0 + n), in logical order: the cutting of csrc/dit_forward.hip."""
    S, R, shift = ring
    if R <= 0:
        return [(row0, n)]
    seg = []
    if row0 < S:
        m = min(n, S - row0)
        seg.append((row0, m))
        row0, n = row0 + m, n - m
    if n > 0:
        p0 = S + (row0 - S + shift) % R
        first = min(n, S + R - p0)
        seg.append((p0, first))
        if n > first:
            seg.append((S, n - first))
    return seg


def test_segments_of_the_placements():
    assert _segments(*(140, M), RING) == [(210, 35), (35, 70)] and _segments(0, M, RING) == [(0, 35), (105, 70)]
    assert _segments(30, M, (0, 0, 0)) == [(30, M)]


def _inputs(d, H):
    g = torch.Generator().manual_seed(d)
    qkv = (torch.randn(M, 3 * d, generator=g) * 2.0)
    v = qkv[:, 2 * d:]
    v[3, 5], v[3, 6], v[40, 0], v[77, d - 1], v[104, 17] = 500.0, -500.0, 1000.0, -230.0, 449.0      # beyond +-448 x scale at both scales
    wq, wk = torch.randn(d, generator=g) * 0.1 + 1, torch.randn(d, generator=g) * 0.1 + 1
    from realtime_video_amd.rope import rope_cos_sin_table
    return qkv.to(DEV, BF), wq.to(DEV, BF), wk.to(DEV, BF), rope_cos_sin_table(128).to(DEV)


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as o
    return o


@pytest.fixture(scope="module")
def bf16_side(ops):
    """(d, H, placement) -> the inputs, the q rows and the bf16 K / V cache rtv_qk_norm_rope_cache_ring writes: computed once, never
    modified."""
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
def test_k8_and_v_rows_equal_the_cache_write_then_the_quantiser(ops, bf16_side, d, H, place):
    row0, ring = PLACEMENTS[place]
    qkv, wq, wk, cs, q_ref, kc, vc = bf16_side(d, H, place)
    segs = _segments(row0, M, ring)
    for k_scale, v_scale in SCALES:
        k8_ref, v8t_ref = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)
        k8_re, v8t_re = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)
        amax_ref, amax_re = (torch.zeros(2, dtype=torch.float32, device=DEV) for _ in range(2))
        for p0, n in segs:
            ops.attn_quantize_kv(kc, vc, k8_ref, v8t_ref, p0, n, k_scale, v_scale, amax=amax_ref)
            fc.quantize_kv(kc, vc, k8_re, v8t_re, p0, n, k_scale, v_scale, amax=amax_re)
        assert torch.equal(k8_ref, k8_re) and torch.equal(v8t_ref, v8t_re) and torch.equal(amax_ref, amax_re)      # the reference side agrees with itself
        k8, v8t = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)
        amax = torch.zeros(2, dtype=torch.float32, device=DEV)
        q = ops.qk_norm_rope_k8(qkv, k8, row0, H, wq, wk, cs, GRID, START, ring=ring, k_scale=k_scale, amax=amax)
        src = 0
        for p0, n in segs:
            ops.attn_quantize_v_rows(qkv[src:src + n, 2 * d:].view(n, H, 128), v8t, ROWS, p0, v_scale, amax=amax)
            src += n
        assert torch.equal(q, q_ref), "q_out"
        assert torch.equal(k8, k8_ref), "k8"
        assert torch.equal(v8t, v8t_ref), "v8t"
        assert torch.equal(amax, amax_ref), (amax.tolist(), amax_ref.tolist())
        assert float(amax[1]) == 1000.0 and int((k8 != SENTINEL).any(1).any(1).sum()) <= M      # (the outliers were there; no row beyond the M written)
    # without q role and without maxima (the kv_only pass): the same codes, q_out not needed
    k8n = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)[0]
    assert ops.qk_norm_rope_k8(qkv, k8n, row0, H, wq, wk, cs, GRID, START, ring=ring, k_scale=SCALES[-1][0], want_q=False) is None
    assert torch.equal(k8n, k8)


@pytest.mark.parametrize("d,H", WIDTHS[:1] + WIDTHS[2:])
def test_v_rows_in_two_calls_equal_one_call(ops, d, H):
    """[a, b) then [b, c) equals [a, c), b inside a storage tile and inside a 4-key word: no call writes a neighbour's bytes."""
    qkv = _inputs(d, H)[0]
    v = qkv[:, 2 * d:]
    a, b, c = 30, 77, 135
    one, two = (fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)[1] for _ in range(2))
    am1, am2 = (torch.zeros(2, dtype=torch.float32, device=DEV) for _ in range(2))
    ops.attn_quantize_v_rows(v[:c - a].view(c - a, H, 128), one, ROWS, a, 0.5, amax=am1)
    ops.attn_quantize_v_rows(v[b - a:c - a].view(c - b, H, 128), two, ROWS, b, 0.5, amax=am2)      # the later rows first
    ops.attn_quantize_v_rows(v[:b - a].view(b - a, H, 128), two, ROWS, a, 0.5, amax=am2)
    assert torch.equal(one, two) and torch.equal(am1, am2) and float(am1[0]) == 0.0
    rows = torch.arange(ROWS, device=DEV)
    outside = fc.gather_v(one, rows[(rows < a) | (rows >= c)])
    assert bool((outside == SENTINEL).all()) and bool((fc.gather_v(one, rows[a:c]) == fc.codes(v[:c - a].view(c - a, H, 128), 0.5)).all())


def test_entry_points_refuse_before_any_launch(ops):
    """What include/rtv_hip_attn_fp8_only.h documents as refused raises, and neither q_out nor the shadows have been written."""
    from realtime_video_amd import _lib
    d, H = WIDTHS[0]
    qkv, wq, wk, cs = _inputs(d, H)
    k8, v8t = fc.empty_shadow(ROWS, H, fill=SENTINEL, device=DEV)
    q_out = torch.full((M, d), 7.0, dtype=BF, device=DEV)
    amax = torch.zeros(2, dtype=torch.float32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    F, gh, gw = GRID

    def k_call(qkv_p=p(qkv), q_p=p(q_out), k8_p=p(k8), rows=ROWS, k_scale=1.0, amax_p=p(amax), row0=0, m=M, heads=H, ring=(0, 0, 0), wk_p=p(wk)):
        _lib.call("rtv_qk_norm_rope_k8", qkv_p, q_p, k8_p, rows, k_scale, amax_p, row0, m, d, heads, 1e-6, p(wq), wk_p, p(cs), F, gh, gw, START, 0,
                  *ring, stream)

    for kw, msg in [(dict(qkv_p=None), "null pointer"), (dict(k8_p=None), "null pointer"), (dict(wk_p=None), "null pointer"),
                    (dict(k8_p=ctypes.c_void_p(k8.data_ptr() + 8)), "16-byte aligned"), (dict(q_p=ctypes.c_void_p(q_out.data_ptr() + 2)), "16-byte aligned"),
                    (dict(amax_p=ctypes.c_void_p(amax.data_ptr() + 2)), "4-byte aligned"), (dict(rows=0), "cache_rows must be positive"),
                    (dict(row0=ROWS - M + 1), r"outside \[0, cache_rows\)"), (dict(rows=244, row0=140, ring=RING), r"outside \[0, cache_rows\)"),
                    (dict(row0=-1), "negative cache row"), (dict(ring=(35, 210, 210)), "bad ring"), (dict(row0=141, ring=RING), "beyond the end of the ring"),
                    (dict(heads=4), "head_dim must be 128"), (dict(heads=3), "num_heads"), (dict(m=M + 1), "token grid"),
                    (dict(k_scale=0.0), "finite and positive"), (dict(k_scale=float("inf")), "finite and positive"),
                    (dict(k_scale=float("nan")), "finite and positive")]:
        with pytest.raises(RuntimeError, match=msg):
            k_call(**kw)

    v = qkv[:, 2 * d:]

    def v_call(v_p=p(v), stride=3 * d, rows=M, heads=H, v8t_p=p(v8t), cache_rows=ROWS, row0=0, v_scale=1.0, amax_p=p(amax)):
        _lib.call("rtv_attn_quantize_v_rows", v_p, stride, rows, heads, v8t_p, cache_rows, row0, v_scale, amax_p, stream)

    for kw, msg in [(dict(v_p=None), "null pointer"), (dict(v8t_p=None), "null pointer"), (dict(v_p=ctypes.c_void_p(v.data_ptr() + 2)), "16-byte aligned"),
                    (dict(v8t_p=ctypes.c_void_p(v8t.data_ptr() + 4)), "16-byte aligned"), (dict(amax_p=ctypes.c_void_p(amax.data_ptr() + 1)), "4-byte aligned"),
                    (dict(rows=0), "must be positive"), (dict(heads=0), "must be positive"), (dict(cache_rows=0), "must be positive"),
                    (dict(row0=-1), r"outside \[0, cache_rows\)"), (dict(row0=ROWS - M + 1), r"outside \[0, cache_rows\)"),
                    (dict(stride=d - 8), "row stride"), (dict(stride=3 * d + 4), "row stride"), (dict(v_scale=0.0), "finite and positive"),
                    (dict(v_scale=-1.0), "finite and positive"), (dict(v_scale=float("nan")), "finite and positive"), (dict(heads=65536, stride=65536 * 128), "65535 heads")]:
        with pytest.raises(RuntimeError, match=msg):
            v_call(**kw)
    torch.cuda.synchronize()
    assert bool((k8 == SENTINEL).all()) and bool((v8t == SENTINEL).all()) and bool((q_out == 7.0).all()) and bool((amax == 0).all())
    k_call()                   # the unaltered calls run
    v_call()
    torch.cuda.synchronize()
    assert bool((k8[:M] != SENTINEL).any()) and bool((k8[M:] == SENTINEL).all()) and float(amax[0]) > 0 and float(amax[1]) == 1000.0
