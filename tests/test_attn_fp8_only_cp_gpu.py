"""The two kernels of the code exchange on the e4m3-only KV cache (include/rtv_hip_attn_fp8_only_cp.h), bit for bit: STAGE against
the codes the unsharded writers (rtv_qk_norm_rope_k8, rtv_attn_quantize_v_rows) leave for the same rows, COMMIT against the numpy
restatement of tests/attn_fp8_only_cp_cases.py, and the two together against the unsharded writers on the whole block.  Every array
starts from a sentinel byte, so bytes that must stay untouched are compared as well."""
import ctypes

import numpy as np
import pytest
import torch

import attn_fp8_cases as fc
import attn_fp8_only_cp_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
GRID, START, WORLD, M = cc.STAGE_GRID, cc.STAGE_START, cc.STAGE_WORLD, cc.STAGE_M
S = M // WORLD
SCALES = (2.0, 0.5)


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as o
    return o


def _inputs(d):
    g = torch.Generator().manual_seed(d)
    qkv = torch.randn(M, 3 * d, generator=g) * 2.0
    v = qkv[:, 2 * d:]
    v[3, 5], v[49, 6], v[50, 0], v[99, d - 1], v[149, 17] = 500.0, -500.0, 1000.0, -230.0, 449.0      # beyond +-448 x v_scale, at the shard edges
    wq, wk = torch.randn(d, generator=g) * 0.1 + 1, torch.randn(d, generator=g) * 0.1 + 1
    from realtime_video_amd.rope import rope_cos_sin_table
    return qkv.to(DEV, BF), wq.to(DEV, BF), wk.to(DEV, BF), rope_cos_sin_table(128).to(DEV)


@pytest.fixture(scope="module")
def whole(ops):
    """(d, H) -> the inputs and what the unsharded compact writers leave for the block in a cache of exactly M rows from row 0: the K
    codes [M, d], the V codes un-transposed [M, d], the maxima.  Computed once, never modified."""
    memo = {}

    def get(d, H):
        if d not in memo:
            qkv, wq, wk, cs = _inputs(d)
            k8, v8t = fc.empty_shadow(M, H, fill=cc.SENTINEL, device=DEV)
            amax = torch.zeros(2, dtype=torch.float32, device=DEV)
            ops.qk_norm_rope_k8(qkv, k8, 0, H, wq, wk, cs, GRID, START, k_scale=SCALES[0], amax=amax, want_q=False)
            ops.attn_quantize_v_rows(qkv[:, 2 * d:].view(M, H, 128), v8t, M, 0, SCALES[1], amax=amax)
            v = fc.gather_v(v8t, torch.arange(M, device=DEV))
            memo[d] = (qkv, wq, wk, cs, k8.view(M, d).clone(), v.reshape(M, d).clone(), amax)
        return memo[d]
    return get


def _stage_shard(ops, qkv, kv8, r, H, wk, cs, amax):
    return ops.attn_fp8_stage_kv8(qkv[r * S:(r + 1) * S], kv8, r * S, H, wk, cs, GRID, START, k_scale=SCALES[0], v_scale=SCALES[1], amax=amax)


@pytest.mark.parametrize("d,H", cc.WIDTHS)
def test_stage_equals_the_unsharded_writers_shard_by_shard(ops, whole, d, H):
    qkv, wq, wk, cs, k_ref, v_ref, amax_ref = whole(d, H)
    kv8 = ops.attn_fp8_staging(M, H, WORLD, DEV, fill=cc.SENTINEL)
    assert tuple(kv8.shape) == (WORLD, 2, S, d) and kv8.is_contiguous()
    tables = []
    for n, r in enumerate((1, 2, 0)):                                   # not in rank order: a shard writes its own segment only
        amax = torch.zeros(2, dtype=torch.float32, device=DEV)
        _stage_shard(ops, qkv, kv8, r, H, wk, cs, amax)
        assert torch.equal(kv8[r, 0], k_ref[r * S:(r + 1) * S]), f"K codes of shard {r}"
        assert torch.equal(kv8[r, 1], v_ref[r * S:(r + 1) * S]), f"V codes of shard {r}"
        untouched = [x for x in range(WORLD) if x not in (1, 2, 0)[:n + 1]]
        assert all(bool((kv8[x] == cc.SENTINEL).all()) for x in untouched), f"shard {r} wrote another rank's segment"
        # the maxima of the rows the call wrote: the unsharded writers on those rows alone
        k8_r, v8t_r = fc.empty_shadow(M, H, device=DEV)
        want = torch.zeros(2, dtype=torch.float32, device=DEV)
        ops.qk_norm_rope_k8(qkv[r * S:(r + 1) * S], k8_r, 0, H, wq, wk, cs, GRID, START, row_offset=r * S, k_scale=SCALES[0], amax=want, want_q=False)
        ops.attn_quantize_v_rows(qkv[r * S:(r + 1) * S, 2 * d:].view(S, H, 128), v8t_r, M, r * S, SCALES[1], amax=want)
        assert torch.equal(amax, want), (r, amax.tolist(), want.tolist())
        assert float(amax[1]) == float(qkv[r * S:(r + 1) * S, 2 * d:].float().abs().max())
        tables.append(amax)
    assert torch.equal(torch.stack(tables).amax(0), amax_ref) and float(amax_ref[1]) == 1000.0
    # without maxima: the same codes
    kv8n = ops.attn_fp8_staging(M, H, WORLD, DEV, fill=cc.SENTINEL)
    for r in range(WORLD):
        _stage_shard(ops, qkv, kv8n, r, H, wk, cs, None)
    assert torch.equal(kv8n, kv8)


def _commit_case(ops, name, H, seed=0):
    Mc, world, cache_rows, row0, ring = cc.COMMIT_CASES[name]
    rng = np.random.default_rng(seed + H)
    kv8 = rng.integers(0, 256, size=(world, 2, Mc // world, H * 128), dtype=np.uint8)
    k8, v8t = cc.empty_cache(cache_rows, H)
    cc.commit(kv8, k8, v8t, row0, ring)
    g_k8, g_v8t = fc.empty_shadow(cache_rows, H, fill=cc.SENTINEL, device=DEV)
    ops.attn_fp8_commit_kv8(torch.from_numpy(kv8).to(DEV), g_k8, g_v8t, row0, ring)
    return (k8, v8t), (g_k8.cpu().numpy(), g_v8t.cpu().numpy()), cc.physical_rows(row0, Mc, ring), cache_rows


@pytest.mark.parametrize("name,H", [(n, 2) for n in cc.COMMIT_CASES] + [("sink_ring_one_wrap", 5)])
def test_commit_equals_the_restatement_and_keeps_the_sentinel(ops, name, H):
    (k8, v8t), (g_k8, g_v8t), p, cache_rows = _commit_case(ops, name, H)
    assert np.array_equal(g_k8, k8), "k8"
    assert np.array_equal(g_v8t, v8t), "v8t"
    outside = np.setdiff1d(np.arange(cache_rows), p)
    assert (g_k8[outside] == cc.SENTINEL).all() and (cc.ungather_v(g_v8t, outside) == cc.SENTINEL).all()
    assert not (g_k8[p] == cc.SENTINEL).all(axis=(1, 2)).any()          # every row of the block arrived (random bytes: never a sentinel row)


@pytest.mark.parametrize("name", ["no_ring_partial_tiles", "sink_ring_one_wrap"])
@pytest.mark.parametrize("d,H", cc.WIDTHS)
def test_stage_over_all_shards_then_commit_equals_the_unsharded_writers(ops, whole, d, H, name):
    Mc, world, cache_rows, row0, ring = cc.COMMIT_CASES[name]
    assert (Mc, world) == (M, WORLD)
    qkv, wq, wk, cs = whole(d, H)[:4]
    k8_ref, v8t_ref = fc.empty_shadow(cache_rows, H, fill=cc.SENTINEL, device=DEV)
    amax_ref = torch.zeros(2, dtype=torch.float32, device=DEV)
    ops.qk_norm_rope_k8(qkv, k8_ref, row0, H, wq, wk, cs, GRID, START, ring=ring, k_scale=SCALES[0], amax=amax_ref, want_q=False)
    src = 0
    for p0, n in cc.segments(row0, M, ring):
        ops.attn_quantize_v_rows(qkv[src:src + n, 2 * d:].view(n, H, 128), v8t_ref, cache_rows, p0, SCALES[1], amax=amax_ref)
        src += n
    kv8 = ops.attn_fp8_staging(M, H, WORLD, DEV, fill=cc.SENTINEL)
    amax = torch.zeros(2, dtype=torch.float32, device=DEV)
    for r in range(WORLD):
        _stage_shard(ops, qkv, kv8, r, H, wk, cs, amax)
    k8, v8t = fc.empty_shadow(cache_rows, H, fill=cc.SENTINEL, device=DEV)
    ops.attn_fp8_commit_kv8(kv8, k8, v8t, row0, ring)
    assert torch.equal(k8, k8_ref), "k8"
    assert torch.equal(v8t, v8t_ref), "v8t"
    assert torch.equal(amax, amax_ref), (amax.tolist(), amax_ref.tolist())


def test_entry_points_refuse_before_any_launch(ops):
    """What include/rtv_hip_attn_fp8_only_cp.h documents as refused raises with its message, and nothing has been written."""
    from realtime_video_amd import _lib
    d, H = cc.WIDTHS[0]
    qkv, wq, wk, cs = _inputs(d)
    _, _, cache_rows, row0, ring = cc.COMMIT_CASES["sink_ring_one_wrap"]
    kv8 = ops.attn_fp8_staging(M, H, WORLD, DEV, fill=cc.SENTINEL)
    k8, v8t = fc.empty_shadow(cache_rows, H, fill=cc.SENTINEL, device=DEV)
    amax = torch.zeros(2, dtype=torch.float32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    F, gh, gw = GRID

    def stage(qkv_p=p(qkv), kv8_p=p(kv8), world=WORLD, begin=0, count=S, k_scale=1.0, v_scale=1.0, amax_p=p(amax), heads=H, wk_p=p(wk), start=START):
        _lib.call("rtv_attn_fp8_stage_kv8", qkv_p, kv8_p, world, begin, count, k_scale, v_scale, amax_p, d, heads, 1e-6, wk_p, p(cs), F, gh, gw,
                  start, stream)

    bad = (0.0, -1.0, float("inf"), float("nan"))
    for kw, msg in [(dict(kv8_p=None), "null pointer"), (dict(qkv_p=None), "null pointer"), (dict(wk_p=None), "null pointer"),
                    (dict(kv8_p=p(kv8, 8)), "16-byte aligned"), (dict(qkv_p=p(qkv, 2)), "16-byte aligned"), (dict(amax_p=p(amax, 2)), "4-byte aligned"),
                    (dict(world=4), "multiple of world"), (dict(world=0), "multiple of world"),
                    (dict(begin=M - S + 1), r"outside \[0, M\)"), (dict(begin=-1), r"outside \[0, M\)"), (dict(count=0), r"outside \[0, M\)"),
                    (dict(begin=S - 1, count=2), "one rank's segment"), (dict(heads=4), "head_dim must be 128"),
                    (dict(start=1024), "RoPE table")] \
            + [(dict(k_scale=s), "finite and positive") for s in bad] + [(dict(v_scale=s), "finite and positive") for s in bad]:
        with pytest.raises(RuntimeError, match=msg):
            stage(**kw)

    def commit(kv8_p=p(kv8), world=WORLD, m=M, heads=H, k8_p=p(k8), v8t_p=p(v8t), rows=cache_rows, r0=row0, rg=ring):
        _lib.call("rtv_attn_fp8_commit_kv8", kv8_p, world, m, heads, k8_p, v8t_p, rows, r0, *rg, stream)

    for kw, msg in [(dict(kv8_p=None), "null pointer"), (dict(k8_p=None), "null pointer"), (dict(v8t_p=None), "null pointer"),
                    (dict(kv8_p=p(kv8, 4)), "16-byte aligned"), (dict(k8_p=p(k8, 8)), "16-byte aligned"), (dict(v8t_p=p(v8t, 1)), "16-byte aligned"),
                    (dict(world=4), "multiple of world"), (dict(m=0), "multiple of world"), (dict(heads=0), "H must be"), (dict(heads=65536), "H must be"),
                    (dict(rows=0), "cache_rows must be positive"), (dict(r0=-1), "cache_row0 non-negative"),
                    (dict(rg=(64, 256, 256)), "bad ring"), (dict(rg=(-1, 256, 0)), "bad ring"),
                    (dict(rg=(0, 0, 0), r0=cache_rows - M + 1), r"outside \[0, cache_rows\)"),          # no ring: the window ends past the cache
                    (dict(rows=319), r"outside \[0, cache_rows\)"),                                       # the ring ends past the cache
                    (dict(r0=171), r"outside \[0, cache_rows\)")]:                                        # the block ends past the ring
        with pytest.raises(RuntimeError, match=msg):
            commit(**kw)
    torch.cuda.synchronize()
    assert all(bool((t == cc.SENTINEL).all()) for t in (kv8, k8, v8t)) and bool((amax == 0).all())
    stage()                    # the unaltered calls run
    commit()
    torch.cuda.synchronize()
    assert bool((kv8[0] != cc.SENTINEL).any()) and bool((kv8[1:] == cc.SENTINEL).all()) and float(amax[0]) > 0 and float(amax[1]) > 0
    assert bool((k8[cc.physical_rows(row0, M, ring)[:S]] != cc.SENTINEL).any())
