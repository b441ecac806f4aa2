"""The K smoothing kernels (csrc/attn_fp8.hip, include/rtv_hip_attn_fp8_center.h) against tests/attn_fp8_center_cases.py: the
column-mean kernel against fp64 within the fp32 summation bound and bit for bit against itself, the centred quantiser bit for bit
against the restatement, and the unchanged attention kernel on a centred shadow - inside the bound of tests/attn_fp8_cases.py
against the reference on the centred codes, and at most half the plain shadow's error against the fp64 definition."""
import ctypes
import math
import os

import pytest
import torch

import attn_cases as ac
import attn_fp8_cases as fc
import attn_fp8_center_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
PROFILE = "r20_attn_fp8_center_parity.txt"      # under profiles/; a run with RTV_PROFILE_DIR set writes it there


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


def _k_cache(cache_rows, H, interleaved, seed):
    """A K cache [cache_rows, H, 128] with channel offsets, dense or the K plane of an interleaved arena whose V plane is poison."""
    k = cc.structured_k(cache_rows, H, 16.0, seed=seed)
    if not interleaved:
        return k.to(DEV)
    arena = torch.full((cache_rows, 2, H, 128), 3.0e4, dtype=BF16)
    arena[:, 0] = k
    return arena.to(DEV)[:, 0]


# ------------------------------------------------------------------------------------------------ the mean kernel
def _windows(rows):
    """(cache_rows, seg0, seg1) for a window of `rows` rows: one range that starts inside a storage tile, two ranges with a gap, and
    the wrapped pair of a ring behind 70 sink rows - the tail of the cache first, then rows from 70 on (inside storage tile 1)."""
    out = [(rows + 101, (37, rows), (0, 0))]
    if rows >= 2:
        n1 = max(1, rows // 3)
        n0 = rows - n1
        out.append((rows + 150, (3, n0), (n0 + 90, n1)))
        cache_rows = 70 + rows + 50
        out.append((cache_rows, (cache_rows - n0, n0), (70, n1)))
    return out


@pytest.mark.parametrize("interleaved", [False, True], ids=["dense", "arena"])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 200, 4680])
def test_mean_kernel(ops, rows, H, interleaved):
    for cache_rows, seg0, seg1 in _windows(rows):
        k = _k_cache(cache_rows, H, interleaved, seed=rows + H)
        assert k.stride(0) == (2 if interleaved else 1) * H * 128
        got = ops.attn_kv_center(k, seg0, seg1)
        again = ops.attn_kv_center(k, seg0, seg1)
        sel = torch.cat([k[seg0[0]:seg0[0] + seg0[1]], k[seg1[0]:seg1[0] + seg1[1]]]).double()
        assert sel.shape[0] == rows
        want = sel.mean(0)
        bound = rows * 2.0 ** -24 * sel.abs().mean(0)
        err = (got.double() - want).abs()
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"ATTN_KV_CENTER rows={rows} H={H} arena={int(interleaved)} seg0={seg0} seg1={seg1} err/bound={worst:.3f}")
        assert bool((err <= bound).all()), (seg0, seg1, worst)
        assert torch.equal(got, again), "two calls on the same input differ"


def test_mean_kernel_refusals_launch_nothing(ops):
    from realtime_video_amd import _lib
    lib = _lib.load()
    H, rows = 2, 300
    k = _k_cache(rows, H, False, seed=1)
    center = torch.full((H, 128), 7.0, device=DEV)
    ws = torch.full((ops.attn_kv_center_workspace_bytes(rows, H) // 4,), 7.0, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(k=k.data_ptr(), rs=H * 128, row0=5, n0=200, row1=250, n1=50, H=H, center=center.data_ptr(), ws=ws.data_ptr(),
                ws_bytes=ws.numel() * 4)
    order = list(good)

    def mean(**kw):
        a = dict(good, **kw)
        return lib.rtv_attn_kv_center(*[a[n] for n in order], stream)

    bad = [dict(k=0), dict(center=0), dict(ws=0), dict(k=k.data_ptr() + 2), dict(center=center.data_ptr() + 4), dict(ws=ws.data_ptr() + 8),
           dict(n0=0), dict(n0=-5), dict(H=0), dict(n1=-1), dict(row0=-1), dict(row1=-1), dict(rs=H * 128 - 8), dict(rs=H * 128 + 4),
           dict(ws_bytes=H * 512 - 4), dict(n0=256, n1=1, ws_bytes=H * 1024 - 4)]
    for kw in bad:
        assert mean(**kw) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_kv_center:"), kw
    torch.cuda.synchronize()
    assert bool((center == 7.0).all()) and bool((ws == 7.0).all()), "a refused call launched"
    with pytest.raises(ValueError):
        ops.attn_kv_center(k, (100, 201))
    with pytest.raises(ValueError):
        ops.attn_kv_center(k, (0, 10), (295, 6))
    assert mean() == 0
    torch.cuda.synchronize()
    assert not bool((center == 7.0).any())


# ------------------------------------------------------------------------------------------------ the centred quantiser
QH, QROWS = 3, 200
QRANGES = [(0, 64), (5, 70), (63, 65), (130, 200)]


def _kv(interleaved, seed=7):
    g = torch.Generator().manual_seed(seed)
    arena = torch.empty(QROWS, 2, QH, 128, dtype=BF16)
    arena[:, 0] = cc.structured_k(QROWS, QH, 16.0, seed=seed)
    arena[:, 1] = (torch.randn(QROWS, QH, 128, generator=g) * 3).to(BF16)
    arena[QROWS // 2, 0, 0, 5], arena[QROWS // 3, 1, QH - 1, 77] = 1000.0, -2000.0        # saturate; amax shows it
    arena[0, 0, 0, 0], arena[QROWS - 1, 0, 1, 127] = 2.0 ** -12, -0.0
    arena = arena.to(DEV)
    if interleaved:
        return arena[:, 0], arena[:, 1]
    return arena[:, 0].contiguous(), arena[:, 1].contiguous()


@pytest.mark.parametrize("interleaved", [False, True], ids=["dense", "arena"])
def test_centred_quantiser_bit_for_bit(ops, interleaved):
    kc, vc = _kv(interleaved)
    g = torch.Generator().manual_seed(3)
    center_dev = ((torch.rand(QH, 128, generator=g) * 2 - 1) * 32).to(DEV)
    center = center_dev.cpu().to(DEV)                                                     # as read back from the device
    for scales in ((1.0, 1.0), (0.5, 3.0)):
        for a, b in QRANGES:
            k8, v8t = (t.to(DEV) for t in fc.empty_shadow(QROWS, QH, fill=0xA5))
            amax = torch.zeros(2, device=DEV)
            ops.attn_quantize_kv(kc, vc, k8, v8t, a, b - a, *scales, amax=amax, center=center_dev)
            k8r, v8tr = (t.to(DEV) for t in fc.empty_shadow(QROWS, QH, fill=0xA5))        # every byte outside the range stays 0xA5
            amax_r = torch.zeros(2, device=DEV)
            cc.quantize_kv_centered(kc, vc, k8r, v8tr, a, b - a, center, *scales, amax=amax_r)
            assert torch.equal(k8, k8r), (a, b, scales)
            assert torch.equal(v8t, v8tr), (a, b, scales)
            assert torch.equal(amax, amax_r), (amax, amax_r)
            assert float(amax[0]) == float((kc[a:b].float() - center).abs().max())
            out_rows = torch.ones(QROWS, dtype=torch.bool, device=DEV)
            out_rows[a:b] = False
            assert bool((k8[out_rows] == 0xA5).all())
            assert bool((fc.gather_v(v8t, out_rows.nonzero().flatten()) == 0xA5).all())
    # [a, b) then [b, c) equals [a, c), without amax
    for a, b, c in ((0, 63, QROWS), (5, 64, 70), (3, 4, 69), (63, 64, 65)):
        k8, v8t = (t.to(DEV) for t in fc.empty_shadow(QROWS, QH, fill=0xA5))
        ops.attn_quantize_kv(kc, vc, k8, v8t, a, b - a, center=center_dev)
        ops.attn_quantize_kv(kc, vc, k8, v8t, b, c - b, center=center_dev)
        k8o, v8to = (t.to(DEV) for t in fc.empty_shadow(QROWS, QH, fill=0xA5))
        ops.attn_quantize_kv(kc, vc, k8o, v8to, a, c - a, center=center_dev)
        assert torch.equal(k8, k8o) and torch.equal(v8t, v8to), (a, b, c)
    # a zero centre: the plain quantiser's bytes and maxima
    zero = torch.zeros(QH, 128, device=DEV)
    for a, b in QRANGES:
        outs = []
        for center_arg in (zero, None):
            k8, v8t = (t.to(DEV) for t in fc.empty_shadow(QROWS, QH, fill=0xA5))
            amax = torch.zeros(2, device=DEV)
            ops.attn_quantize_kv(kc, vc, k8, v8t, a, b - a, 0.5, 3.0, amax=amax, center=center_arg)
            outs.append((k8, v8t, amax))
        assert all(torch.equal(x, y) for x, y in zip(*outs)), (a, b)


def test_centred_quantiser_refusals_launch_nothing(ops):
    kc, vc = _kv(False)
    k8, v8t = (t.to(DEV) for t in fc.empty_shadow(QROWS, QH, fill=0xA5))
    center = torch.zeros(QH, 128, device=DEV)
    for bad in (torch.zeros(QH, 64, device=DEV), torch.zeros(QH, 128, device=DEV, dtype=torch.float64), torch.zeros(QH + 1, 128, device=DEV),
                torch.zeros(QH, 129, device=DEV)[:, 1:]):
        with pytest.raises(ValueError):
            ops.attn_quantize_kv(kc, vc, k8, v8t, 0, 64, center=bad)
    with pytest.raises(RuntimeError, match="attn_quantize_kv: row range"):
        ops.attn_quantize_kv(kc, vc, k8, v8t, 190, 20, center=center)
    with pytest.raises(RuntimeError, match="attn_quantize_kv: scales"):
        ops.attn_quantize_kv(kc, vc, k8, v8t, 0, 64, k_scale=0.0, center=center)
    torch.cuda.synchronize()
    assert bool((k8 == 0xA5).all()) and bool((v8t == 0xA5).all()), "a refused call launched"


# ------------------------------------------------------------------------------------------------ the kernel on a centred shadow
def test_attention_kernel_on_a_centred_shadow(ops):
    """rtv_attn_fwd_fp8, unchanged, on the biased operands (offset 16 on every 8th K channel): Lq = 96 over the 200 keys from
    physical row 37 on, H = 2, the centre from the mean kernel over that window.  Inside the bound of tests/attn_fp8_cases.py against
    the reference on the centred codes; against the fp64 definition on the bf16 operands at most 0.5 x the plain shadow's rel-L2."""
    Lq, Lkv, H, first = 96, 200, 2, 37
    q, k, v = cc.biased_operands(Lq, Lkv, H, 16.0)
    cache_rows = first + Lkv + 23
    g = torch.Generator().manual_seed(5)
    kb, vb = (torch.randn(1, cache_rows, H, 128, generator=g).to(BF16) for _ in range(2))   # rows outside the window: other keys
    kb[0, first:first + Lkv], vb[0, first:first + Lkv] = k, v
    spec = ac.Spec("biased[96x200@37]", q[None], kb, vb, (first, Lkv)).to(DEV)
    launch = fc.Launch(spec)
    center = ops.attn_kv_center(launch.kc, launch.seg0)
    definition = cc.definition(*(t[None].to(DEV) for t in (q, k, v)))[0]

    k8, v8t = ops.attn_fp8_shadow(cache_rows, H, DEV)
    ops.attn_quantize_kv(launch.kc, launch.vc, k8, v8t)
    plain = ops.attn_fwd_fp8(launch.q, k8, v8t, launch.seg0)
    ok_plain, _ = fc.bound_ratio(plain, *fc.reference(launch, k8, v8t))

    k8c, v8tc = ops.attn_fp8_shadow(cache_rows, H, DEV)
    ops.attn_quantize_kv(launch.kc, launch.vc, k8c, v8tc, center=center)
    k8r, v8tr = fc.empty_shadow(cache_rows, H, device=DEV)
    cc.quantize_kv_centered(launch.kc, launch.vc, k8r, v8tr, 0, cache_rows, center.cpu().to(DEV))
    assert torch.equal(k8c, k8r) and torch.equal(v8tc, v8tr) and torch.equal(v8tc, v8t)
    smooth = ops.attn_fwd_fp8(launch.q, k8c, v8tc, launch.seg0)
    ok, ratio = fc.bound_ratio(smooth, *fc.reference(launch, k8r, v8tr))

    r_plain, r_smooth = fc.rel_l2(plain, definition), fc.rel_l2(smooth, definition)
    line = (f"fp8 attention, Lq=96 over 200 keys from physical row 37, H=2, K = N(0,1) + offset 16 on every 8th channel; rel-L2 against "
            f"the fp64 definition on the bf16 operands: plain shadow {r_plain:.4f}, centred shadow {r_smooth:.4f}, ratio "
            f"{r_smooth / r_plain:.3f} (accepted: 0.5); err / bound of the centred launch against the reference on its codes {ratio:.3f} "
            f"(accepted: 2)")
    print("ATTN_FP8_CENTER_PARITY", line)
    if os.environ.get("RTV_PROFILE_DIR"):                                                  # how profiles/r20_attn_fp8_center_parity.txt was made
        with open(os.path.join(os.environ["RTV_PROFILE_DIR"], PROFILE), "w") as f:
            f.write(line + "\n")
    assert ok_plain and ok, ratio
    assert bool(torch.isfinite(smooth).all())
    assert r_smooth <= 0.5 * r_plain
    assert not math.isclose(r_plain, r_smooth)
