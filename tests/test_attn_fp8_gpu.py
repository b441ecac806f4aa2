"""The fp8 attention kernels (csrc/attn_fp8.hip) against the restatements of tests/attn_fp8_cases.py: the quantiser bit for bit,
the attention kernel against the derived bound on the peaked inputs of tests/attn_cases.py (every launch once plain and once with
NaN codes in every shadow byte outside the key window), its rounding quality against the emulation on the diffuse input, the
refusals, and the plug-in switch of realtime_video_amd.attention.  What the inputs, the bound and the mutants are worth is checked
on the CPU in tests/test_attn_fp8_cpu.py."""
import ctypes
import math

import pytest
import torch

import attn_cases as ac
import attn_fp8_cases as fc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------ quantiser
def _cache(rows, H, interleaved, seed):
    g = torch.Generator().manual_seed(seed)
    arena = (torch.randn(rows, 2, H, 128, generator=g) * 3).to(BF16)
    arena[rows // 2, 0, 0, 5], arena[rows // 3, 1, H - 1, 77] = 1000.0, -2000.0            # beyond 448: saturates, amax shows it
    arena[0, 0, 0, 0], arena[rows - 1, 1, 0, 127] = 2.0 ** -12, -0.0                        # flushes to zero / signed zero
    arena = arena.to(DEV)
    if interleaved:
        return arena[:, 0], arena[:, 1]
    return arena[:, 0].contiguous(), arena[:, 1].contiguous()


CACHES = [(300, 2, False), (300, 2, True), (1100, 2, False), (70, 3, False)]
RANGES = [(0, None), (5, 59), (63, 2), (64, 64), (130, 1)]        # (first row, rows; None = all): those that fit the cache


@pytest.mark.parametrize("rows,H,interleaved", CACHES, ids=lambda v: str(v))
def test_quantiser_bit_for_bit(ops, rows, H, interleaved):
    kc, vc = _cache(rows, H, interleaved, seed=rows + H)
    for scales in ((1.0, 1.0), (0.5, 3.0)):
        for row0, n in RANGES:
            n = rows - row0 if n is None else n
            if row0 + n > rows:
                continue
            k8, v8t = (t.to(DEV) for t in fc.empty_shadow(rows, H, fill=0xAA))
            amax = torch.tensor([0.0, 7.0], device=DEV)
            ops.attn_quantize_kv(kc, vc, k8, v8t, row0, n, *scales, amax=amax)
            k8r, v8tr = (t.to(DEV) for t in fc.empty_shadow(rows, H, fill=0xAA))           # every byte outside the range stays 0xAA
            amax_r = torch.tensor([0.0, 7.0], device=DEV)
            fc.quantize_kv(kc, vc, k8r, v8tr, row0, n, *scales, amax=amax_r)
            assert torch.equal(k8, k8r), (row0, n, scales)
            assert torch.equal(v8t, v8tr), (row0, n, scales)
            assert torch.equal(amax, amax_r), (amax, amax_r)
    # without amax; [a, b) then [b, c) equals [a, c)
    for a, b, c in ((0, 63, rows), (5, 64, 70), (3, 4, 69)):
        k8, v8t = (t.to(DEV) for t in fc.empty_shadow(rows, H, fill=0xAA))
        ops.attn_quantize_kv(kc, vc, k8, v8t, a, b - a)
        ops.attn_quantize_kv(kc, vc, k8, v8t, b, c - b)
        k8o, v8to = (t.to(DEV) for t in fc.empty_shadow(rows, H, fill=0xAA))
        ops.attn_quantize_kv(kc, vc, k8o, v8to, a, c - a)
        assert torch.equal(k8, k8o) and torch.equal(v8t, v8to), (a, b, c)


# ------------------------------------------------------------------------------------------------ kernel against the bound
def _poison(launch, k8, v8t):
    """NaN codes into every k8 / v8t byte of rows outside the key window (the unwritten slots of the last storage tile included)."""
    tiles = v8t.shape[0]
    inside = torch.zeros(tiles * 64, dtype=torch.bool, device=k8.device)
    inside[launch.window_rows(k8.device)] = True
    out_rows = (~inside).nonzero().flatten()
    k8[out_rows[out_rows < k8.shape[0]]] = fc.NAN_CODE
    v8t[out_rows >> 6, :, :, fc.SLOT_MAP.to(k8.device)[out_rows & 63]] = fc.NAN_CODE


def _run(ops, launch, poison=False):
    """Quantiser + kernel on one launch (tensors on the GPU) -> output [Lq, H, 128]."""
    k8, v8t = ops.attn_fp8_shadow(launch.cache_rows, launch.kc.shape[1], DEV)
    ops.attn_quantize_kv(launch.kc, launch.vc, k8, v8t, 0, None, launch.k_scale, launch.v_scale)
    if poison:
        _poison(launch, k8, v8t)
    return ops.attn_fwd_fp8(launch.q, k8, v8t, launch.seg0, launch.seg1, k_scale=launch.k_scale, v_scale=launch.v_scale,
                            causal_block=launch.causal_block, q_offset=launch.q_offset)


def _check(ops, spec, family):
    spec = spec.to(DEV)
    for b in range(spec.q.shape[0]):
        launch = fc.Launch(spec, b)
        ref, E = fc.reference(launch, *launch.shadow())          # the restated shadow: the quantiser has its own test
        for poison in (False, True):
            out = _run(ops, launch, poison)
            ok, ratio = fc.bound_ratio(out, ref, E)
            print(f"ATTN_FP8_RATIO family={family} case={launch.name} poison={int(poison)} ratio={ratio:.3f}")
            assert bool(torch.isfinite(out).all()), f"{launch.name}: non-finite output (poison={poison})"
            assert ok, f"{launch.name}: poison={poison}, err / (E + 2^-8 |ref| + 5e-7) = {ratio:.3f} (accepted: 2)"


@pytest.mark.parametrize("Lq,Lkv,B,offset", ac.EVERY_KEY, ids=lambda v: str(v))
def test_every_key(ops, Lq, Lkv, B, offset):
    _check(ops, ac.spec_every_key(Lq, Lkv, BF16, B, offset), "every_key")


@pytest.mark.parametrize("far", [False, True], ids=["last", "far"])
@pytest.mark.parametrize("Lq,Lkv,cb,off", ac.CAUSAL, ids=lambda v: str(v))
def test_causal(ops, Lq, Lkv, cb, off, far):
    _check(ops, ac.spec_causal(Lq, Lkv, cb, off, BF16, far), "causal")


@pytest.mark.parametrize("Lq,Lkv", ac.OUTSIDE, ids=lambda v: str(v))
def test_outside(ops, Lq, Lkv):
    _check(ops, ac.spec_outside(Lq, Lkv, BF16), "outside")


@pytest.mark.parametrize("seg0,seg1", ac.TWO_RANGE_WINDOWS, ids=lambda v: f"{v[0]}+{v[1]}")
def test_two_ranges(ops, seg0, seg1):
    _check(ops, ac.spec_two_ranges(seg0, seg1, dtype=BF16), "two_ranges")


@pytest.mark.parametrize("Lq,Lkv", ac.STAIRCASE, ids=lambda v: str(v))
def test_staircase(ops, Lq, Lkv):
    _check(ops, ac.spec_staircase(Lq, Lkv, BF16), "staircase")


def test_gaussian_bound_and_rounding_quality(ops):
    """The worst-case bound is loose on diffuse inputs (E is about 1.5 |ref| at the median: a kernel that truncated P instead of
    rounding it would stay inside), so the kernel's rel-L2 against the reference must also stay within 1.25 x that of the
    emulation, whose P is rounded to nearest."""
    spec = ac.spec_gaussian().to(DEV)
    _check(ops, spec, "gaussian")
    launch = fc.Launch(spec)
    k8, v8t = launch.shadow()
    ref, _ = fc.reference(launch, k8, v8t)
    r_kernel, r_emul = fc.rel_l2(_run(ops, launch), ref), fc.rel_l2(fc.emulate(launch, k8, v8t), ref)
    print(f"ATTN_FP8_REL_L2 gaussian kernel={r_kernel:.4e} emulation={r_emul:.4e}")
    assert r_kernel <= 1.25 * r_emul


def test_scales_cancel(ops):
    """k_scale = 2, v_scale = 0.5 against scale 1, on inputs both grids hold exactly (fc.on_both_grids: with N(0, 1) data the two
    shadows would round the values below 2^-6 differently, which is the quantiser's doing and not the kernel's)."""
    spec = fc.on_both_grids(ac.spec_every_key(300, 200, BF16)).to(DEV)
    one, two = fc.Launch(spec), fc.Launch(spec, k_scale=2.0, v_scale=0.5)
    ref1, E1 = fc.reference(one, *one.shadow())
    out1, out2 = _run(ops, one), _run(ops, two)
    ok, ratio = fc.bound_ratio(out2, ref1, E1)
    print(f"ATTN_FP8_RATIO family=scales ratio={ratio:.3f} bit_identical={torch.equal(out1, out2)}")
    assert ok and fc.bound_ratio(out1, ref1, E1)[0]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(ops):
    from realtime_video_amd import _lib
    lib = _lib.load()
    H, rows, Lq = 2, 130, 40
    kc, vc = _cache(rows, H, False, seed=1)
    k8, v8t = ops.attn_fp8_shadow(rows, H, DEV)
    ops.attn_quantize_kv(kc, vc, k8, v8t)
    q = torch.randn(Lq, H, 128, device=DEV).to(BF16)
    out = torch.full((Lq, H, 128), 7.0, dtype=BF16, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rs = H * 128
    good = dict(q=q.data_ptr(), k8=k8.data_ptr(), v8t=v8t.data_ptr(), o=out.data_ptr(), Lq=Lq, H=H, cache_rows=rows, row0=3, n0=60,
                row1=100, n1=20, q_rs=rs, o_rs=rs, scale=0.088, k_scale=1.0, v_scale=1.0, causal_block=0, q_offset=0)
    order = list(good)

    def fwd(**kw):
        a = dict(good, **kw)
        return lib.rtv_attn_fwd_fp8(*[a[n] for n in order], stream)

    bad = [dict(q=0), dict(k8=0), dict(v8t=0), dict(o=0), dict(q=q.data_ptr() + 2), dict(k8=k8.data_ptr() + 8), dict(v8t=v8t.data_ptr() + 4),
           dict(o=out.data_ptr() + 2), dict(Lq=0), dict(Lq=-3), dict(H=0), dict(n0=0), dict(n0=-1), dict(n1=-1), dict(row0=-1),
           dict(row0=100, n0=31), dict(row1=-1), dict(row1=120, n1=11), dict(causal_block=8), dict(scale=0.0), dict(scale=-1.0),
           dict(scale=math.nan), dict(k_scale=math.inf), dict(k_scale=0.0), dict(v_scale=-1.0), dict(v_scale=math.nan),
           dict(q_rs=rs - 8), dict(o_rs=rs + 4)]
    for kw in bad:
        assert fwd(**kw) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_fwd_fp8:"), kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call launched"
    assert fwd() == 0 and fwd(causal_block=8, n1=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())

    k8b, v8tb = (t.to(DEV) for t in fc.empty_shadow(rows, H, fill=0xAA))
    amax = torch.zeros(2, device=DEV)
    qgood = dict(k=kc.data_ptr(), v=vc.data_ptr(), rs=rs, row0=5, rows=100, H=H, k8=k8b.data_ptr(), v8t=v8tb.data_ptr(), cache_rows=rows,
                 k_scale=1.0, v_scale=1.0, amax=amax.data_ptr())
    qorder = list(qgood)

    def quant(**kw):
        a = dict(qgood, **kw)
        return lib.rtv_attn_quantize_kv(*[a[n] for n in qorder], stream)

    qbad = [dict(k=0), dict(v=0), dict(k8=0), dict(v8t=0), dict(k=kc.data_ptr() + 2), dict(v8t=v8tb.data_ptr() + 1), dict(amax=amax.data_ptr() + 2),
            dict(rows=0), dict(rows=-1), dict(H=0), dict(cache_rows=0), dict(row0=-1), dict(row0=31, rows=100), dict(rs=rs - 8), dict(rs=rs + 2),
            dict(k_scale=0.0), dict(k_scale=math.nan), dict(v_scale=math.inf), dict(v_scale=-2.0)]
    for kw in qbad:
        assert quant(**kw) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_quantize_kv:"), kw
    torch.cuda.synchronize()
    assert bool((k8b == 0xAA).all()) and bool((v8tb == 0xAA).all()) and float(amax.abs().sum()) == 0.0, "a refused call launched"
    assert quant() == 0 and quant(amax=0) == 0


# ------------------------------------------------------------------------------------------------ plug-in
def test_plugin_precision_switch(ops):
    from realtime_video_amd import attention as at
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(2, n, 3, 128, generator=g).to(BF16).to(DEV) for n in (150, 333, 333))
    assert at.get_precision() == "bf16"
    before = at.attention(q, k, v)
    sage_before = at.sageattn_func(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2))
    try:
        assert at.set_precision("fp8") == "bf16"
        got = at.attention(q, k, v)
        sage = at.sageattn_func(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2))
        with pytest.raises(ValueError):
            at.set_precision("int8")
    finally:
        at.set_precision("bf16")
    for b in range(2):
        k8, v8t = ops.attn_fp8_shadow(333, 3, DEV)
        ops.attn_quantize_kv(k[b], v[b], k8, v8t)
        want = ops.attn_fwd_fp8(q[b], k8, v8t, (0, 333))
        assert torch.equal(got[b], want) and torch.equal(sage[b].transpose(0, 1), want)
    assert not torch.equal(got, before)
    assert torch.equal(at.attention(q, k, v), before)
    assert torch.equal(at.sageattn_func(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)), sage_before)
