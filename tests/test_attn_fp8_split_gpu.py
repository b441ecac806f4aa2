"""The KV split of the fp8 attention kernel (rtv_attn_fwd_fp8_split, csrc/attn_fp8.hip) on the inputs of
tests/attn_fp8_split_cases.py: every launch once plain and once with NaN codes in every shadow byte outside the key window, against
the unchanged bound of tests/attn_fp8_cases.py; one range bit for bit the unsplit kernel; two launches bit for bit each other; the
rounding quality on the diffuse input; the refusals.  What the inputs, the bound and the mutants are worth is checked on the CPU in
tests/test_attn_fp8_split_cpu.py."""
import ctypes

import pytest
import torch

import attn_cases as ac
import attn_fp8_cases as fc
import attn_fp8_split_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


def _poison(launch, k8, v8t):
    """NaN codes into every k8 / v8t byte of rows outside the key window (the rule of tests/test_attn_fp8_gpu.py)."""
    inside = torch.zeros(v8t.shape[0] * 64, dtype=torch.bool, device=k8.device)
    inside[launch.window_rows(k8.device)] = True
    out_rows = (~inside).nonzero().flatten()
    k8[out_rows[out_rows < k8.shape[0]]] = fc.NAN_CODE
    v8t[out_rows >> 6, :, :, fc.SLOT_MAP.to(k8.device)[out_rows & 63]] = fc.NAN_CODE


def _shadow(ops, launch, poison=False):
    k8, v8t = ops.attn_fp8_shadow(launch.cache_rows, launch.kc.shape[1], DEV)
    ops.attn_quantize_kv(launch.kc, launch.vc, k8, v8t, 0, None, launch.k_scale, launch.v_scale)
    if poison:
        _poison(launch, k8, v8t)
    return k8, v8t


def _fwd(ops, launch, k8, v8t, S, **kw):
    return ops.attn_fwd_fp8(launch.q, k8, v8t, launch.seg0, launch.seg1, k_scale=launch.k_scale, v_scale=launch.v_scale,
                            causal_block=launch.causal_block, q_offset=launch.q_offset, kv_splits=S, **kw)


def _check(ops, spec, splits, family):
    """The reference once per spec; every S plain and poisoned; one of them launched twice."""
    launch = fc.Launch(spec.to(DEV))
    ref, E = fc.reference(launch, *launch.shadow())
    for poison in (False, True):
        k8, v8t = _shadow(ops, launch, poison)
        for S in splits:
            out = _fwd(ops, launch, k8, v8t, S)
            ok, ratio = fc.bound_ratio(out, ref, E)
            print(f"ATTN_FP8_SPLIT_RATIO family={family} case={launch.name} S={S} poison={int(poison)} ratio={ratio:.3f}")
            assert bool(torch.isfinite(out).all()), f"{launch.name}: S {S}: non-finite output (poison={poison})"
            assert ok, f"{launch.name}: S {S}, poison={poison}, err / (E + 2^-8 |ref| + 5e-7) = {ratio:.3f} (accepted: 2)"
        assert torch.equal(out, _fwd(ops, launch, k8, v8t, splits[-1])), f"{launch.name}: two launches differ"


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("seg0,seg1", sc.WINDOWS, ids=lambda v: f"{v[0]}+{v[1]}")
def test_windows(ops, seg0, seg1, family):
    ran = 0
    for S in sc.SPLITS:                      # the inputs depend on S: the targets sit at the ends of its ranges
        spec = sc.spec_window(family, seg0, seg1, S)
        if spec is not None:
            _check(ops, spec, (S,), family)
            ran += 1
    if not ran:
        assert family in ("staircase", "tie3") and seg0[1] + seg1[1] < 193, "only the 131-key window may be too short for a family"


@pytest.mark.parametrize("Lq,Lkv,cb,off", sc.CAUSAL, ids=lambda v: str(v))
def test_block_causal(ops, Lq, Lkv, cb, off):
    _check(ops, ac.spec_causal(Lq, Lkv, cb, off, BF16), sc.SPLITS, "causal")


@pytest.mark.parametrize("H", sc.HEAD_MAPS)
def test_head_maps(ops, H):
    _check(ops, sc.spec_window("one_hot", (3, 1100), (0, 0), 3, H), (3,), f"heads{H}")


def test_one_range_is_the_unsplit_kernel(ops):
    """kv_splits = 1 through the new entry point, and a kv_splits the clamp brings down to 1 (a window inside one storage tile)."""
    for spec in (ac.spec_two_ranges((600, 500), (2, 300), dtype=BF16), ac.spec_causal(520, 1100, 96, 37, BF16)):
        launch = fc.Launch(spec.to(DEV))
        k8, v8t = _shadow(ops, launch)
        ws = torch.empty(16, dtype=torch.float32, device=DEV)                  # (a workspace routes ops.attn_fwd_fp8 to the new entry)
        assert torch.equal(_fwd(ops, launch, k8, v8t, 1, workspace=ws), _fwd(ops, launch, k8, v8t, 1))
    launch = fc.Launch(ac.spec_every_key(300, 40, BF16).to(DEV))               # rows 5..44: one tile
    k8, v8t = _shadow(ops, launch)
    assert sc.window_tiles(launch.seg0, launch.seg1) == 1
    assert torch.equal(_fwd(ops, launch, k8, v8t, 16, workspace=torch.empty(16, dtype=torch.float32, device=DEV)), _fwd(ops, launch, k8, v8t, 1))


def test_gaussian_bound_and_rounding_quality(ops):
    """The rule of tests/test_attn_fp8_gpu.py: rel-L2 against the reference at most 1.25 x that of the (split) emulation."""
    spec = ac.spec_gaussian()
    _check(ops, spec, sc.SPLITS, "gaussian")
    launch = fc.Launch(spec.to(DEV))
    k8, v8t = launch.shadow()
    ref, _ = fc.reference(launch, k8, v8t)
    cpu = fc.Launch(spec)
    for S in sc.SPLITS:
        r_kernel = fc.rel_l2(_fwd(ops, launch, *_shadow(ops, launch), S), ref)
        r_emul = fc.rel_l2(sc.emulate_split(cpu, *cpu.shadow(), S).to(DEV), ref)
        print(f"ATTN_FP8_SPLIT_REL_L2 gaussian S={S} kernel={r_kernel:.4e} emulation={r_emul:.4e}")
        assert r_kernel <= 1.25 * r_emul


def test_refusals_launch_nothing(ops):
    from realtime_video_amd import _lib
    lib = _lib.load()
    H, rows, Lq = 2, 300, 40
    g = torch.Generator().manual_seed(1)
    kc, vc = ((torch.randn(rows, H, 128, generator=g) * 3).to(BF16).to(DEV) for _ in range(2))
    k8, v8t = ops.attn_fp8_shadow(rows, H, DEV)
    ops.attn_quantize_kv(kc, vc, k8, v8t)
    q = torch.randn(Lq, H, 128, generator=g).to(BF16).to(DEV)
    out = torch.full((Lq, H, 128), 7.0, dtype=BF16, device=DEV)
    need = lib.rtv_attn_split_workspace_bytes(1, Lq, H, 4)
    ws = torch.full((need // 4 + 4,), 9.0, dtype=torch.float32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rs = H * 128
    good = dict(q=q.data_ptr(), k8=k8.data_ptr(), v8t=v8t.data_ptr(), o=out.data_ptr(), Lq=Lq, H=H, cache_rows=rows, row0=3, n0=150,
                row1=200, n1=90, q_rs=rs, o_rs=rs, scale=0.088, k_scale=1.0, v_scale=1.0, causal_block=0, q_offset=0, kv_splits=4,
                ws=ws.data_ptr(), ws_bytes=need)
    order = list(good)

    def fwd(**kw):
        a = dict(good, **kw)
        return lib.rtv_attn_fwd_fp8_split(*[a[n] for n in order], stream)

    nan = float("nan")
    bad = [dict(q=0), dict(k8=0), dict(v8t=0), dict(o=0), dict(q=q.data_ptr() + 2), dict(k8=k8.data_ptr() + 8), dict(o=out.data_ptr() + 2),
           dict(Lq=0), dict(H=0), dict(n0=0), dict(n1=-1), dict(row0=-1), dict(row0=200, n0=101), dict(row1=-1), dict(row1=250, n1=51),
           dict(causal_block=8), dict(scale=0.0), dict(scale=nan), dict(k_scale=0.0), dict(v_scale=-1.0), dict(q_rs=rs - 8), dict(o_rs=rs + 4),
           dict(kv_splits=0), dict(kv_splits=-2), dict(kv_splits=17), dict(ws=0), dict(ws=ws.data_ptr() + 4), dict(ws_bytes=need - 4),
           dict(ws_bytes=0), dict(kv_splits=5)]                                  # (5 ranges in a workspace sized for 4)
    for kw in bad:
        assert fwd(**kw) != 0, kw
        assert lib.rtv_last_error().decode().startswith("attn_fwd_fp8_split:"), kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 9.0).all()), "a refused call launched"
    # the workspace counts only while more than one range is left: kv_splits = 1, and 16 clamped to a one-tile window
    assert fwd(kv_splits=1, ws=0, ws_bytes=0) == 0 and fwd(kv_splits=16, row0=3, n0=40, n1=0, ws=0, ws_bytes=0) == 0
    assert fwd() == 0 and fwd(causal_block=8, n1=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())
