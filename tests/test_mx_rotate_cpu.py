"""CPU-only tests of the block Hadamard rotation of the MXFP4 / MXFP6 quantisers (include/rtv_hip_mx_rotate.h;
enable_mxfp4(rotate=True) / enable_mxfp6(rotate=True)): the restatement tests/mx_rotate_oracle.py against exact arithmetic, the
mutants it must tell apart on the inputs of the GPU tests, what the rotation is for (the error on operands with outlier channels),
the binding, the refusals that need no device, and the code objects."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import mx_rotate_oracle as ro
import mxfp4_oracle
import mxfp6_oracle
from mx_oracle import BLOCK, mx_dequantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtime_video_amd", "csrc")
BF = torch.bfloat16
FORMATS = {"mxfp4": mxfp4_oracle, "mxfp6": mxfp6_oracle}
SHAPES = [(5, 256), (5, 2048), (3, 2080), (2, 13824)]                  # the quantiser shapes of tests/test_mx_rotate_gpu.py


# ----------------------------------------------------------------------------------------- the rotation itself
def _narrow(rows, K, q_lo, q_hi, seed):
    """bf16 [rows, K] of magnitudes m * 2^q, m in [1, 2) with 8 significant bits, q_lo <= q <= q_hi, random signs"""
    g = torch.Generator().manual_seed(seed)
    m = 1 + torch.randint(0, 128, (rows, K), generator=g).double() / 128
    q = torch.randint(q_lo, q_hi + 1, (rows, K), generator=g)
    sign = torch.where(torch.rand(rows, K, generator=g) < 0.5, -1.0, 1.0).double()
    return (sign * torch.ldexp(m, q)).to(BF)


def test_rotated_product_is_the_plain_product_exactly():
    """rotate32(x, 3) . rotate32(w, 2)^T == x . w^T in float64, bit for bit, on bf16 operands whose blocks span 9 binades (fewer than
    16; with 8-bit significands and 5 bits of growth over the five stages every butterfly result then fits fp32's 24 bits: 9 + 8 + 5
    = 22).  Every partial sum of both products is a multiple of 2^-35 below 2^16, so float64 evaluates both without rounding."""
    x = _narrow(64, 512, -6, 2, seed=1)
    w = _narrow(96, 512, -10, -2, seed=2)
    xr, wr = ro.rotate32(x, ro.SHIFT_ACT), ro.rotate32(w, ro.SHIFT_WEIGHT)
    assert xr.dtype == torch.float32 and xr.shape == x.shape
    plain = x.double() @ w.double().t()
    assert torch.equal(xr.double() @ wr.double().t(), plain)
    assert float(plain.abs().max()) > 0
    # the rotation is the Sylvester matrix: entry (k, n) = (-1)^popcount(k & n), checked on unit vectors
    eye = torch.eye(BLOCK).to(BF)
    H = torch.tensor([[(-1.0) ** bin(k & n).count("1") for n in range(BLOCK)] for k in range(BLOCK)])
    assert torch.equal(ro.rotate32(eye, 0), H)
    assert torch.equal(H @ H.t(), 32 * torch.eye(BLOCK))


def test_stage_order_matters_on_wide_blocks_only():
    """On a block that spans 20 binades fp32 rounds inside the butterflies, so running the stages in the opposite order gives other
    values - which is why the order is part of the ABI; on narrow blocks any order gives the same."""
    def reversed_stages(x):
        v = x.float().reshape(-1, BLOCK).clone()
        for b in reversed(range(5)):
            lo = torch.tensor([k for k in range(BLOCK) if not (k >> b) & 1])
            hi = lo | (1 << b)
            s, d = v[:, lo] + v[:, hi], v[:, lo] - v[:, hi]
            v = torch.empty_like(v)
            v[:, lo], v[:, hi] = s, d
        return v.reshape(x.shape)

    narrow = _narrow(8, 256, -6, 2, seed=3)
    assert torch.equal(reversed_stages(narrow), ro.rotate32(narrow, 0))
    wide = ro.outlier_rows(mxfp4_oracle, 5, 256)
    assert not torch.equal(reversed_stages(wide), ro.rotate32(wide, 0))


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_outlier_rows_hold_what_they_promise(fmt):
    mx = FORMATS[fmt]
    for M, d in SHAPES[:3]:
        x = ro.outlier_rows(mx, M, d).double()
        nz = x[x != 0].abs()
        assert float(nz.min()) >= 2.0 ** -60 and float(nz.max()) <= 2.0 ** 60
        blocks = x.reshape(-1, BLOCK)
        count = (blocks != 0).sum(dim=1)
        assert int((count == 0).sum()) >= 2 and int((count == 1).sum()) >= 1            # all-zero blocks, single-value blocks
        top = blocks.abs().amax(dim=1)
        low = torch.where(blocks != 0, blocks.abs(), top.unsqueeze(1)).amin(dim=1)
        assert int((top >= low * 2.0 ** 20).sum()) >= 1                                  # a block that spans 20 binades
        r = ro.rotate32(x.to(BF), ro.SHIFT_ACT).double()
        assert bool(torch.isfinite(r).all()) and float(r[r != 0].abs().min()) >= 2.0 ** -120   # no fp32 subnormal anywhere


def _stored(mx, values, e):
    codes = mx.nibbles(values) if mx is mxfp4_oracle else mx.sextets(values)
    return codes, mx.pack_scales(e)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("mutant", ro.MUTANTS)
def test_every_mutant_shows_on_the_inputs_of_the_gpu_tests(fmt, mutant):
    """The wrong index mapping, the shift off by one and the swapped stage-3 outputs each change codes or scale bytes on
    outlier_rows, at every quantiser shape and both shifts the GPU test runs."""
    mx = FORMATS[fmt]
    for M, d in SHAPES:
        x = ro.outlier_rows(mx, M, d)
        for shift in (ro.SHIFT_WEIGHT, ro.SHIFT_ACT):
            good = _stored(mx, *ro.mx_quantize_rot(mx, x, shift))
            bad = _stored(mx, *ro.mx_quantize_rot(mx, x, shift, mutant=mutant))
            assert not (torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1])), (M, d, shift)
    # and the rotation is really on: the unrotated quantiser gives other codes
    x = ro.outlier_rows(mx, 5, 256)
    assert not torch.equal(_stored(mx, *mx.mx_quantize(x))[0], _stored(mx, *ro.mx_quantize_rot(mx, x, 0))[0])


def test_a_single_value_spreads_to_32_equal_magnitudes():
    x = torch.zeros(32, 32, dtype=BF)
    x[torch.arange(32), torch.arange(32)] = 1.5
    r = ro.rotate32(x, 0)
    assert bool((r.abs() == 1.5).all())
    for mx in FORMATS.values():
        v, e = ro.mx_quantize_rot(mx, x, 0)
        assert bool((v.abs() == 6.0).all()) and bool((e == -2).all())


# ----------------------------------------------------------------------------------------- what it is for
def _product_error(mx, x, w, rotate):
    if rotate:
        xq = mx_dequantize(*ro.mx_quantize_rot(mx, x, ro.SHIFT_ACT))
        wq = mx_dequantize(*ro.mx_quantize_rot(mx, w, ro.SHIFT_WEIGHT))
    else:
        xq, wq = mx_dequantize(*mx.mx_quantize(x)), mx_dequantize(*mx.mx_quantize(w))
    want = x.double() @ w.double().t()
    return float(((xq @ wq.t()) - want).norm() / want.norm())


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_rotation_recovers_outlier_channels_and_is_neutral_on_gaussian_operands(fmt):
    """rel-L2 of the dequantised product against x w^T in float64, M, N, K = 64, 96, 512, on the restatement alone.  Activations with
    every 32nd column times 32: rotated <= 0.85 x unrotated.  Gaussian activations: rotated <= 1.05 x unrotated.
    Measured with these seeds (profiles/r18_mx_rotate_parity.txt): MXFP4 0.758 and 0.967, MXFP6 0.717 and 0.988."""
    mx = FORMATS[fmt]
    x, w = ro.product_operands()
    plain, rot = _product_error(mx, x, w, False), _product_error(mx, x, w, True)
    xo = ro.outlier_columns(x)
    plain_o, rot_o = _product_error(mx, xo, w, False), _product_error(mx, xo, w, True)
    print(f"{fmt} rel-L2 of the product, restatement: gaussian {plain:.4f} -> rotated {rot:.4f} (ratio {rot / plain:.3f}); "
          f"every 32nd column x32 {plain_o:.4f} -> rotated {rot_o:.4f} (ratio {rot_o / plain_o:.3f})")
    assert rot_o <= 0.85 * plain_o
    assert rot <= 1.05 * plain


# ----------------------------------------------------------------------------------------- binding and workspace
def test_shift_constants_equal_their_python_twins():
    from realtime_video_amd import _lib, ops
    text = open(os.path.join(ROOT, "include", "rtv_hip_mx_rotate.h")).read()
    act = int(re.search(r"^#define RTV_MX_ROT_ACT_SHIFT (\d+)$", text, flags=re.M).group(1))
    weight = int(re.search(r"^#define RTV_MX_ROT_WEIGHT_SHIFT (\d+)$", text, flags=re.M).group(1))
    assert (act, weight) == (ro.SHIFT_ACT, ro.SHIFT_WEIGHT) == (_lib.MX_ROT_ACT_SHIFT, _lib.MX_ROT_WEIGHT_SHIFT) == (3, 2)
    assert (ops.MX_ROT_ACT_SHIFT, ops.MX_ROT_WEIGHT_SHIFT) == (act, weight)
    assert act + weight == 5 and _lib.MX_ROT_MAX_SHIFT == 5            # 2^-3 * 2^-2 = 1 / 32


def test_binding_has_the_rotated_entry_points():
    from realtime_video_amd import _lib
    P = _lib.MX_ROTATE_PROTOTYPES
    assert set(P) == {"rtv_quantize_mxfp4_rot", "rtv_quantize_mxfp6_rot", "rtv_layernorm_modulate_mxfp4_rot",
                      "rtv_layernorm_modulate_mxfp6_rot"}
    for f, plain in (("mxfp4", _lib.MXFP4_PROTOTYPES), ("mxfp6", _lib.MXFP6_PROTOTYPES)):
        restype, args = plain[f"rtv_quantize_{f}"]
        assert P[f"rtv_quantize_{f}_rot"] == (restype, args[:-1] + [ctypes.c_int, args[-1]])      # + int shift in front of the stream
        assert P[f"rtv_layernorm_modulate_{f}_rot"] == plain[f"rtv_layernorm_modulate_{f}"]
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert _lib.ABI_VERSION == 105                                     # no layout and no signature of rtv_hip.h changed


def test_workspace_of_the_rotated_modes_is_that_of_the_unrotated_ones():
    from realtime_video_amd import _lib
    lib = _lib.load()
    Cfg = _lib.STRUCTS["rtv_dit_config"]
    sizes = {}
    for mode in (3, 4, 5, 6):
        cfg = Cfg(dim=1536, ffn_dim=8960, num_heads=12, num_layers=2, freq_dim=256, text_dim=4096, text_len=512, in_dim=16,
                  out_dim=16, eps=1e-6, use_fp8=mode, max_attn_kv_splits=0)
        sizes[mode] = lib.rtv_dit_workspace_bytes(ctypes.byref(cfg), 3, 30, 52)
    assert sizes[5] == sizes[3] and sizes[6] == sizes[4] and sizes[3] > 0


# ----------------------------------------------------------------------------------------- refusals, before any launch
def _cpu_model(**kw):
    from realtime_video_amd.causal_model import CausalWanModel
    args = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=256, device="cpu")
    args.update(kw)
    return CausalWanModel(**args)


def _enable(model, name, rotate):
    return getattr(model, "enable_" + name)(rotate=rotate)


@pytest.mark.parametrize("name,mode", [("mxfp4", 5), ("mxfp6", 6)])
def test_rotated_modes_are_exclusive_with_every_other_mode_in_both_orders(name, mode):
    other = "mxfp6" if name == "mxfp4" else "mxfp4"
    for left in (1, 2, 3, 4, 5, 6):
        if left == mode:
            continue
        model = _cpu_model()
        model._cfg.use_fp8 = left                                      # what the other enable_* calls leave behind
        with pytest.raises(RuntimeError, match="reload the weights first"):
            _enable(model, name, True)
    model = _cpu_model()
    model._cfg.use_fp8 = mode
    for call in (lambda: model.enable_fp8(), lambda: model.enable_fp8("row"), lambda: _enable(model, other, False),
                 lambda: _enable(model, other, True), lambda: _enable(model, name, False)):
        with pytest.raises(RuntimeError, match="reload the weights first"):
            call()
    with pytest.raises(RuntimeError, match=f"enable_{name} after .*enable_{name}\\(rotate=True\\)"):     # the other value of rotate, named
        getattr(model, "enable_" + name)()
    assert _enable(model, name, True) is model and model._cfg.use_fp8 == mode        # a second call is a no-op
    model = _cpu_model()
    model._cfg.use_fp8 = mode - 2                                      # unrotated first, rotated afterwards
    with pytest.raises(RuntimeError, match=f"enable_{name} after .*enable_{name}\\(rotate=False\\)"):
        _enable(model, name, True)


@pytest.mark.parametrize("name,multiple", [("mxfp4", 256), ("mxfp6", 128)])
def test_rotated_modes_keep_the_width_and_context_parallel_refusals(name, multiple):
    from realtime_video_amd.parallel import SimulatedContextParallel
    with pytest.raises(ValueError, match=f"multiple of {multiple}"):
        _enable(_cpu_model(text_dim=multiple // 2 * 3), name, True)
    model = _cpu_model()
    model.context_parallel = SimulatedContextParallel(2, "rows")
    with pytest.raises(RuntimeError, match="context parallelism"):
        _enable(model, name, True)
    with pytest.raises(RuntimeError, match="load weights before"):
        _enable(_cpu_model(), name, True)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_launch_checks_come_before_any_launch(fmt):
    """The argument checks of the unrotated entries, with their error strings, plus the shift's: the pointers are never read."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)
    quantize = getattr(lib, f"rtv_quantize_{fmt}_rot")
    layernorm = getattr(lib, f"rtv_layernorm_modulate_{fmt}_rot")

    def q(x=p, ld=64, M=1, d=64, codes=p, ld_codes=48, ld_scales=8, shift=3):
        st = quantize(x, ld, M, d, codes, ld_codes, p, ld_scales, shift, None)
        return st, lib.rtv_last_error().decode()

    for shift in (-1, 6, 32):
        st, msg = q(shift=shift)
        assert st != 0 and f"quantize_{fmt}: shift must be in 0 .. 5" in msg
    for kw, what in ((dict(d=48, ld=48), "d must be a multiple of 32"), (dict(ld=60), "ld a multiple of 8"),
                     (dict(x=ctypes.c_void_p(base + 8)), "x must be 16-byte aligned"), (dict(codes=ctypes.c_void_p(base + 2)), "codes 4-byte aligned"),
                     (dict(ld_codes=16), "ld_codes must be a multiple of 4"), (dict(ld_scales=1), "ld_scales >="),
                     (dict(x=None), "null pointer"), (dict(M=0), "empty tensor"), (dict(d=14368, ld=14368), "d must be <= 14336")):
        st, msg = q(**kw)
        assert st != 0 and msg.startswith(f"quantize_{fmt}: ") and what in msg, (kw, msg)

    def ln(x=p, d=64, ld_codes=48, shift=None, scale=None, weight=None, bias=None):
        st = layernorm(x, p, ld_codes, p, 8, 1, d, 1e-6, shift, scale, 0, 0, 0, weight, bias, None)
        return st, lib.rtv_last_error().decode()

    for kw, what in ((dict(d=48), "d must be a multiple of 32 and <= 8192"), (dict(d=8224), "d must be a multiple of 32 and <= 8192"),
                     (dict(x=ctypes.c_void_p(base + 8)), "x must be 16-byte aligned"), (dict(ld_codes=16), "ld_codes must be a multiple of 4"),
                     (dict(shift=p), "shift and scale go together"), (dict(weight=p), "weight and bias go together"),
                     (dict(shift=p, scale=p, weight=p, bias=p), "affine and modulation are exclusive")):
        st, msg = ln(**kw)
        assert st != 0 and msg.startswith(f"layernorm_modulate_{fmt}: ") and what in msg, (kw, msg)


# ----------------------------------------------------------------------------------------- code objects
def test_rotated_kernels_have_no_scratch_and_exchange_inside_the_quad(tmp_path):
    """Eight kernels (three row quantisers and the LayerNorm-fused one, per format): no scratch, no spills, at most 64 VGPRs (the
    occupancy of the unrotated kernels), and the two exchange stages are DPP quad_perm moves.  What stays on ds_bpermute_b32 is what
    the unrotated kernels have per chunk - the two exchanges of the block maximum and MXFP6's one of the packer - so the rotation
    added none (it would add 16 per chunk): MAXC chunks x 3 at the most, plus the wave reductions of the LayerNorm."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), f"{hipcc} is missing: the library cannot be built without it, so the audit fails, it does not skip"
    out = tmp_path / "mx_rotate.s"
    r = subprocess.run([hipcc, "--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-O3", "-std=c++17", "-fPIC", "-S",
                        "--cuda-device-only", os.path.join(CSRC, "mx_rotate.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    asm = out.read_text()
    meta = {}
    for entry in re.split(r"\n  - \.agpr_count:", asm.split("amdhsa.kernels:")[1])[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", entry)}
    assert len(meta) == 8 and all("mx_rot_kernel" in n for n in meta), list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)
        body = re.split(rf"\n{re.escape(name)}:[^\n]*\n", asm)[1].split(".Lfunc_end")[0]
        chunks = 4 if "layernorm" in name else int(re.search(r"ELi(\d)ELb", name).group(1))
        assert len(re.findall(r"quad_perm:\[1,0,3,2\]", body)) >= 8 and len(re.findall(r"quad_perm:\[2,3,0,1\]", body)) >= 8, name
        reductions = 12 if "layernorm" in name else 0                   # LayerNorm's two row sums: six xor steps of a wave each
        assert len(re.findall(r"ds_bpermute_b32", body)) <= 3 * chunks + reductions, (name, len(re.findall(r"ds_bpermute_b32", body)))
