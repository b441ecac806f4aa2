"""CPU-only tests of the MXFP4 mode (enable_mxfp4(), include/rtv_hip_mxfp4.h): the inputs the GPU tests feed the quantiser are strong
enough to tell the format from three near misses, the exact GEMM case is exact, the binding and the workspace, the refusals that
come before any launch, and the code objects of the new kernels."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import mxfp4_oracle as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtime_video_amd", "csrc")
QUANT_SHAPES = [(5, 256), (5, 2048), (3, 2080), (5, 5120), (2, 13824)]      # tests/test_mxfp4_gpu.py runs exactly these
# (the last one is the smallest shape that takes the split-K hand-off: tests/test_mxfp4_gpu.py says why)
EXACT_SHAPES = [(257, 264, 256), (300, 520, 512), (257, 264, 768), (513, 1536, 1024), (257, 264, 2048)]


# ----------------------------------------------------------------------------------------- the restatement itself
def test_restatement_on_hand_computed_blocks():
    x = torch.zeros(4, 32)
    x[0, :8] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 4.0])            # amax 4 -> e = 0: the seven ties
    x[1, :4] = torch.tensor([-7.5, 6.5, 0.26, -0.25]) * 2.0 ** 10                      # amax 7.5 * 2^10 -> e = 10, saturation
    x[3, :3] = torch.tensor([3.0, -1.0, 0.374]) * 2.0 ** -20                            # amax 3 * 2^-20 -> e = -21: values x 2
    v, e = mx.mx_quantize(x.to(torch.bfloat16))
    assert e.reshape(-1).tolist() == [0, 10, -127, -21]
    assert v[0, :8].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 4.0]                # ties go to the even code
    assert v[1, :4].tolist() == [-6.0, 6.0, 0.5, -0.0]
    assert v[2].abs().max() == 0
    assert v[3, :3].tolist() == [6.0, -2.0, 0.5]                                        # 0.748 -> 0.5 (below the tie at 0.75)
    assert mx.pack_scales(e.reshape(4, 1))[:, 0].tolist() == [127, 137, 0, 106]
    n = mx.nibbles(v)
    assert n[0, :8].tolist() == [0, 2, 2, 4, 4, 6, 6, 6] and n[1, :4].tolist() == [15, 7, 1, 0]
    p = mx.pack_codes(v)
    assert p[0, :4].tolist() == [0x20, 0x42, 0x64, 0x66] and torch.equal(mx.unpack_nibbles(p), n)


def test_scale_order_puts_a_lanes_four_blocks_in_one_aligned_dword():
    """In the 64-deep step st of a 256-element K-tile lanes with g = lane >> 5 own block 2 st + g: byte 4 g + st of the tile."""
    for kt in range(3):
        for g in range(2):
            for st in range(4):
                assert mx.scale_pos(8 * kt + 2 * st + g) == 8 * kt + 4 * g + st
    assert sorted(mx.scale_pos(b) for b in range(64)) == list(range(64))
    assert [mx.scale_bytes(k) for k in (32, 256, 2080, 5120)] == [8, 8, 72, 160]
    text = open(os.path.join(ROOT, "include", "rtv_hip_mxfp4.h")).read()
    assert "#define RTV_MXFP4_SCALE_POS(b) (((b) & ~7) | (((b) & 1) << 2) | (((b) & 7) >> 1))" in text
    assert "#define RTV_MXFP4_SCALE_BYTES(K) ((((K) / RTV_MXFP4_BLOCK) + 7) & ~7)" in text


# ----------------------------------------------------------------------------------------- tie and saturation coverage
@pytest.mark.parametrize("M,d", QUANT_SHAPES)
def test_structured_rows_cover_ties_saturation_zero_blocks_and_the_exponent_range(M, d):
    x = mx.structured_rows(M, d)
    v, e = mx.mx_quantize(x)
    xb = x.double().reshape(M, d // 32, 32)
    t = torch.ldexp(xb, -e.unsqueeze(-1)).abs()                      # in units of the block scale
    ties = sum(int((t == tie).sum()) for tie in mx.TIES)
    assert ties >= 64 and all(int((t == tie).sum()) > 0 for tie in mx.TIES)
    amax = t.amax(dim=-1)
    assert int((amax == 4.0).sum()) > 0                               # a maximum that is an exact power of two
    assert int(((amax > 6.0) & (amax < 8.0)).sum()) > 0               # saturating blocks
    zero = xb.abs().amax(dim=-1) == 0
    assert int(zero.sum()) > 0 and bool((e[zero] == -127).all())      # an all-zero block: scale byte 0
    assert bool((x.float() < 0).any())
    live = e[~zero]
    assert int(live.min()) == -100 and int(live.max()) == 100
    assert bool(torch.isfinite(x.float()).all())

    def differs(**mutant):
        vm, em = mx.mx_quantize(x, **mutant)
        return not (torch.equal(mx.nibbles(vm), mx.nibbles(v)) and torch.equal(em, e))

    assert differs(tie_order=mx._LARGE_FIRST), "round-half-away is not told apart: the inputs are too weak"
    assert differs(ceil_scale=True), "a ceiling scale is not told apart: the inputs are too weak"
    assert differs(saturate=False), "a conversion without saturation is not told apart: the inputs are too weak"


# ----------------------------------------------------------------------------------------- exact GEMM case
@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_exact_gemm_case_is_exact_in_fp32(M, N, K):
    """Codes are arbitrary and both operands' block exponents lie in {-1, 0, 1}: every term is a multiple of 2^-4 of magnitude
    <= 144, so with sum |terms| < 2^19 every partial sum, in any order, is a multiple of 2^-4 below 2^19 = 23 bits: exact in fp32."""
    c = mx.exact_case(M, N, K)
    for e in (c["ea"], c["ew"]):
        assert int(e.min()) == -1 and int(e.max()) == 1
    assert not torch.equal(c["a"][:8], c["w"][:8]) and not torch.equal(c["ea"][:8], c["ew"][:8])      # no symmetry between the operands
    da, dw = mx.mx_dequantize(c["a"], c["ea"]), mx.mx_dequantize(c["w"], c["ew"])
    assert float((da.abs().amax()) * (dw.abs().amax())) <= 144.0
    assert bool((torch.ldexp(da, torch.tensor(2)) == torch.ldexp(da, torch.tensor(2)).round()).all())      # multiples of 2^-2
    assert bool((torch.ldexp(dw, torch.tensor(2)) == torch.ldexp(dw, torch.tensor(2)).round()).all())
    total, mag = mx.product_fp64(c["a"], c["ea"], c["w"], c["ew"])
    assert float(mag.max()) <= 2.0 ** 19
    assert torch.equal(total.float().double(), total)                 # the fp64 sum itself is an fp32 number
    # distinct scales per row and per block: no block column and no row of exponents is constant (K = 256 has 8 blocks a row)
    for e in (c["ea"], c["ew"]):
        assert bool((e.min(dim=0).values != e.max(dim=0).values).all())
        assert int((e.min(dim=1).values != e.max(dim=1).values).sum()) >= e.shape[0] * 9 // 10


# ----------------------------------------------------------------------------------------- binding and workspace
def test_binding_has_the_mxfp4_entry_points():
    from realtime_video_amd import _lib
    P = _lib.MXFP4_PROTOTYPES
    assert set(P) == {"rtv_quantize_mxfp4", "rtv_layernorm_modulate_mxfp4", "rtv_gemm_mxfp4"}
    q = P["rtv_quantize_mxfp4"][1]
    assert [q[i] for i in (1, 5, 7)] == [ctypes.c_int64] * 3 and len(q) == 9
    assert P["rtv_gemm_mxfp4"][1][4:6] == [ctypes.c_void_p, ctypes.c_void_p] and len(P["rtv_gemm_mxfp4"][1]) == 20
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_struct_fields_are_unchanged():
    from realtime_video_amd import _lib
    assert [n for n, _ in _lib.STRUCTS["rtv_dit_weights"]._fields_] == [
        "patch_w", "patch_b", "text0_w", "text0_b", "text2_w", "text2_b", "time0_w", "time0_b", "time2_w", "time2_b", "tproj_w",
        "tproj_b", "head_w", "head_b", "modulation", "head_modulation", "rope_cs", "layers", "fp8_scales", "fp8_row_scales"]
    assert [n for n, _ in _lib.STRUCTS["rtv_dit_step"]._fields_] == [
        "x", "t", "context", "out", "F", "gh", "gw", "kv_k", "kv_v", "kv_row_stride", "ca_k", "ca_v", "compute_cross_kv",
        "cache_row0", "kv_lo", "kv_hi", "start_frame", "causal_block", "gemm_tile_cfg", "row_begin", "row_count", "ring_lo",
        "ring_size", "ring_shift", "text_rows", "kv_only", "attn_kv_splits", "ca_vo_ld"]
    assert _lib.ABI_VERSION == 105


# rtv_dit_workspace_bytes of commit ddf8a9a (the parent of the MXFP4 mode) on the shape of tests/test_fp8_rows_cpu.py.  Literals on
# purpose - not to be regenerated from the library.
PARENT_WORKSPACE = {0: 190635008, 1: 232567808, 2: 232586752}


def test_workspace_of_the_other_modes_is_the_parents_and_mode_3_has_one():
    from realtime_video_amd import _lib
    lib = _lib.load()
    Cfg = _lib.STRUCTS["rtv_dit_config"]
    sizes = {}
    for mode in (0, 1, 2, 3):
        cfg = Cfg(dim=1536, ffn_dim=8960, num_heads=12, num_layers=2, freq_dim=256, text_dim=4096, text_len=512, in_dim=16,
                  out_dim=16, eps=1e-6, use_fp8=mode, max_attn_kv_splits=0)
        sizes[mode] = lib.rtv_dit_workspace_bytes(ctypes.byref(cfg), 3, 30, 52)
    assert {m: sizes[m] for m in (0, 1, 2)} == PARENT_WORKSPACE
    # codes (rows * K / 2) and block scales (rows * K / 32) of the widest activation fit the fp8 buffer (rows * K)
    assert sizes[3] > sizes[0] and sizes[3] - sizes[0] >= max(3 * 30 * 52, 512) * 8960 * 17 // 32


# ----------------------------------------------------------------------------------------- refusals, before any launch
def _cpu_model(**kw):
    from realtime_video_amd.causal_model import CausalWanModel
    args = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=256, device="cpu")
    args.update(kw)
    return CausalWanModel(**args)


def test_enable_mxfp4_refuses_a_width_that_is_no_multiple_of_256():
    with pytest.raises(ValueError, match="multiple of 256"):
        _cpu_model(text_dim=128).enable_mxfp4()
    with pytest.raises(ValueError, match="multiple of 256"):
        _cpu_model(ffn_dim=640).enable_mxfp4()


def test_enable_mxfp4_refuses_a_model_that_runs_fp8():
    for mode in (1, 2):
        model = _cpu_model()
        model._cfg.use_fp8 = mode                                    # what enable_fp8() / enable_fp8("row") leave behind
        with pytest.raises(RuntimeError, match="reload the weights first"):
            model.enable_mxfp4()
    model = _cpu_model()
    model._cfg.use_fp8 = 3                                           # and the other direction
    with pytest.raises(RuntimeError, match="reload the weights first"):
        model.enable_fp8()
    with pytest.raises(RuntimeError, match="reload the weights first"):
        model.enable_fp8("row")


def test_enable_mxfp4_refuses_context_parallelism():
    from realtime_video_amd.parallel import SimulatedContextParallel
    model = _cpu_model()
    model.context_parallel = SimulatedContextParallel(2, "rows")
    with pytest.raises(RuntimeError, match="context parallelism"):
        model.enable_mxfp4()


def test_gemm_refuses_a_k_that_is_no_multiple_of_256():
    """The argument checks come before anything touches the device: the pointers here are never read."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for K in (128, 384):
        st = lib.rtv_gemm_mxfp4(p, K // 2, p, K // 2, p, p, p, 8, 1, 8, K, None, 0, None, 0, 0, 0, None, 0, None)
        assert st != 0 and "multiple of 256" in lib.rtv_last_error().decode()
    st = lib.rtv_quantize_mxfp4(p, 48, 1, 48, p, 24, p, 8, None)
    assert st != 0 and "multiple of 32" in lib.rtv_last_error().decode()


# ----------------------------------------------------------------------------------------- code objects
def _device_asm(tmp_path, unit):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), f"{hipcc} is missing: the library cannot be built without it, so the audit fails, it does not skip"
    out = tmp_path / (unit + ".s")
    r = subprocess.run([hipcc, "--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-O3", "-std=c++17", "-fPIC", "-S",
                        "--cuda-device-only", os.path.join(CSRC, unit + ".hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out.read_text()


def _kernel_metadata(asm):
    """{kernel name: {key: int}} from the amdhsa.kernels metadata of a device assembly."""
    meta = {}
    for entry in re.split(r"\n  - \.agpr_count:", asm.split("amdhsa.kernels:")[1])[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", entry)}
    return meta


@pytest.mark.parametrize("unit,kernels", [("gemm_mxfp4", 1), ("mxfp4", 4)])
def test_new_kernels_have_no_scratch_and_no_spills(tmp_path, unit, kernels):
    asm = _device_asm(tmp_path, unit)
    meta = _kernel_metadata(asm)
    assert len(meta) == kernels and all("mxfp4" in n for n in meta), list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    if unit == "gemm_mxfp4":
        mfma = re.findall(r"^\s*(v_mfma\S*) .*$", asm, flags=re.M)
        lines = re.findall(r"^\s*v_mfma_scale_f32_32x32x64_f8f6f4 .*cbsz:4 blgp:4\s*$", asm, flags=re.M)
        assert len(lines) >= 32 and len(lines) == len(mfma), (len(lines), len(mfma))   # nothing but the block-scaled FP4 MFMA
