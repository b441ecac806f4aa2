"""CPU-only tests of the MXFP6 mode (enable_mxfp6(), include/rtv_hip_mxfp6.h): the inputs the GPU tests feed the quantiser are strong
enough to tell the format from three near misses, the packers and the storage macros, the exact GEMM case is exact, the binding and
the workspace, the refusals that come before any launch, and the code objects of the new kernels."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import mxfp6_oracle as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "realtime_video_amd", "csrc")
QUANT_SHAPES = [(5, 256), (5, 2048), (3, 2080), (5, 5120), (2, 13824)]      # tests/test_mxfp6_gpu.py runs exactly these
# tests/test_mxfp6_gpu.py runs exactly these and says why
EXACT_SHAPES = [(257, 264, 128), (257, 264, 256), (257, 264, 384), (300, 520, 512), (257, 264, 768), (513, 1536, 1024),
                (257, 264, 2048), (257, 264, 2176)]
SEEDS = (0, 11, 256, 1280)                                                   # every seed tests/test_mxfp6_gpu.py passes to exact_case


# ----------------------------------------------------------------------------------------- the restatement itself
def test_value_table_is_e2m3():
    assert len(mx.E2M3) == 32 and list(mx.E2M3) == sorted(mx.E2M3)
    assert mx.E2M3[:9] == (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0)
    assert mx.E2M3[15:18] == (1.875, 2.0, 2.25) and mx.E2M3[23:26] == (3.75, 4.0, 4.5) and mx.E2M3[31] == 7.5
    # every tie is the midpoint of two neighbours of the table
    mids = {(a + b) / 2 for a, b in zip(mx.E2M3, mx.E2M3[1:])}
    assert set(mx.TIES) == mids and len(mx.TIES) == 31


def test_restatement_on_hand_computed_blocks():
    x = torch.zeros(4, 32)
    x[0, :8] = torch.tensor([0.0625, 0.1875, 0.9375, 1.9375, 2.125, 3.875, 4.25, 4.0])    # amax 4.25 -> e = 0: ties of every range
    x[1, :5] = torch.tensor([-7.75, 7.625, 7.25, 0.07, -0.0625]) * 2.0 ** 10                # amax 7.75 * 2^10 -> e = 10, saturation
    x[3, :3] = torch.tensor([3.0, -1.0, 0.46]) * 2.0 ** -20                                # amax 3 * 2^-20 -> e = -21: values x 2
    v, e = mx.mx_quantize(x.to(torch.bfloat16))
    assert e.reshape(-1).tolist() == [0, 10, -127, -21]
    assert v[0, :8].tolist() == [0.0, 0.25, 1.0, 2.0, 2.0, 4.0, 4.0, 4.0]                   # ties go to the even code
    assert v[1, :5].tolist() == [-7.5, 7.5, 7.0, 0.125, -0.0]                               # 7.25 ties to code 30 (7.0), not 31
    assert v[2].abs().max() == 0
    assert v[3, :3].tolist() == [6.0, -2.0, 0.875]                                          # 0.918 -> 0.875 (below the tie at 0.9375)
    assert mx.pack_scales(e.reshape(4, 1))[:, 0].tolist() == [127, 137, 0, 106]
    s = mx.sextets(v)
    assert s[0, :8].tolist() == [0, 2, 8, 16, 16, 24, 24, 24] and s[1, :5].tolist() == [63, 31, 30, 1, 0]
    p = mx.pack_codes(v)
    # elements 0..3 of row 0 = codes 0, 2, 8, 16: bits 0 | 2 << 6 | 8 << 12 | 16 << 18 = 0x408080
    assert p[0, :3].tolist() == [0x80, 0x80, 0x40] and torch.equal(mx.unpack_codes(p), s)
    assert torch.equal(mx.code_values(mx.unpack_codes(p, canonical=False)), v)


def test_packers_round_trip_and_a_block_is_24_bytes_little_endian():
    g = torch.Generator().manual_seed(1)
    s = torch.randint(0, 64, (7, 160), generator=g).to(torch.uint8)
    p = mx.pack_sextets(s)
    assert p.shape == (7, mx.code_bytes(160)) == (7, 120)
    assert torch.equal(mx.unpack_codes(p, canonical=False), s)
    # the header's statement, bit by bit: block b is bytes [24 b, 24 b + 24), element j of the block at bits [6 j, 6 j + 6)
    for row, b, j in ((0, 0, 0), (3, 2, 5), (6, 4, 31), (2, 1, 10), (5, 3, 21)):
        blk = p[row, mx.BLOCK_BYTES * b:mx.BLOCK_BYTES * (b + 1)].tolist()
        string = sum(byte << (8 * i) for i, byte in enumerate(blk))
        assert (string >> (6 * j)) & 63 == int(s[row, 32 * b + j])
        k = 32 * b + j
        bit = mx.code_bit(k)
        row_string = sum(byte << (8 * i) for i, byte in enumerate(p[row].tolist()))
        assert (row_string >> bit) & 63 == int(s[row, k])


def test_scale_order_puts_a_lanes_two_blocks_in_one_aligned_word():
    """In the 64-deep step st of a 128-element K-tile lanes with g = lane >> 5 own block 2 st + g: byte 2 g + st of the tile."""
    for kt in range(5):
        for g in range(2):
            for st in range(2):
                assert mx.scale_pos(4 * kt + 2 * st + g) == 4 * kt + 2 * g + st
    assert sorted(mx.scale_pos(b) for b in range(64)) == list(range(64))
    assert [mx.scale_bytes(k) for k in (32, 128, 256, 2080, 5120)] == [4, 4, 8, 68, 160]
    assert [mx.code_bytes(k) for k in (32, 128, 2080)] == [24, 96, 1560]
    text = open(os.path.join(ROOT, "include", "rtv_hip_mxfp6.h")).read()
    assert "#define RTV_MXFP6_SCALE_POS(b) (((b) & ~3) | (((b) & 1) << 1) | (((b) & 3) >> 1))" in text
    assert "#define RTV_MXFP6_SCALE_BYTES(K) ((((K) / RTV_MXFP6_BLOCK) + 3) & ~3)" in text
    assert "#define RTV_MXFP6_CODE_BYTES(K) ((K) / 4 * 3)" in text
    assert "#define RTV_MXFP6_CODE_BIT(k) ((k) * 6)" in text
    assert "#define RTV_MXFP6_BLOCK_BYTES 24" in text
    from realtime_video_amd import ops
    for k in (32, 128, 256, 2080, 5120):
        assert ops.mxfp6_scale_bytes(k) == mx.scale_bytes(k) and ops.mxfp6_code_bytes(k) == mx.code_bytes(k)


# ----------------------------------------------------------------------------------------- tie and saturation coverage
@pytest.mark.parametrize("M,d", QUANT_SHAPES)
def test_structured_rows_cover_ties_saturation_zero_blocks_and_the_exponent_range(M, d):
    x = mx.structured_rows(M, d)
    v, e = mx.mx_quantize(x)
    xb = x.double().reshape(M, d // 32, 32)
    t = torch.ldexp(xb, -e.unsqueeze(-1)).abs()                      # in units of the block scale
    counts = [int((t == tie).sum()) for tie in mx.TIES]
    assert sum(counts) >= 128 and all(c > 0 for c in counts)         # every one of the 31 ties, in all four spacings
    assert bool((x.float()[(t == mx.TIES[0]).reshape(M, d)] != 0).any())
    amax = t.amax(dim=-1)
    assert int((amax == 4.0).sum()) > 0                               # a maximum that is an exact power of two
    assert int(((amax > 7.5) & (amax < 8.0)).sum()) > 0               # saturating blocks
    assert int((amax == 7.75).sum()) > 0                              # the maximum that ties with 8
    zero = xb.abs().amax(dim=-1) == 0
    assert int(zero.sum()) > 0 and bool((e[zero] == -127).all())      # an all-zero block: scale byte 0
    assert bool((x.float() < 0).any())
    live = e[~zero]
    assert int(live.min()) == -100 and int(live.max()) == 100
    assert bool(torch.isfinite(x.float()).all())
    assert torch.equal(mx.code_values(mx.sextets(v)), torch.where(v == 0, torch.zeros_like(v), v))   # every value is in the table

    def differs(**mutant):
        vm, em = mx.mx_quantize(x, **mutant)
        return not (torch.equal(mx.sextets(vm), mx.sextets(v)) and torch.equal(em, e))

    assert differs(tie_order=mx._LARGE_FIRST), "round-half-away is not told apart: the inputs are too weak"
    assert differs(ceil_scale=True), "a ceiling scale is not told apart: the inputs are too weak"
    assert differs(saturate=False), "a conversion without saturation is not told apart: the inputs are too weak"


# ----------------------------------------------------------------------------------------- exact GEMM case
@pytest.mark.parametrize("M,N,K", EXACT_SHAPES)
def test_exact_gemm_case_is_exact_in_fp32(M, N, K):
    """Codes are arbitrary and both operands' block exponents lie in {-1, 0, 1}: every term is a multiple of 2^-8 (two multiples of
    1/8 times at least 2^-2), so with sum |terms| <= 2^16 every partial sum, in any order, is a multiple of 2^-8 of at most 24 bits:
    exact in fp32.  Asserted for every seed the GPU tests use."""
    for seed in SEEDS:
        c = mx.exact_case(M, N, K, seed=seed)
        for e in (c["ea"], c["ew"]):
            assert int(e.min()) == -1 and int(e.max()) == 1
        assert not torch.equal(c["a"][:8], c["w"][:8]) and not torch.equal(c["ea"][:8], c["ew"][:8])   # no symmetry between the operands
        da, dw = mx.mx_dequantize(c["a"], c["ea"]), mx.mx_dequantize(c["w"], c["ew"])
        for dq in (da, dw):
            sc = torch.ldexp(dq, torch.tensor(4))
            assert bool((sc == sc.round()).all())                     # multiples of 2^-4
        total, mag = mx.product_fp64(c["a"], c["ea"], c["w"], c["ew"])
        assert float(mag.max()) <= 2.0 ** 16, (seed, float(mag.max()))
        assert torch.equal(total.float().double(), total)             # the fp64 sum itself is an fp32 number
        if seed == 0:
            assert len(set(mx.sextets(c["a"]).reshape(-1).tolist())) >= 62        # all 32 magnitudes, both signs (-0 reads as 0)
            # distinct scales per row and per block: no block column of exponents is constant, and (from two blocks a row on) hardly
            # any row
            for e in (c["ea"], c["ew"]):
                assert bool((e.min(dim=0).values != e.max(dim=0).values).all())
                if K >= 256:
                    assert int((e.min(dim=1).values != e.max(dim=1).values).sum()) >= e.shape[0] * 9 // 10


# ----------------------------------------------------------------------------------------- binding and workspace
def test_binding_has_the_mxfp6_entry_points():
    from realtime_video_amd import _lib
    P = _lib.MXFP6_PROTOTYPES
    assert set(P) == {"rtv_quantize_mxfp6", "rtv_layernorm_modulate_mxfp6", "rtv_gemm_mxfp6"}
    # the argument lists of the MXFP4 twins
    for name, proto in P.items():
        assert proto == _lib.MXFP4_PROTOTYPES[name.replace("mxfp6", "mxfp4")], name
    q = P["rtv_quantize_mxfp6"][1]
    assert [q[i] for i in (1, 5, 7)] == [ctypes.c_int64] * 3 and len(q) == 9
    assert P["rtv_gemm_mxfp6"][1][4:6] == [ctypes.c_void_p, ctypes.c_void_p] and len(P["rtv_gemm_mxfp6"][1]) == 20
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_struct_fields_and_abi_are_unchanged():
    from realtime_video_amd import _lib
    assert [n for n, _ in _lib.STRUCTS["rtv_dit_weights"]._fields_][-2:] == ["fp8_scales", "fp8_row_scales"]
    assert [n for n, _ in _lib.STRUCTS["rtv_dit_config"]._fields_][-2:] == ["use_fp8", "max_attn_kv_splits"]
    assert _lib.ABI_VERSION == 105


# rtv_dit_workspace_bytes of commit 16c47ca (the parent of the MXFP6 mode) on the shape of tests/test_mxfp4_cpu.py.  Literals on
# purpose - not to be regenerated from the library.
PARENT_WORKSPACE = {0: 190635008, 1: 232567808, 2: 232586752, 3: 232567808}


def test_workspace_of_the_other_modes_is_the_parents_and_mode_4_fits_the_fp8_buffer():
    from realtime_video_amd import _lib
    lib = _lib.load()
    Cfg = _lib.STRUCTS["rtv_dit_config"]
    sizes = {}
    for mode in (0, 1, 2, 3, 4):
        cfg = Cfg(dim=1536, ffn_dim=8960, num_heads=12, num_layers=2, freq_dim=256, text_dim=4096, text_len=512, in_dim=16,
                  out_dim=16, eps=1e-6, use_fp8=mode, max_attn_kv_splits=0)
        sizes[mode] = lib.rtv_dit_workspace_bytes(ctypes.byref(cfg), 3, 30, 52)
    assert {m: sizes[m] for m in (0, 1, 2, 3)} == PARENT_WORKSPACE
    # codes (rows * 3 K / 4) and block scales (rows * K / 32) of the widest activation fit the fp8 buffer (rows * K): 25 / 32 of it
    assert sizes[4] == sizes[1] and sizes[4] - sizes[0] >= max(3 * 30 * 52, 512) * 8960 * 25 // 32


# ----------------------------------------------------------------------------------------- refusals, before any launch
def _cpu_model(**kw):
    from realtime_video_amd.causal_model import CausalWanModel
    args = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=1, text_dim=256, device="cpu")
    args.update(kw)
    return CausalWanModel(**args)


def test_enable_mxfp6_refuses_a_width_that_is_no_multiple_of_128():
    with pytest.raises(ValueError, match="multiple of 128"):
        _cpu_model(text_dim=192).enable_mxfp6()
    with pytest.raises(ValueError, match="multiple of 128"):
        _cpu_model(ffn_dim=576).enable_mxfp6()


def test_enable_mxfp6_is_exclusive_with_the_other_modes_in_both_orders():
    for mode in (1, 2, 3):
        model = _cpu_model()
        model._cfg.use_fp8 = mode                                    # what enable_fp8() / enable_fp8("row") / enable_mxfp4() leave behind
        with pytest.raises(RuntimeError, match="reload the weights first"):
            model.enable_mxfp6()
    model = _cpu_model()
    model._cfg.use_fp8 = 4                                           # and the other direction
    with pytest.raises(RuntimeError, match="reload the weights first"):
        model.enable_fp8()
    with pytest.raises(RuntimeError, match="reload the weights first"):
        model.enable_fp8("row")
    with pytest.raises(RuntimeError, match="reload the weights first"):
        model.enable_mxfp4()
    assert model.enable_mxfp6() is model                             # a second call is a no-op


def test_enable_mxfp6_refuses_context_parallelism():
    from realtime_video_amd.parallel import SimulatedContextParallel
    model = _cpu_model()
    model.context_parallel = SimulatedContextParallel(2, "rows")
    with pytest.raises(RuntimeError, match="context parallelism"):
        model.enable_mxfp6()


def test_launch_checks_come_before_any_launch():
    """The argument checks come before anything touches the device: the pointers here are never read."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)

    def gemm(K=128, N=8, lda=96, ldw=96, A=p, a_scales=p, w_scales=p):
        st = lib.rtv_gemm_mxfp6(A, lda, p, ldw, a_scales, w_scales, p, 8, 1, N, K, None, 0, None, 0, 0, 0, None, 0, None)
        return st, lib.rtv_last_error().decode()

    for K in (64, 192, 352):
        st, msg = gemm(K=K, lda=K // 4 * 3 + 15 & ~15, ldw=K // 4 * 3 + 15 & ~15)
        assert st != 0 and "multiple of 128" in msg
    st, msg = gemm(N=12)
    assert st != 0 and "N must be a multiple of 8" in msg
    for kw in (dict(lda=100), dict(ldw=104), dict(lda=80)):          # not 16-byte rows; shorter than 3 K / 4
        st, msg = gemm(**kw)
        assert st != 0 and "leading dimensions" in msg
    st, msg = gemm(A=ctypes.c_void_p(base + 8))
    assert st != 0 and "16-byte aligned" in msg
    st, msg = gemm(a_scales=ctypes.c_void_p(base + 2))
    assert st != 0 and "4-byte aligned" in msg
    st = lib.rtv_gemm_mxfp6(p, 1 << 20, p, 96, p, p, p, 8, 4096, 8, 128, None, 0, None, 0, 0, 0, None, 0, None)
    assert st != 0 and "4 GiB" in lib.rtv_last_error().decode()
    st = lib.rtv_quantize_mxfp6(p, 48, 1, 48, p, 36, p, 4, None)
    assert st != 0 and "multiple of 32" in lib.rtv_last_error().decode()
    st = lib.rtv_quantize_mxfp6(p, 64, 1, 64, p, 40, p, 4, None)     # a row of 64 elements needs 48 bytes of codes
    assert st != 0 and "3 d / 4" in lib.rtv_last_error().decode()


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


@pytest.mark.parametrize("unit,kernels", [("gemm_mxfp6", 1), ("mxfp6", 4)])
def test_new_kernels_have_no_scratch_and_no_spills(tmp_path, unit, kernels):
    asm = _device_asm(tmp_path, unit)
    meta = _kernel_metadata(asm)
    assert len(meta) == kernels and all("mxfp6" in n for n in meta), list(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    if unit == "gemm_mxfp6":
        (m,) = meta.values()
        assert m["vgpr_count"] <= 256                                                   # two waves per SIMD
        mfma = re.findall(r"^\s*(v_mfma\S*) .*$", asm, flags=re.M)
        lines = re.findall(r"^\s*v_mfma_scale_f32_32x32x64_f8f6f4 .*cbsz:2 blgp:2\s*$", asm, flags=re.M)
        assert len(lines) >= 32 and len(lines) == len(mfma), (len(lines), len(mfma))   # nothing but the block-scaled FP6 MFMA
        # the fragment reads stay 8-byte reads: a paired read is banked over 128 bytes and runs at half the rate
        assert not re.search(r"^\s*ds_read2", asm, flags=re.M)
        # every MFMA of the K loop sits in its phase: four between two barriers (the compiler may otherwise sink them)
        loop = asm[asm.index("Inner Loop Header"):]
        runs = [len(re.findall(r"v_mfma_scale", seg)) for seg in loop.split("s_barrier")[:16]]
        assert max(runs) <= 4, runs
