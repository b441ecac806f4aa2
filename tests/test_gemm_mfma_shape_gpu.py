"""GEMM checks that do not depend on the shape of the matrix instruction (32x32x16 or 16x16x32) a kernel is built on: exact-integer
products and exact epilogue chains catch any fragment, accumulator or epilogue mapping slip bit for bit whatever the order of the
fp32 sums; split-K and deep-K checks carry the bars of test_kernels_gpu.py.  They hold for the product library (gemm8 on 16x16x32)
and for its -DRTV_G8_MFMA16=0 A/B build (32x32x16, RTV_LIB_PATH=.../librtv_hip_m32.so) alike."""
import functools

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFGS = (0, 4, 5, 6, 7, 9, 19)   # default dispatch, 256x256 (plain / split-K), 128x256 (plain / split-K), 160x256 (split-K / plain)


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    _ops.ensure_gemm_workspace(torch.device(DEV))
    return _ops


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _randn(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(torch.bfloat16).to(DEV)


def _tern(rows, cols, seed):
    """entries in {-1, 0, 1}"""
    return (torch.randint(-1, 2, (rows, cols), generator=_gen(seed)).to(torch.bfloat16)).to(DEV)


@functools.lru_cache(maxsize=None)
def _integer_problem(M, N, K, k_pad=0):
    """(a, w, exact product as bf16): 256 or fewer non-zero K columns, so every output is an integer of magnitude <= 256, exact in
    fp32 in any summation order and exact in bf16.  k_pad: the K columns are spread evenly over k_pad columns, zeros between."""
    a, w = _tern(M, K, 11), _tern(N, K, 12)
    if k_pad:
        step = k_pad // K
        ap, wp = torch.zeros(M, k_pad, dtype=a.dtype, device=DEV), torch.zeros(N, k_pad, dtype=a.dtype, device=DEV)
        ap[:, ::step], wp[:, ::step] = a, w
        a, w = ap, wp
    ref = a.float() @ w.float().t()
    assert float(ref.abs().max()) <= 256 and torch.equal(ref, ref.round())
    return a, w, ref.to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(1, 264, 192), (37, 200, 128), (161, 264, 192), (300, 520, 256), (585, 1536, 256), (4680, 512, 128)])
def test_gemm_exact_integer_product(ops, M, N, K):
    """A, W in {-1, 0, 1}: the fp32 product is exact whatever the order of the sums, so every tile config must return it bit for bit:
    one-row and ragged problems, a last column tile of 8 columns, several tiles, the ragged 19th row tile with idle waves (4680)."""
    a, w, ref = _integer_problem(M, N, K)
    for cfg in CFGS:
        out = ops.gemm(a, w, tile_cfg=cfg)
        assert torch.equal(out, ref), (cfg, int((out != ref).sum()))


@pytest.mark.parametrize("M,N,K", [(128, 32, 256), (256, 96, 64), (4096, 32, 4096)])
def test_gemm_exact_integer_product_value_projection(ops, M, N, K):
    """The text encoder's value projection V^T = W_v . n^T (t5_encoder.hip): A is the weight [dim_attn, dim], W the normed rows
    [rows, dim], the output [dim_attn, rows] with ldc = rows - N as small as 32, where every other GEMM test starts at 64.  The
    same integer-exact product, every tile config; at K = 4096 the 256 non-zero K columns are spread over the whole depth.  K = 64 is
    one K tile: the 160x256 kernel (tile configs 9 and 19, which the default dispatch takes from K = 1024 on only) needs two and
    says so instead of computing."""
    a, w, ref = _integer_problem(M, N, min(K, 256), K if K > 256 else 0)
    assert a.shape == (M, K) and w.shape == (N, K)
    for cfg in CFGS:
        if K < 128 and cfg in (9, 19):
            with pytest.raises(RuntimeError, match="gemm5: K must be a multiple of 64, >= 128"):
                ops.gemm(a, w, tile_cfg=cfg)
            continue
        out = ops.gemm(a, w, tile_cfg=cfg)
        assert out.stride(0) == N and torch.equal(out, ref), (cfg, int((out != ref).sum()))


def _direct_epilogue_out(M, N):
    """an output whose rows are 8 bytes off 16-byte alignment: the kernels take the direct register-layout epilogue (no LDS image)"""
    return torch.empty(M, N + 8, dtype=torch.bfloat16, device=DEV)[:, 4:4 + N]


@pytest.mark.parametrize("M,N,K", [(161, 264, 192), (300, 520, 256)])
def test_gemm_exact_integer_product_direct_epilogue(ops, M, N, K):
    a, w, ref = _integer_problem(M, N, K)
    for cfg in CFGS:
        out = ops.gemm(a, w, out=_direct_epilogue_out(M, N), tile_cfg=cfg)
        assert torch.equal(out, ref), (cfg, int((out != ref).sum()))


def _gelu_tanh64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _gelu_safe_bias(n, seed):
    """n random bf16 values whose GELU-tanh lies well inside a bf16 rounding interval, so that the expected bf16 is unambiguous.  The
    kernel evaluates 0.5 x (1 + tanh u) as 0.5 x (2 - 2 / (1 + exp 2u)) in fp32 with a fast exponential: the absolute error of the
    bracket is a few fp32 ulps of 2 (~2e-7), i.e. <= 2e-6 relative for x >= -1.5 where the bracket is >= 0.13 (further down it
    cancels).  Values within 2^-11 = 5e-4 (relative; a quarter of the bf16 half-ulp) of a rounding boundary are not used.
    Returns (bias, bf16(gelu(bias)))."""
    cand = (torch.randn(16 * n, generator=_gen(seed)) * 1.5).to(torch.bfloat16)
    y = _gelu_tanh64(cand)
    yb = y.float().to(torch.bfloat16)
    ulp = torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(1e-30))) - 7)      # bf16 spacing at y
    dist_to_boundary = ulp / 2 - (y - yb.double()).abs()
    ok = (dist_to_boundary > y.abs() * 2.0 ** -11) & (y.abs() > 1e-3) & (cand.double() >= -1.5)
    idx = torch.nonzero(ok).flatten()[:n]
    assert idx.numel() == n
    return cand[idx].to(DEV), yb[idx].to(DEV)


@functools.lru_cache(maxsize=None)
def _epilogue_problem():
    M, N, K, rpf = 300, 264, 128, 101   # frame boundaries (101, 202) inside a 16-row block; the last column tile holds 8 columns
    a = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    w = _randn(N, K, seed=2)
    bias, gate, res = _randn(N, seed=3), _randn(3, N, seed=5), _randn(M, N, seed=4)
    frame = (torch.arange(M, device=DEV) // rpf)
    # y = bf16(0 + bias) = bias;  t = bf16(y * gate);  out = bf16(res + t)   (products of two bf16 are exact in fp32)
    t = (bias.float()[None, :] * gate.float()[frame]).to(torch.bfloat16)
    exp_gate_res = (res.float() + t.float()).to(torch.bfloat16)
    gbias, gexp = _gelu_safe_bias(N, 7)
    return dict(M=M, N=N, rpf=rpf, a=a, w=w, bias=bias, gate=gate, res=res, exp_gate_res=exp_gate_res, gbias=gbias,
                exp_gelu=gexp[None, :].expand(M, N).contiguous())


@pytest.mark.parametrize("direct", [False, True])
def test_gemm_epilogue_mapping_exact(ops, direct):
    """A = 0, so the output is the epilogue of a zero accumulator: every element depends on its own (row, column) only through bias,
    gate row (frame of the row) and residual, and the chain y = bf16(acc + bias); y = bf16(act(y)); t = bf16(y * gate);
    out = bf16(res + t) restated in torch must come back bit for bit - for the LDS-image epilogue and the direct one."""
    p = _epilogue_problem()
    M, N = p["M"], p["N"]
    for cfg in CFGS:
        mk = (lambda: _direct_epilogue_out(M, N)) if direct else (lambda: None)
        out = ops.gemm(p["a"], p["w"], bias=p["gbias"], act=1, out=mk(), tile_cfg=cfg)
        assert torch.equal(out, p["exp_gelu"]), ("bias + gelu", cfg, int((out != p["exp_gelu"]).sum()))
        out = ops.gemm(p["a"], p["w"], bias=p["bias"], gate=p["gate"], gate_stride=N, rows_per_frame=p["rpf"], residual=p["res"],
                       out=mk(), tile_cfg=cfg)
        assert torch.equal(out, p["exp_gate_res"]), ("bias + gate + residual", cfg, int((out != p["exp_gate_res"]).sum()))
        out = ops.gemm(p["a"], p["w"], out=mk(), tile_cfg=cfg)
        assert torch.equal(out, torch.zeros_like(out)), ("none", cfg)


@pytest.mark.parametrize("M,N,K,cfg", [(300, 520, 2048, 5), (585, 1536, 5120, 7)])
def test_gemm_split_k_register_image(ops, M, N, K, cfg):
    """Split-K publishes the accumulators as a per-lane register image and the reducer adds images elementwise, whatever the grouping
    of the registers into MFMA blocks: repeatable bits, the rel-L2 bar of test_gemm_split_k_sum_order_is_fixed against the fp32
    product, and exact on integer inputs (256 non-zero K columns spread over all K segments)."""
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    outs = [ops.gemm(a, w, bias=b, tile_cfg=cfg).clone() for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    err = rel_l2(outs[0], a.float() @ w.float().t() + b.float())
    print(f"split-K {M}x{N}x{K} cfg {cfg}: rel-L2 {err:.3e}")
    assert err <= 1e-2
    ai, wi, ref = _integer_problem(M, N, 256, K)
    out = ops.gemm(ai, wi, tile_cfg=cfg)
    assert torch.equal(out, ref), int((out != ref).sum())


def test_gemm_random_data_at_depth(ops):
    M, N, K = 4680, 512, 5120
    a, w, b = _randn(M, K, seed=1), _randn(N, K, seed=2, scale=K ** -0.5), _randn(N, seed=3, scale=0.1)
    err = rel_l2(ops.gemm(a, w, bias=b, tile_cfg=0), a.float() @ w.float().t() + b.float())
    print(f"default dispatch {M}x{N}x{K}: rel-L2 {err:.3e}")
    assert err <= 1e-2
