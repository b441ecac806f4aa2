"""Cases for the text encoder's e4m3 weight storage: the weight-only fp8 GEMM rtv_gemm_w8 (csrc/gemm_w8.hip, include/rtv_hip_t5_w8.h)
and the encoder on dequantised weights.  Cases, references, named slips; no GPU and no pytest in here.  tests/test_t5_w8_cpu.py proves
that the acceptance would notice each slip, tests/test_t5_w8_gpu.py holds the kernel and the encoder to it.

The arithmetic every test pins, for x [M, K] bf16 and codes c [N, K] e4m3 with row scales s [N]:
    y[m, n] = bf16( fp32_acc( sum_k x[m, k] * value(c[n, k]) ) * s[n] )
Why integers: A and the codes are iid integers in [-8, 8] (exact in bf16 and in e4m3), build() asserts (|A| @ |W|^T).max() < 2^24,
so every partial sum over any subset of K in any order is an integer fp32 holds exactly: the K steps, the permuted k order inside a
step, the K segments and the order of the slab reduction cannot show.  The kernel then does ONE fp32 multiplication and ONE rounding
to bf16, which torch restates bit for bit: bf16(fp32(sum) * s).  With power-of-two scales the product is exact too (the exact
cases); the case "odd_scales" has full-mantissa scales so that a scale folded into a bf16 operand shows.

The decode table: a sum starts at +0, so the one product x * value(-0) = -0 gives +0 + -0 = +0: the arithmetic above maps the code
0x80 to +0, and that is what the table expects of it (a decode of 0x80 to anything but a zero still shows)."""
import dataclasses

import torch

BF = torch.bfloat16
E4 = torch.float8_e4m3fn
# the kernel's constants (csrc/gemm_w8.hip), restated
KSTEP = 128                     # k per step; K % KSTEP == 0
STRIP = 64                      # output channels per workgroup
CHUNK = 128                     # rows per workgroup at most
RING = 4                        # K steps of codes in flight: whole rounds run in one code path, the steps left in another
TARGET_WGS = 512                # strips x segments the plan aims at
MAX_SEGMENTS = 16
EXACT_MAX = 2 ** 24
NAN_CODE = 0x7F
GUARD_ROWS = 8                  # rows of NaN in front of and behind a strided operand
PAD_A, PAD_W = 16, 32           # lda = K + 16 elements, ldw = K + 32 bytes
PAD_OUT, OUT_OFFSET = 16, 8     # the output is a window at column 8 of rows 16 elements longer
SENTINEL = -1.5                 # what the output buffer holds around the window
ENCODER_WIDTHS = (4096, 10240)  # every K the encoder uses


# ------------------------------------------------------------------------------------------------ the K plan
def segments(N, K):
    """K segments for (N, K) - w8_segments: a function of N and K alone."""
    steps, strips = K // KSTEP, -(-N // STRIP)
    return max(1, min(-(-TARGET_WGS // strips), MAX_SEGMENTS, steps // 2))


def segment_steps(N, K):
    """[(first K step, end K step)] of every segment."""
    steps, S = K // KSTEP, segments(N, K)
    return [(s * steps // S, (s + 1) * steps // S) for s in range(S)]


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    transpose: bool = False
    odd_scales: bool = False
    seed: int = 0


def _both(name, M, N, K, seed):
    return [Case(name, M, N, K, False, seed=seed), Case(name + "_t", M, N, K, True, seed=seed)]


K_CASES = (_both("k_one_step", 32, STRIP, KSTEP, 1) + _both("k_two_steps", 32, STRIP, 2 * KSTEP, 2) +
           _both("k_three_steps", 32, STRIP, 3 * KSTEP, 3) +                  # an odd count, still one segment
           _both("k_smallest_cut", 32, STRIP, 4 * KSTEP, 4) +                 # two segments of two steps
           _both("k_unequal_segments", 32, STRIP, 5 * KSTEP, 5) +             # segments of two and three steps
           _both("k_four_segments", 32, STRIP, 9 * KSTEP, 6))                 # 2, 2, 2, 3
# segments longer than the ring: one round and a step (N = 4096 cuts K into 8), one round and three steps
RING_CASES = [Case("ring_round_and_one", 32, 4096, 8 * 5 * KSTEP, seed=7), Case("ring_round_and_three", 32, 4096, 8 * 7 * KSTEP, seed=8)]
N_CASES = (_both("n_sixteen", 32, 16, 2 * KSTEP, 10) + _both("n_one_strip", 32, STRIP, 2 * KSTEP, 11) +
           _both("n_strip_and_16", 32, STRIP + 16, 2 * KSTEP, 12) + _both("n_ragged_strips", 32, 3 * STRIP + 16, 2 * KSTEP, 13))
M_CASES = [c for i, M in enumerate((32, 64, 96, 128, 160, 512)) for c in _both(f"m_{M}", M, STRIP + 16, 5 * KSTEP, 20 + i)]
MODEL_CASES = [Case("model_qk", 32, 8192, 4096, seed=30), Case("model_o", 32, 4096, 4096, seed=31),
               Case("model_v_t", 32, 4096, 4096, True, seed=32), Case("model_gate_fc1", 32, 20480, 4096, seed=33),
               Case("model_fc2", 32, 4096, 10240, seed=34)]
ODD_SCALES = [Case("odd_scales", 32, STRIP + 16, 5 * KSTEP, odd_scales=True, seed=40)]
SMALL_CASES = K_CASES + N_CASES + M_CASES + ODD_SCALES
EXACT_CASES = SMALL_CASES + RING_CASES + MODEL_CASES


def by_name(name):
    return next(c for c in EXACT_CASES if c.name == name)


@dataclasses.dataclass
class Operands:
    a: torch.Tensor             # bf16 [M][K]
    codes: torch.Tensor         # uint8 [N][K]: e4m3 bit patterns
    s: torch.Tensor             # float32 [N]
    isum: torch.Tensor = None   # float64 [M][N], filled by build()
    max_int: int = 0


def value(codes, layout=E4):
    """The float32 value of every code (uint8 bit patterns)."""
    return codes.view(layout).float()


def scales(N, odd=False):
    s = 2.0 ** (-(torch.arange(N) % 23)).float()                  # changes with every row: a shifted index shows
    if odd:
        s = s * (1.0 + (torch.arange(N) % 97 + 1).float() / 128.0 + 2.0 ** -20)     # mantissas bf16 cannot hold
    return s


def operands(c, launch=0):
    g = torch.Generator().manual_seed(3000 + 11 * c.seed + launch)
    a = torch.randint(-8, 9, (c.M, c.K), generator=g).float()
    w = torch.randint(-8, 9, (c.N, c.K), generator=g).float()
    codes = w.to(E4)
    assert torch.equal(codes.float(), w)
    return Operands(a.to(BF), codes.view(torch.uint8), scales(c.N, c.odd_scales))


def build(c, launch=0, device="cpu"):
    """Operands with the exact integer product and the exactness condition asserted."""
    o = operands(c, launch)
    a, w = o.a.to(device).double(), value(o.codes).to(device).double()
    o.max_int = int((a.abs() @ w.abs().t()).max())
    assert o.max_int < EXACT_MAX, (c.name, o.max_int)
    o.isum = (a @ w.t()).cpu()
    return o


def finish(acc, s, transpose=False):
    """fp32 sums [M][N] -> what the kernel stores: one fp32 multiplication, one rounding; [N][M] when transposed."""
    y = (acc.float() * s.float()[None, :]).to(BF)
    return y.t().contiguous() if transpose else y


def reference(c, o):
    return finish(o.isum, o.s, c.transpose)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.uint8)


def mismatches(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape)
    return int((bits(a.cpu()) != bits(b.cpu())).sum())


# ------------------------------------------------------------------------------------------------ strided operands, output windows
def guarded_a(a, device):
    M, K = a.shape
    buf = torch.full((M + 2 * GUARD_ROWS, K + PAD_A), float("nan"), dtype=BF, device=device)
    buf[GUARD_ROWS:GUARD_ROWS + M, :K] = a.to(device)
    return buf, buf[GUARD_ROWS:GUARD_ROWS + M, :K]


def guarded_codes(codes, device):
    N, K = codes.shape
    buf = torch.full((N + 2 * GUARD_ROWS, K + PAD_W), NAN_CODE, dtype=torch.uint8, device=device)
    buf[GUARD_ROWS:GUARD_ROWS + N, :K] = codes.to(device)
    return buf, buf[GUARD_ROWS:GUARD_ROWS + N, :K].view(E4)


def output_window(rows, cols, device):
    buf = torch.full((rows, cols + PAD_OUT), SENTINEL, dtype=BF, device=device)
    return buf, buf[:, OUT_OFFSET:OUT_OFFSET + cols]


def sentinels_changed(buf, cols):
    keep = torch.ones(buf.shape[1], dtype=torch.bool)
    keep[OUT_OFFSET:OUT_OFFSET + cols] = False
    return int((buf[:, keep.to(buf.device)] != SENTINEL).sum())


# ------------------------------------------------------------------------------------------------ the decode table
DECODE_M, DECODE_N, DECODE_K = 256, 16, 256


def decode_table():
    """W rows hold all 254 non-NaN codes (row n is the byte sequence rotated by 17 n; the two NaN codes become 0x00), A is the
    identity: y[m, n] = bf16(value(W[n, m]) * s[n]), exact with power-of-two scales - subnormal codes, +-448, and 0x80 as +0 (the
    module docstring).  Two row chunks, one segment."""
    k = torch.arange(DECODE_K)
    codes = ((k[None, :] + 17 * torch.arange(DECODE_N)[:, None]) % 256).to(torch.uint8)
    codes[(codes & 0x7F) == NAN_CODE] = 0
    assert torch.unique(codes).numel() == 254
    a = torch.eye(DECODE_M, DECODE_K).to(BF)
    s = scales(DECODE_N)
    c = Case("decode_table", DECODE_M, DECODE_N, DECODE_K)
    return c, Operands(a, codes, s, isum=None)


def decode_reference(o):
    """bf16(value(W[n, m]) * s[n]) as [m][n]; + 0.0 is the accumulator the one product is added to (-0 -> +0)."""
    return finish(value(o.codes).double().t() + 0.0, o.s)


# ------------------------------------------------------------------------------------------------ the kernel restated, and its slips
SLIPS = {
    "scale_of_previous_row": "y[m, n] scaled with s[n - 1]",
    "scale_in_bf16_before_accumulation": "the weights dequantised to bf16(value * s) in front of the MFMA, no scale behind it",
    "last_k_step_dropped": "the K loop ends one step early",
    "segment_dropped": "the reduction leaves the last slab out",
    "segment_twice": "the reduction adds the first slab twice",
    "transposed_strides_exchanged": "the transposed store writes C[m * ldc + n]",
    "e5m2_layout": "a code decoded as e5m2",
    "subnormals_flushed": "codes with a zero exponent field decoded as zero",
    "second_chunk_reads_first": "the rows of the second row chunk read the first chunk's rows of A",
}


def emulate(c, o, slip=None):
    """The kernel's structure in float64 on exact data: per segment a partial sum, the slabs added in ascending order, one scale, one
    rounding; `slip` names a mutation.  Without a slip this equals reference() on the exact cases."""
    assert slip is None or slip in SLIPS
    a = o.a.double()
    w = value(o.codes, torch.float8_e5m2 if slip == "e5m2_layout" else E4).double()
    if slip == "subnormals_flushed":
        w = torch.where((o.codes & 0x78) == 0, torch.zeros_like(w), w)
    s = o.s.clone()
    if slip == "scale_of_previous_row":
        s = torch.roll(s, 1)
    if slip == "scale_in_bf16_before_accumulation":
        w = (w.float() * s[:, None]).to(BF).double()
        s = torch.ones_like(s)
    if slip == "second_chunk_reads_first" and c.M > CHUNK:
        a = a[torch.arange(c.M) % CHUNK]
    slabs = []
    segs = segment_steps(c.N, c.K)
    for i, (k0, k1) in enumerate(segs):
        if slip == "last_k_step_dropped" and i == len(segs) - 1:
            k1 -= 1
        slabs.append(a[:, k0 * KSTEP:k1 * KSTEP] @ w[:, k0 * KSTEP:k1 * KSTEP].t())
    if slip == "segment_dropped" and len(slabs) > 1:
        slabs = slabs[:-1]
    if slip == "segment_twice" and len(slabs) > 1:
        slabs = [slabs[0]] + slabs
    acc = slabs[0]
    for part in slabs[1:]:
        acc = acc + part
    y = finish(acc, s, False)
    if not c.transpose:
        return y
    if slip == "transposed_strides_exchanged":
        assert c.N >= c.M
        flat = torch.full((c.N * c.M,), SENTINEL, dtype=BF)          # a dense [N][M] buffer written at m * ldc + n, ldc = M
        idx = (torch.arange(c.M)[:, None] * c.M + torch.arange(c.N)[None, :]).reshape(-1)
        flat[idx] = y.reshape(-1)                                    # later writes win, as good a model as any: it is wrong anyway
        return flat.view(c.N, c.M)
    return y.t().contiguous()


def slip_applies(c, slip, decode=False):
    """Whether `slip` can change this case at all."""
    if slip == "subnormals_flushed":
        return decode
    if decode:
        return slip in ("scale_of_previous_row", "e5m2_layout", "second_chunk_reads_first", "last_k_step_dropped")
    if slip == "scale_in_bf16_before_accumulation":
        return c.odd_scales
    if slip in ("segment_dropped", "segment_twice"):
        return segments(c.N, c.K) > 1
    if slip == "transposed_strides_exchanged":
        return c.transpose and c.N >= c.M
    if slip == "second_chunk_reads_first":
        return c.M > CHUNK
    return True


# ------------------------------------------------------------------------------------------------ row locality
LOCALITY_SHAPES = [(3 * STRIP + 16, 5 * KSTEP), (STRIP + 16, 2 * KSTEP)]        # cut into unequal segments; one segment
LOCALITY_MS = (32, 96, 160)


def gaussian_problem(N, K, M=max(LOCALITY_MS), seed=0):
    """Gaussian rows and quantised Gaussian weights: (a bf16 [M][K], codes uint8 [N][K], scales [N])."""
    from fp8_rows_oracle import fp8_rows_quantize
    g = torch.Generator().manual_seed(5000 + seed)
    a = torch.randn(M, K, generator=g).to(BF)
    q, s = fp8_rows_quantize((torch.randn(N, K, generator=g) * K ** -0.5).to(BF))
    return a, q.view(torch.uint8), s.reshape(-1).contiguous()


# ------------------------------------------------------------------------------------------------ the encoder
LINEAR_KEYS = ("attn.q.weight", "attn.k.weight", "attn.v.weight", "attn.o.weight", "ffn.gate.0.weight", "ffn.fc1.weight",
               "ffn.fc2.weight")


def quantised(w, key):
    """(codes, scales [N, 1]) of one matrix of the state dict as enable_fp8_weights() makes them: the bf16 checkpoint value through
    the quantiser restatement of tests/fp8_rows_oracle.py."""
    from fp8_rows_oracle import fp8_rows_quantize
    return fp8_rows_quantize(w[key].to(BF))


def dequantised(w):
    """The state dict with the matrices of every Linear replaced by value(c) * s_w (float64: the product is exact there; the fp64 and
    fp32 chains of t5_cases.encoder_chain cast it to their own type)."""
    out = dict(w)
    for key in w:
        if key.startswith("blocks.") and key.split(".", 2)[2] in LINEAR_KEYS:
            q, s = quantised(w, key)
            out[key] = q.double() * s.double()
    return out
