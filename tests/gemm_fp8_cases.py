"""Bit-exact cases for the fp8 Linear path: the two e4m3 GEMM kernels (csrc/gemm_fp8.hip, csrc/gemm_fp8_rows.hip - one body,
csrc/gemm_fp8_body.h, around two de-quantise steps) and the per-tensor activation quantiser of csrc/gemm_fp8.hip.  Cases, integer
operands, plain references, named slips.  No GPU and no pytest in here; tests/test_gemm_fp8_cases_cpu.py proves that the acceptance
would notice each slip, tests/test_gemm_fp8_exact_gpu.py holds the kernels to it.

Why integers: A and W are iid integers in [-8, 8] (exact in e4m3), every scale is a power of two.  build() asserts
(|A| @ |W|^T).max() < 2^24, so every partial sum over any subset of K in any order is an integer that fp32 holds exactly - the
K-tile order, the split-K segments and the order of the slab reduction cannot show - and that the scaled sum is representable in
fp32, so the expected output is bf16(RNE(exact)) bit for bit: one rounding.  With a bias the kernel's own chain is restated:
bf16(fp32(exact) + fp32(bias)), one fp32 addition and one rounding.

Not observable with such data, and therefore not among the slips: the order of the fp32 additions (K-tiles, MFMA steps, slabs)
and the order of the two scale multiplications - every intermediate is exact either way.  The Gaussian tests of
tests/test_fp8_rows_gpu.py and tests/test_kernels_gpu.py cover those."""
import dataclasses

import torch

BF = torch.bfloat16
E4 = torch.float8_e4m3fn
BM = BN = 256                   # output tile of the kernel body
BK = 128                        # K-tile in e4m3 elements = bytes
GROUP_M = 8                     # rows of tiles per supertile of the tile order
G_PLAN = 256                    # compute units the recorded plans are worked out for
MAX_S = 8                       # most K segments per split tile
SPLIT_MAX_UNITS = 256           # slabs in the workspace (csrc/gemm_split.h)
EXACT_MAX = 2 ** 24             # integers below are exact in fp32
S_X, S_W = 2.0 ** -3, 2.0 ** -5  # the per-tensor kernel's scales
NAN_CODE = 0x7F                 # e4m3fn NaN (0xFF is the other one)
GUARD_ROWS = 64                 # rows of NaN codes in front of and behind a strided operand
GUARD_OUT = -1.5                # value of the guard columns beside an output slice
PAD_A, PAD_W = 16, 32           # padding columns of the strided operands: lda = K + 16, ldw = K + 32


# ------------------------------------------------------------------------------------------------ the split-K plan
def plan(T, nk, G=G_PLAN):
    """(R, S, split_first) of plan_split_k (csrc/gemm8.hip) for T tiles of nk K-tiles on G compute units with a workspace
    attached, allow_half = false and extra_units = 0 - what both fp8 launchers pass.  R = tiles of the partial last round that
    are cut along K (0: no split), S = K segments per such tile (1: no split), split_first = 1: the split units take the lowest
    block ids."""
    R = T % G
    if R > 0:
        S = min(G // R, MAX_S, nk // 4)         # the units fit one round; at least 4 K-tiles per segment
        if S >= 2 and R * S <= SPLIT_MAX_UNITS:
            return R, S, int(R * S * 4 <= G)
    return 0, 1, 0


def segments(nk, S):
    """[(kt_begin, kt_end)] of the S segments of a split tile (split_unit_of_block, csrc/gemm_split.h)."""
    return [(nk * s // S, nk * (s + 1) // S) for s in range(S)]


# ------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    plan: tuple                 # (R, S, split_first) the case is meant to take at G_PLAN compute units
    big: bool = False           # reference too large for the CPU proof: build() runs where the GPU test runs
    seed: int = 0

    @property
    def tiles_m(self):
        return -(-self.M // BM)

    @property
    def tiles_n(self):
        return -(-self.N // BN)

    @property
    def tiles(self):
        return self.tiles_m * self.tiles_n

    @property
    def nk(self):
        return self.K // BK

    @property
    def needs_g_plan(self):
        """True when the recorded plan holds at G_PLAN compute units only: the case splits, or has more tiles than one round."""
        return self.plan[1] > 1 or self.tiles > G_PLAN


def _depth(K, pl):
    return Case(f"depth_257_264_{K}", 257, 264, K, pl, seed=K // BK)


# (257, 264, K): four tiles, an M tail of one row, a last column tile of 8 columns
DEPTH_CASES = [_depth(128, (0, 1, 0)),          # one K-tile: the checked tail instantiation alone
               _depth(256, (0, 1, 0)),          # both checked tail tiles
               _depth(384, (0, 1, 0)),          # one steady-state trip
               _depth(640, (0, 1, 0)),          # three steady-state trips, still under 4 K-tiles per segment
               _depth(1024, (4, 2, 1)),         # two segments of 4: own registers + the other slab
               _depth(1664, (4, 3, 1)),         # segments of 4, 4 and 5 K-tiles: the reduction from zero over all slabs
               _depth(4096, (4, 8, 1))]         # the most segments
# the smallest legal problems: the clamped scale reads at M - 1 and N - 4; at K = 1024 a single tile is split
MIN_CASES = [Case("min_1_8_128", 1, 8, 128, (0, 1, 0), seed=40), Case("min_1_8_1024", 1, 8, 1024, (1, 2, 1), seed=41)]
TILE_MAP_CASES = [
    Case("supertile_short_group_2100_520_128", 2100, 520, 128, (0, 1, 0), seed=50),    # 9 x 3 tiles: the last group has one row
    Case("split_first_4680_3592_1024", 4680, 3592, 1024, (29, 2, 1), big=True, seed=51),    # 19 x 15 = 285 tiles
    Case("split_last_1800_9224_1024", 1800, 9224, 1024, (40, 2, 0), big=True, seed=52),     # 8 x 37 = 296 tiles
]
GEMM_CASES = DEPTH_CASES + MIN_CASES + TILE_MAP_CASES
DIRECT_STORE_CASES = [c for c in DEPTH_CASES if c.K in (384, 1664)]       # bias into an output 8 bytes off 16-byte alignment
STRIDED_CASES = [c for c in DEPTH_CASES if c.K in (640, 1024)]            # one unsplit, one split


def by_name(name):
    return next(c for c in GEMM_CASES if c.name == name)


# ------------------------------------------------------------------------------------------------ operands
@dataclasses.dataclass
class Operands:
    a: torch.Tensor             # float32 integers [M][K]
    w: torch.Tensor             # float32 integers [N][K]
    aq: torch.Tensor            # the same as e4m3
    wq: torch.Tensor
    sa: torch.Tensor            # float32 [M]: the per-row kernel's activation scales
    sw: torch.Tensor            # float32 [N]
    bias: torch.Tensor          # bf16 [N] (always built; a run may leave it out)
    isum: torch.Tensor = None   # float64 [M][N]: A @ W^T, filled by build()
    max_int: int = 0            # largest (|A| @ |W|^T) element, filled by build()


def row_scales(M, N):
    """Power-of-two scales that change with every row and every column, with different periods: a row / column swap or a shifted
    index shows."""
    return 2.0 ** ((torch.arange(M) % 31) - 15).float(), 2.0 ** (-(torch.arange(N) % 23)).float()


def operands(c, launch=0, lo=-8, hi=8):
    """The integer operands of launch `launch` of a case (the GPU test launches every case twice, on different data) from a
    seeded CPU generator; the cast to e4m3 is asserted lossless."""
    g = torch.Generator().manual_seed(2000 + 7 * c.seed + launch)
    a = torch.randint(lo, hi + 1, (c.M, c.K), generator=g).float()
    w = torch.randint(lo, hi + 1, (c.N, c.K), generator=g).float()
    aq, wq = a.to(E4), w.to(E4)
    assert torch.equal(aq.float(), a) and torch.equal(wq.float(), w), f"{c.name}: the e4m3 cast is not lossless"
    sa, sw = row_scales(c.M, c.N)
    bias = torch.randn(c.N, generator=g).to(BF)
    return Operands(a, w, aq, wq, sa, sw, bias)


def build(c, launch=0, device="cpu", lo=-8, hi=8):
    """Operands of a case on `device` with the exactness condition asserted and the integer product filled in."""
    o = operands(c, launch, lo, hi)
    for f in ("a", "w", "aq", "wq", "sa", "sw", "bias"):
        setattr(o, f, getattr(o, f).to(device))
    a64, w64 = o.a.double(), o.w.double()
    o.max_int = int((a64.abs() @ w64.abs().t()).max())
    assert o.max_int < EXACT_MAX, f"{c.name}: (|A| @ |W|^T).max() = {o.max_int} >= 2^24"
    o.isum = a64 @ w64.t()
    return o


# ------------------------------------------------------------------------------------------------ reference
SLIPS = {
    "k_tile_dropped": "one K-tile left out of the sum",
    "k_tile_stale": "one K-tile taken twice in place of its neighbour (a stale LDS buffer)",
    "segment_bound_off_by_one": "a split segment ends one K-tile late: that K-tile is counted by two segments",
    "reducer_adds_own_registers": "the S > 2 reducer adds the slabs to its own registers: its segment is counted twice",
    "previous_launch_slabs": "a segment's slab of the previous launch added in place of this launch's",
    "s_a_m_plus_1": "row m scaled by s_a[m + 1]",
    "s_w_n_plus_4": "column n scaled by s_w[n + 4]",
    "gate_without_row_offset": "the gate frame taken from m, not from row_offset + m",
    "padding_column_read": "a padding column of A read as data",
}
ROWS, TENSOR = "rows", "tensor"        # the per-row and the per-tensor kernel


def tile_product(o, kt0, kt1):
    """Integer product over the K-tiles [kt0, kt1)."""
    return o.a[:, kt0 * BK:kt1 * BK].double() @ o.w[:, kt0 * BK:kt1 * BK].double().t()


def integer_sum(c, o, slip=None, previous=None):
    """The integer sums a kernel with the named slip would hand to its de-quantise step.  `previous`: the operands of the launch
    before this one (previous_launch_slabs)."""
    nk = c.nk
    S = c.plan[1]
    segs = segments(nk, S)
    if slip == "k_tile_dropped":
        return o.isum - tile_product(o, nk - 1, nk)
    if slip == "k_tile_stale":                               # the last K-tile's LDS buffer still holds its predecessor
        assert nk >= 2
        return o.isum - tile_product(o, nk - 1, nk) + tile_product(o, nk - 2, nk - 1)
    if slip == "segment_bound_off_by_one":
        assert S > 1
        return o.isum + tile_product(o, segs[0][1], segs[0][1] + 1)
    if slip == "reducer_adds_own_registers":
        assert S > 2
        return o.isum + tile_product(o, *segs[S - 1])
    if slip == "previous_launch_slabs":
        assert S > 1 and previous is not None
        return o.isum - tile_product(o, *segs[0]) + tile_product(previous, *segs[0])
    if slip == "padding_column_read":                        # the K window of A starts one byte late: its last column is padding
        nan = torch.full_like(o.isum[:, :1], float("nan"))
        return o.isum + nan
    return o.isum


def _shifted(s, by):
    """s[min(i + by, n - 1)]"""
    i = (torch.arange(s.numel(), device=s.device) + by).clamp(max=s.numel() - 1)
    return s[i]


def reference(c, o, kernel, use_bias=False, slip=None, previous=None):
    """Expected bf16 output [M][N] of a case through `kernel` (ROWS: the varying scales, TENSOR: S_X and S_W), the scaled sum
    asserted representable in fp32."""
    isum = integer_sum(c, o, slip, previous)
    if kernel == ROWS:
        sa = _shifted(o.sa, 1) if slip == "s_a_m_plus_1" else o.sa
        sw = _shifted(o.sw, 4) if slip == "s_w_n_plus_4" else o.sw
        exact = isum * sa.double().reshape(-1, 1) * sw.double().reshape(1, -1)
    else:
        exact = isum * (S_X * S_W)
    y = exact.float()
    if slip != "padding_column_read":
        assert torch.equal(y.double(), exact), f"{c.name}: the scaled sum is not representable in fp32"
    if use_bias:
        y = y + o.bias.float()
    return y.to(BF)


def covering_slips(c, kernel):
    """The named slips whose effect the case must show through `kernel`."""
    s = ["k_tile_dropped"]
    if c.nk >= 2:
        s.append("k_tile_stale")
    if c.plan[1] > 1:
        s += ["segment_bound_off_by_one", "previous_launch_slabs"]
    if c.plan[1] > 2:
        s.append("reducer_adds_own_registers")
    if kernel == ROWS:
        if c.M > 1:
            s.append("s_a_m_plus_1")
        s.append("s_w_n_plus_4")
    if c in STRIDED_CASES:
        s.append("padding_column_read")
    return s


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def mismatches(got, ref):
    """Number of elements whose bit patterns differ."""
    return int((bits(got) != bits(ref.to(got.device))).sum())


# ------------------------------------------------------------------------------------------------ guarded strided layout
def guarded_operand(q, pad, device):
    """An e4m3 matrix as a view into a larger buffer: `pad` padding columns behind every row and GUARD_ROWS rows in front of and
    behind the matrix, all holding the NaN code - a read outside the K range or outside the rows makes the output NaN, it does not
    fault.  Returns (buffer, view)."""
    rows, K = q.shape
    buf = torch.full((rows + 2 * GUARD_ROWS, K + pad), NAN_CODE, dtype=torch.uint8)
    buf[GUARD_ROWS:GUARD_ROWS + rows, :K] = q.cpu().view(torch.uint8)
    buf = buf.to(device).view(E4)
    return buf, buf[GUARD_ROWS:GUARD_ROWS + rows, :K]


def guarded_output(M, N, device, offset=8):
    """A bf16 output as a column slice between guard columns of GUARD_OUT.  offset = 8: rows and first element 16-byte aligned
    (the store through LDS); offset = 4: every row 8 bytes off 16-byte alignment (the direct store).  Returns (buffer, view)."""
    buf = torch.full((M, N + 2 * offset), GUARD_OUT, dtype=BF, device=device)
    return buf, buf[:, offset:offset + N]


def guards_changed(buf, view_cols, offset):
    """Number of guard elements of a guarded_output buffer that no longer hold GUARD_OUT."""
    g = torch.cat([buf[:, :offset], buf[:, offset + view_cols:]], 1)
    return int((g != GUARD_OUT).sum())


# ------------------------------------------------------------------------------------------------ epilogue case
EPI_M, EPI_N, EPI_K, EPI_RPF = 300, 264, 128, 101      # tests/test_gemm_mfma_shape_gpu.py: _epilogue_problem


def gelu_safe_bias(n, seed):
    """(bias, bf16(gelu(bias))) on the GPU: _gelu_safe_bias of tests/test_gemm_mfma_shape_gpu.py, imported where it is used (that
    module needs pytest and places its tensors on the device)."""
    import test_gemm_mfma_shape_gpu as shape
    return shape._gelu_safe_bias(n, seed)


def epilogue_problem(device="cpu"):
    """All A codes zero, W random codes without the two NaN codes: the accumulators are zero and the output is the epilogue chain
    alone, y = bf16(acc + bias); y = bf16(act(y)); t = bf16(y * gate); out = bf16(res + t).  Frame boundaries (101, 202) lie inside
    a 32-row block; the last column tile holds 8 columns.  The GELU operands are added by the GPU test (gelu_safe_bias)."""
    M, N, K, rpf = EPI_M, EPI_N, EPI_K, EPI_RPF
    g = torch.Generator().manual_seed(77)
    wc = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    wc = wc.masked_fill((wc & 0x7F) == NAN_CODE, 0)
    bias = torch.randn(N, generator=g).to(BF)
    gate = torch.randn(3, N, generator=g).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    sa, sw = row_scales(M, N)
    p = dict(M=M, N=N, K=K, rpf=rpf, aq=torch.zeros(M, K, dtype=torch.uint8).view(E4), wq=wc.view(E4), sa=sa, sw=sw, bias=bias,
             gate=gate, res=res)
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in p.items()}


def epilogue_reference(p, rows=None, row_offset=0, slip=None):
    """bf16(res + bf16(bias * gate[frame of row_offset + m])) on the first `rows` rows (products of two bf16 are exact in fp32)."""
    rows = p["M"] if rows is None else rows
    m = torch.arange(rows, device=p["bias"].device)
    frame = (m if slip == "gate_without_row_offset" else m + row_offset) // p["rpf"]
    t = (p["bias"].float()[None, :] * p["gate"].float()[frame]).to(BF)
    return (p["res"][:rows].float() + t.float()).to(BF)


# ------------------------------------------------------------------------------------------------ quantiser
FP8_MAX = 448.0
QUANT_WIDTH = 272                       # a multiple of 16; column 0 of every row holds 448
# (M, d, ld = ldq): one chunk; three rows of chunks; the widest row (1728 chunks over 256 threads); more rows than the 1024
# workgroups of the grid, twice over; strided with rows 1024 and up in the second trip of the row loops
QUANT_SHAPES = [(1, 16, 16), (5, 48, 48), (3, 13824, 13824), (2050, 16, 16), (1500, 272, 280)]
QUANT_PAD_IN = 3e38                     # input padding columns: a read outside d changes the scale
QUANT_PAD_OUT = 0x55                    # output padding bytes


def quant_peaks(M, d):
    """(name, row, column) of the places the single maximum is put at in turn."""
    p = [("first", 0, 0), ("last", M - 1, d - 1)]
    if M > 1024:
        p.append(("row_1024", 1024, 0))
    return p


def all_bf16_values():
    """Every finite bf16 value with |x| <= 448, in bit-pattern order: 34754 values, both zeros and the subnormals included."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    keep = torch.isfinite(v) & (v.float().abs() <= FP8_MAX)
    return v[keep]


def quant_all_values(e=0):
    """bf16 [129][272] = 2^e times: column 0 of every row 448 (so every ROW has the scale 2^e as well), then every finite bf16
    value of magnitude <= 448, then zeros.  Since 448 * fp32(1 / 448) == 1.0f the scale is exactly 2^e, x / s is exact and the
    expected code is torch's own round-to-nearest-even cast of the value: every tie, subnormal, flush to zero, signed zero and the
    saturation point are present.  Asserted for e = 0: all 254 non-NaN codes occur."""
    vals = all_bf16_values()
    assert vals.numel() == 34754
    per_row = QUANT_WIDTH - 1
    rows = -(-vals.numel() // per_row)
    body = torch.zeros(rows * per_row, dtype=BF)
    body[:vals.numel()] = vals
    x = torch.cat([torch.full((rows, 1), FP8_MAX, dtype=BF), body.reshape(rows, per_row)], 1)
    inv = torch.tensor(1.0) / torch.tensor(FP8_MAX)
    assert float(torch.tensor(FP8_MAX) * inv) == 1.0
    if e == 0:
        codes = x.float().to(E4).view(torch.uint8)
        assert torch.unique(codes).numel() == 254 and not bool(((codes & 0x7F) == NAN_CODE).any())
    x = (x.float() * 2.0 ** e).to(BF)
    assert float(x.float().abs().max()) == FP8_MAX * 2.0 ** e
    return x


def quant_shape_data(M, d, ld, peak_row, peak_col, e, sign):
    """bf16 [M][ld]: Gaussian data of magnitude below 400 * 2^e in the first d columns, QUANT_PAD_IN in the padding columns, and
    one element sign * 448 * 2^e at (peak_row, peak_col): the scale is exactly 2^e if and only if that element is seen and
    nothing outside the d columns is."""
    g = torch.Generator().manual_seed(M + d + 3 * peak_row + peak_col)
    x = (torch.randn(M, ld, generator=g) * 100).clamp(-400, 400) * 2.0 ** e
    x[:, d:] = QUANT_PAD_IN
    x[peak_row, peak_col] = sign * FP8_MAX * 2.0 ** e
    x = x.to(BF)
    assert int((x[:, :d].float().abs() == FP8_MAX * 2.0 ** e).sum()) == 1
    return x


def quantize_tensor_restated(x):
    """The per-tensor restatement on the data's device: s = amax.clamp(min=1e-12) * fp32(1 / 448), q = e4m3(clamp(x / s, +-448)).
    -> (codes as float8_e4m3fn, scale as a 1-element float32 tensor)."""
    inv = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(FP8_MAX, dtype=torch.float32)).to(x.device)
    s = x.float().abs().max().clamp(min=1e-12) * inv
    return (x.float() / s).clamp(-FP8_MAX, FP8_MAX).to(E4), s.reshape(1)
