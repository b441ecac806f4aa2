"""Bit-exact cases for the convolution kernels of csrc/vae_conv.hip (rtv_conv_cl, rtv_conv_cl_win, rtv_conv3_norm_silu_cl) and
the layer kernels of csrc/taehv.hip (rtv_taehv_conv, rtv_taehv_enc_conv): cases, integer operands, a plain reference, named
slips and the guarded device layout.  No GPU and no pytest in here; tests/test_conv_exact_cpu.py proves that the acceptance
would notice each slip, tests/test_conv_exact_gpu.py holds the kernels to it.

Why integers: activations and weights are iid in {-1, 0, 1}, the bias an integer in [-8, 8], the residual an integer in
[-64, 64] (all times a power-of-two `unit` where a case needs outputs inside (-1, 1)).  Every product and every partial sum
is then an integer multiple of the unit of at most 2048 units - exact in fp32 in ANY summation order and exact in fp16 at
every rounding point of the epilogue - so the expected output is known bit for bit for every kernel form and no tolerance is
involved.  build() asserts that condition for every case instead of assuming it.

Not observable with such data, and therefore not among the slips: the ORDER of the fp16 roundings in the epilogue
(f16(f16(acc + bias) + residual) against f16(acc + bias + residual)), the fp32 summation order of the taps, and an fp16 instead
of an fp32 accumulator - every intermediate is exact either way.  The Gaussian tests of tests/test_vae_gpu.py and
tests/test_taehv_gpu.py cover those."""
import dataclasses

import torch

NONE, UPSAMPLE2X, DOWN2X, TIME_DOWN2X, GATHER = 0, 1, 2, 3, 16     # include/rtv_hip.h: `resample` of rtv_conv_cl
TILE_H, TILE_W = 16, 32                                            # pixel tile of the halo kernels
EXACT_MAX = 2048                                                   # |integers| up to 2048 are exact in fp16
GUARD_IN = 1024.0                                                  # value of the input guard slices
GUARD_ROWS = 64                                                    # NaN rows in front of and behind an output


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    api: str                    # conv_cl | conv_win | norm_silu | taehv | taehv_enc
    Cin: int
    Cout: int
    T: int
    H: int                      # OUTPUT grid
    W: int
    kt: int = 3
    kh: int = 3
    kw: int = 3
    resample: int = NONE        # conv_cl / conv_win
    n_split: int = 0
    epilogues: tuple = ((True, False),)      # (bias, residual) pairs the GPU test runs
    window: tuple = None        # conv_win: (y_out0, y_in0, in_rows, img_rows); H is then the stripe's rows
    narrow: bool = False        # output is a column slice: out_ld = Cout + 4
    ups: int = 0                # taehv
    relu: int = 0
    head: int = 0
    zero_state: bool = False    # taehv kt = 2: slice 0 all zero
    form: int = -1              # taehv_enc
    n_total: int = 0
    n0: int = 0
    unit: float = 1.0           # power of two: weights and bias are integers times `unit`
    seed: int = 0
    big: bool = False           # reference too large for a CPU slip proof: exactness is checked where the GPU test runs

    @property
    def taps(self):
        return self.kt * self.kh * self.kw


ALL3 = ((True, True), (False, False), (True, False))


def _halo(Cin, Cout, T, H, W, **k):
    return Case(f"halo_{Cin}_{Cout}_{T}x{H}x{W}", "conv_cl", Cin, Cout, T, H, W, epilogues=ALL3, seed=Cin + Cout + H, **k)


HALO_CASES = [_halo(96, 96, 2, 33, 70),            # ragged on both axes
              _halo(32, 96, 1, 16, 32),            # one chunk per slice, exactly one tile
              _halo(192, 384, 3, 17, 31),          # four filter tiles
              _halo(384, 192, 1, 48, 64),          # twelve chunks
              _halo(96, 192, 4, 5, 100)]           # fewer rows than a tile
# 13 x 11 tiles x 2 frames = 286 tiles on 256 CUs: several tiles per persistent workgroup
MANY_TILES = dataclasses.replace(_halo(96, 96, 2, 200, 330), name="halo_many_tiles_96_96_2x200x330", big=True)


def _ups(Cin, Cout, T, h, w):
    return Case(f"ups_{Cin}_{Cout}_{T}x{h}x{w}", "conv_cl", Cin, Cout, T, 2 * h, 2 * w, kt=1, resample=UPSAMPLE2X, seed=Cin + h)


UPS_CASES = [_ups(384, 192, 1, 17, 23), _ups(192, 96, 3, 33, 70)]

GATHER_CASES = [
    Case("gather_cout8_96_8", "conv_cl", 96, 8, 1, 8, 12, epilogues=ALL3, seed=1),
    Case("gather_flag_96_96", "conv_cl", 96, 96, 1, 8, 12, resample=GATHER, epilogues=ALL3, seed=2),
    Case("gather_32_384", "conv_cl", 32, 384, 1, 8, 12, epilogues=ALL3, seed=3),
    Case("gather_flag_192_192", "conv_cl", 192, 192, 4, 16, 24, resample=GATHER, epilogues=ALL3, seed=4),
    Case("shortcut_1x1x1_96_192", "conv_cl", 96, 192, 2, 8, 12, kt=1, kh=1, kw=1, seed=5),
]
TIME_CONV = Case("time_conv_split_384_768", "conv_cl", 384, 768, 2, 6, 10, kt=3, kh=1, kw=1, n_split=384, seed=6)
DOWN_CASES = [
    Case("down2x_96", "conv_cl", 96, 96, 2, 9, 13, kt=1, resample=DOWN2X, seed=7),
    Case("down2x_384", "conv_cl", 384, 384, 1, 8, 12, kt=1, resample=DOWN2X, seed=8),
    Case("time_down2x_192", "conv_cl", 192, 192, 2, 6, 8, kh=1, kw=1, resample=TIME_DOWN2X, seed=9),
    Case("time_down2x_384", "conv_cl", 384, 384, 1, 6, 8, kh=1, kw=1, resample=TIME_DOWN2X, seed=10),
]
NARROW_CASES = [
    Case("narrow_halo_shape_96_96", "conv_cl", 96, 96, 2, 17, 35, epilogues=((True, True),), narrow=True, seed=11),
    Case("narrow_gather_32_128", "conv_cl", 32, 128, 1, 8, 12, epilogues=((True, True),), narrow=True, seed=12),
]
NORM_CASES = [Case("norm_silu_96_2x33x70", "norm_silu", 96, 96, 2, 33, 70, seed=13),
              Case("norm_silu_384_1x5x9", "norm_silu", 384, 96, 1, 5, 9, seed=14)]

# the row-window layer: the stage 2 -> 3 transition of the decoder (nearest 2x + 3x3, 192 -> 96) at latent size 8 x 5
WIN_LATENT_H, WIN_LATENT_W, WIN_T = 8, 5, 2
WIN_WHOLE = Case("win_whole_192_96", "conv_cl", 192, 96, WIN_T, 8 * WIN_LATENT_H, 8 * WIN_LATENT_W, kt=1, resample=UPSAMPLE2X,
                 seed=15)
WIN_WORLDS = (2, 3)


def window_plan(world, rank, h=WIN_LATENT_H, w=WIN_LATENT_W):
    """(y_out0, y_in0, in_rows, img_rows, H) of the stage 2 -> 3 rtv_conv_cl_win call that rank `rank` of a `world`-way
    row-sharded decode issues, from the code that derives them: VAEDecoderWrapper.row_range for the pixel stripe and the
    library's row plan as rtv_vae_cache_slot_rows reports it (cache slots 19 / 25 live at stages 2 / 3; host code only)."""
    import ctypes
    from realtime_video_amd import _lib
    from realtime_video_amd.vae_decoder import VAEDecoderWrapper
    r0, r1 = VAEDecoderWrapper("cpu", row_shard=(rank, world)).row_range(h)

    def stage(slot):
        off, C, H, W, first = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.call("rtv_vae_cache_slot_rows", h, w, r0, r1, slot, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H),
                  ctypes.byref(W), ctypes.byref(first))
        return first.value, H.value, W.value, C.value

    a2, rows2, w2, c2 = stage(19)
    a3, rows3, w3, c3 = stage(25)
    assert (w2, c2, w3, c3) == (4 * w, 192, 8 * w, 96)
    return a3, a2, rows2, 8 * h, rows3


def window_case(world, rank):
    """The stripe of rank `rank` of a `world`-way sharded decode as a Case (needs the built library: window_plan)."""
    y_out0, y_in0, in_rows, img_rows, H = window_plan(world, rank)
    return dataclasses.replace(WIN_WHOLE, name=f"win_world{world}_rank{rank}", api="conv_win", H=H,
                               window=(y_out0, y_in0, in_rows, img_rows))


WINDOWS = [(world, rank) for world in WIN_WORLDS for rank in range(world)]


def window_cases():
    return [window_case(world, rank) for world, rank in WINDOWS]


# rtv_taehv_conv: the eight FORMS of tests/test_taehv_gpu.py
# name, T, H, W, Cin, Cout, kt, ups, n_split, relu, residual, bias, head
_TAEHV_FORMS = [
    ("plain_relu_64", 2, 13, 21, 64, 64, 1, 0, 0, 1, False, True, False),
    ("memblock_window_zero_state", 3, 11, 9, 128, 128, 2, 0, 0, 1, False, True, False),
    ("memblock_window_state", 3, 11, 9, 128, 128, 2, 0, 0, 1, False, True, False),
    ("residual_relu_256", 2, 7, 11, 256, 256, 1, 0, 0, 1, True, True, False),
    ("upsample_fold_256_128", 2, 14, 22, 256, 128, 1, 1, 0, 0, False, False, False),
    ("upsample_fold_split_128", 2, 14, 18, 128, 128, 1, 1, 64, 0, False, False, False),
    ("upsample_fold_split_64_relu", 1, 26, 30, 64, 128, 1, 1, 64, 1, False, False, False),
    ("head_2y_minus_1", 3, 19, 23, 64, 8, 1, 0, 0, 0, False, True, True),
]
TAEHV_CASES = [Case("taehv_" + n, "taehv", Cin, Cout, T, H, W, kt=kt, ups=ups, n_split=ns, relu=relu, head=int(head),
                    epilogues=((bias, res),), zero_state=n.endswith("zero_state"), unit=1 / 64 if head else 1.0, seed=20 + i)
               for i, (n, T, H, W, Cin, Cout, kt, ups, ns, relu, res, bias, head) in enumerate(_TAEHV_FORMS)]
TAEHV_ENC_CASES = [
    Case("taehv_enc_first_layer", "taehv_enc", 3, 64, 2, 13, 21, kt=1, form=0, relu=1, n_total=4, n0=1, unit=0.5, seed=30),
    Case("taehv_enc_stride2_kt1", "taehv_enc", 64, 64, 2, 7, 11, kt=1, form=1, epilogues=((False, False),), seed=31),
    Case("taehv_enc_stride2_kt2", "taehv_enc", 64, 64, 2, 7, 11, kt=2, form=1, epilogues=((False, False),), seed=32),
    Case("taehv_enc_latent_head", "taehv_enc", 64, 16, 3, 9, 13, kt=1, form=2, n_total=6, n0=2, seed=33),
]

# every case that needs no built library to be enumerated (the row-window stripes come from window_cases())
STATIC_CASES = (HALO_CASES + [MANY_TILES] + UPS_CASES + GATHER_CASES + [TIME_CONV] + DOWN_CASES + NARROW_CASES + NORM_CASES
                + [WIN_WHOLE] + TAEHV_CASES + TAEHV_ENC_CASES)
CLAMP_CASES = [c for c in TAEHV_CASES if c.head]


# ------------------------------------------------------------------------------------------------ operands
@dataclasses.dataclass
class Operands:
    x: torch.Tensor             # fp16 channels-last [Tin][inH][inW][Cin]; taehv_enc form 0: planar [3][n_total][H][W]
    w: torch.Tensor             # fp16 [Cout][taps][Cin]; taehv_enc form 0: [64][32], tap c * 9 + dy * 3 + dx
    bias: torch.Tensor          # fp16 [Cout] (always built; a run may leave it out)
    res: torch.Tensor           # fp16 [T][H][W][Cout]
    gamma: torch.Tensor = None  # norm_silu
    max_int: int = 0            # largest |conv + bias + residual| in units, filled by build()


def in_dims(c):
    """(Tin, inH, inW) of the input buffer."""
    if c.api == "taehv":
        return c.T + c.kt - 1, c.H >> c.ups, c.W >> c.ups
    if c.api == "taehv_enc":
        return (c.T * c.kt, 2 * c.H, 2 * c.W) if c.form == 1 else (c.T, c.H, c.W)
    r = c.resample & ~GATHER
    Tin = 2 * c.T + 1 if r == TIME_DOWN2X else c.T + c.kt - 1
    if c.window:
        return Tin, c.window[2], c.W // 2
    if r == UPSAMPLE2X:
        return Tin, c.H // 2, c.W // 2
    if r == DOWN2X:
        return Tin, 2 * c.H, 2 * c.W
    return Tin, c.H, c.W


def _tern(shape, g):
    return torch.randint(-1, 2, shape, generator=g).to(torch.float32)


def operands(c):
    """The integer operands of a case from a seeded CPU generator.  A row-window stripe shares the whole image's operands
    (same seed): its input is the rows [y_in0, y_in0 + in_rows) of the whole input."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    Tin, inH, inW = in_dims(dataclasses.replace(c, window=None, H=c.window[3]) if c.window else c)
    if c.api == "taehv_enc" and c.form == 0:
        x = torch.full((3, c.n_total, c.H, c.W), GUARD_IN)                      # frames outside n0 .. n0 + T are guards
        x[:, c.n0:c.n0 + c.T] = _tern((3, c.T, c.H, c.W), g)
        w = torch.cat([_tern((64, 27), g), torch.zeros(64, 5)], 1)
    else:
        x = _tern((Tin, inH, inW, c.Cin), g)
        if c.zero_state:
            x[0] = 0
        w = _tern((c.Cout, c.taps, c.Cin), g) * c.unit
    if c.head:
        w[3:] = 0                                                                # filters padded 3 -> 8
    bias = torch.randint(-8, 9, (c.Cout,), generator=g).float() * c.unit
    if c.head:
        bias = bias + 0.5                                                        # centre conv + bias in (0, 1)
        bias[3:] = 0
    full_H = c.window[3] if c.window else c.H
    res = torch.randint(-64, 65, (c.T, full_H, c.W, c.Cout), generator=g).float() * c.unit
    gamma = (1.0 + 0.2 * torch.randn(c.Cout, generator=g)).half() if c.api == "norm_silu" else None
    if c.window:
        y_out0, y_in0, in_rows, _ = c.window
        x = x[:, y_in0:y_in0 + in_rows]
        res = res[:, y_out0:y_out0 + c.H]
    return Operands(x.half().contiguous(), w.half().contiguous(), bias.half(), res.half().contiguous(), gamma)


# ------------------------------------------------------------------------------------------------ reference
SLIPS = {
    "dx_mirrored": "tap column dx read at 2 - dx",
    "dy_dx_exchanged": "tap (dy, dx) read at (dx, dy)",
    "time_taps_reversed": "time tap dt reads slice kt - 1 - dt",
    "pad_edge_clamp": "zero padding replaced by the clamped edge pixel",
    "pad_flat_neighbour": "zero padding replaced by the flat-address neighbour (x = -1: previous row's last pixel)",
    "seam_column": "column 32k of a 16 x 32 tile reads inside its own tile",
    "seam_row": "row 16k of a 16 x 32 tile reads inside its own tile",
    "last_chunk_dropped": "the last 32-channel chunk of the last tap is left out",
    "last_chunk_twice": "the last 32-channel chunk of the last tap is added twice",
    "ups_parity_rows": "upsampling source row (y >> 1) + dy - 1 instead of (y + dy - 1) >> 1",
    "ups_parity_cols": "upsampling source column (x >> 1) + dx - 1 instead of (x + dx - 1) >> 1",
    "split_halves_exchanged": "n_split halves written to frames 2t + 1 and 2t",
    "down2x_pad_low": "RTV_CONV_DOWN2X zero padding on the low side",
    "time_down2x_early": "RTV_CONV_TIME_DOWN2X window starts at 2t - 1",
    "bias_n_plus_4": "filter n gets the bias of filter n + 4",
    "residual_neighbour": "pixel p gets the residual of pixel p + 1",
    "window_y_in0_off_by_one": "row window: input buffer row 0 taken for image row y_in0 + 1",
    "taehv_kt2_halves_exchanged": "TAEHV kt = 2: taps 0-8 read slice t + 1, taps 9-17 slice t",
    "taehv_head_without_affine": "TAEHV head clamps conv + bias without the 2y - 1",
}


def _axis(n_out, n_buf, d, *, stride, pad, ups, off_out, off_in, lim, slip_parity, clamp_pad, seam, unbounded):
    """Source index into the input buffer and validity, per output coordinate, for tap offset d along one spatial axis."""
    o = torch.arange(n_out)
    if ups and slip_parity:
        s = ((off_out + o) >> 1) + d - 1                     # the slip: shift in SOURCE resolution
        valid = (s >= 0) & (s < (lim >> 1))
        return (s - off_in).clamp(0, n_buf - 1), valid
    u = (off_out + o) * stride + d - pad                     # image coordinate the tap reads (upsampled resolution if ups)
    if seam:                                                 # stay inside the output tile of o (tiles count from the buffer's row 0)
        lo = (o // seam) * seam + off_out
        inside = (u >= 0) & (u < lim)
        u = torch.where(inside, torch.minimum(torch.maximum(u, lo), lo + seam - 1), u)
    if clamp_pad:
        u = u.clamp(0, lim - 1)
    valid = (u >= 0) & (u < lim)
    s = ((u >> 1) if ups else u) - off_in
    if unbounded:
        return s, valid
    return s.clamp(0, n_buf - 1), valid


def conv_taps(x, w, T, H, W, kt, kh, kw, *, st=1, sy=1, pad_h=None, pad_w=None, ups=0, window=None, t_first=0, slip=None,
              dtype=torch.float32):
    """sum over taps of (shifted slice of x) [pixels x Cin] @ (w[:, tap, :])^T [Cin x Cout], written out: no convolution library
    call (no Winograd / FFT path can creep in).  x [Tin][inH][inW][Cin], w [Cout][kt * kh * kw][Cin] -> [T][H][W][Cout] in
    `dtype`, on x's device.  Output frame t reads slices st * t + dt + t_first; output pixel (y, x) reads image pixel
    (sy * y + dy - pad_h, sy * x + dx - pad_w), zero outside the image; ups: the image is the nearest-2x upsampling of x,
    source ((y + dy - 1) >> 1, (x + dx - 1) >> 1); window = (y_out0, y_in0, in_rows, img_rows): output row 0 is image row
    y_out0, buffer row 0 is source row y_in0, the image has img_rows rows at output resolution."""
    Tin, inH, inW, Cin = x.shape
    Cout = w.shape[0]
    pad_h = kh >> 1 if pad_h is None else pad_h
    pad_w = kw >> 1 if pad_w is None else pad_w
    y_out0, y_in0, _, img_rows = window if window else (0, 0, inH, (inH << ups) if ups else inH)
    if slip == "window_y_in0_off_by_one":
        y_in0 += 1
    lim_w = (inW << ups) if ups else inW
    xf = x.to(dtype).reshape(Tin, inH * inW, Cin)
    wf = w.to(dtype)
    acc = torch.zeros(T, H * W, Cout, dtype=dtype, device=x.device)
    flat_pad = slip == "pad_flat_neighbour"
    for dt in range(kt):
        for dy in range(kh):
            for dx in range(kw):
                tap = (dt * kh + dy) * kw + dx
                sdt, sdy, sdx = dt, dy, dx
                if slip == "dx_mirrored":
                    sdx = kw - 1 - dx
                if slip == "dy_dx_exchanged":
                    sdy, sdx = dx, dy
                if slip in ("time_taps_reversed", "taehv_kt2_halves_exchanged"):
                    sdt = kt - 1 - dt
                ti = torch.arange(T) * st + sdt + t_first
                tv = (ti >= 0) & (ti < Tin)
                ry, vy = _axis(H, inH, sdy, stride=sy, pad=pad_h, ups=ups, off_out=y_out0, off_in=y_in0, lim=img_rows,
                               slip_parity=slip == "ups_parity_rows", clamp_pad=slip == "pad_edge_clamp",
                               seam=TILE_H if slip == "seam_row" else 0, unbounded=False)
                rx, vx = _axis(W, inW, sdx, stride=sy, pad=pad_w, ups=ups, off_out=0, off_in=0, lim=lim_w,
                               slip_parity=slip == "ups_parity_cols", clamp_pad=slip == "pad_edge_clamp",
                               seam=TILE_W if slip == "seam_column" else 0, unbounded=flat_pad)
                flat = ry[:, None] * inW + rx[None, :]
                mask = vy[:, None] & vx[None, :]
                if flat_pad:
                    mask = vy[:, None] & (flat >= 0) & (flat < inH * inW)
                flat = flat.clamp(0, inH * inW - 1).reshape(-1).to(x.device)
                keep = (mask.reshape(1, -1, 1) & tv.reshape(-1, 1, 1)).to(device=x.device, dtype=dtype)
                src = xf[ti.clamp(0, Tin - 1).to(x.device)][:, flat] * keep
                wt = wf[:, tap, :]
                if tap == kt * kh * kw - 1 and slip in ("last_chunk_dropped", "last_chunk_twice"):
                    wt = wt.clone()
                    wt[:, Cin - 32:] *= 0.0 if slip == "last_chunk_dropped" else 2.0
                acc += src @ wt.t()
    return acc.reshape(T, H, W, Cout)


def _f16(v):
    return v.half().to(v.dtype)


def _geometry(c):
    """Keyword arguments of conv_taps for a case."""
    if c.api == "taehv":
        return dict(ups=c.ups)
    if c.api == "taehv_enc":
        return dict(st=c.kt, sy=2) if c.form == 1 else {}
    r = c.resample & ~GATHER
    k = dict(ups=int(r == UPSAMPLE2X), window=c.window)
    if r == DOWN2X:
        k.update(sy=2, pad_h=0, pad_w=0)
    if r == TIME_DOWN2X:
        k.update(st=2)
    return k


def conv_sum(c, ops, slip=None, dtype=torch.float32, device=None):
    """The bare tap sum of a case, [T][H][W][Cout] in `dtype`."""
    x, w = ops.x, ops.w
    if device is not None:
        x, w = x.to(device), w.to(device)
    k = _geometry(c)
    if slip == "down2x_pad_low":
        k.update(pad_h=1, pad_w=1)
    if slip == "time_down2x_early":
        k.update(t_first=-1)
    if c.api == "taehv_enc" and c.form == 0:
        x01 = _f16(0.5 * x.float() + 0.5)[:, c.n0:c.n0 + c.T]                  # the kernel maps to [0, 1], rounds to fp16
        x = x01.permute(1, 2, 3, 0)                                              # [T][H][W][3]
        w = w[:, :27].reshape(64, 3, 9).permute(0, 2, 1)                         # [64][dy * 3 + dx][c]
        return conv_taps(x, w, c.T, c.H, c.W, 1, 3, 3, slip=slip, dtype=dtype)
    return conv_taps(x, w, c.T, c.H, c.W, c.kt, c.kh, c.kw, slip=slip, dtype=dtype, **k)


def _scatter(c, y, slip):
    if not c.n_split:
        return y
    a, b = y[..., :c.n_split], y[..., c.n_split:]
    if slip == "split_halves_exchanged":
        a, b = b, a
    return torch.stack([a, b], 1).reshape(2 * c.T, c.H, c.W, c.n_split)         # filter group s -> frame 2t + s


def reference(c, ops, use_bias=True, use_res=False, slip=None, dtype=torch.float32, device=None, acc=None):
    """Expected output of a case.  conv_cl / conv_win: fp16 [T or 2T][H][W][Cout or n_split] = f16(f16(acc + bias) + residual),
    the kernel's rounding points.  norm_silu: the fp16 conv + bias the norm is taken of.  taehv: fp16 ReLU / residual forms,
    head float32 [T][3][H][W] = clamp(2 * (acc + bias) - 1, -1, 1).  taehv_enc: fp16 [T][H][W][64], form 2 planar
    [16][n_total][H][W] with NaN in the frames the call does not write.  `acc` = a conv_sum() to reuse."""
    acc = conv_sum(c, ops, slip, dtype, device) if acc is None else acc
    dev = acc.device
    v = acc
    if use_bias:
        b = ops.bias.to(dev).to(dtype)
        v = v + (b.roll(-4) if slip == "bias_n_plus_4" else b)
    if use_res:
        r = ops.res.to(dev).to(dtype)
        if slip == "residual_neighbour":
            r = r.reshape(-1, c.Cout).roll(-1, 0).reshape(r.shape)
    if c.api in ("conv_cl", "conv_win", "norm_silu"):
        v = _f16(v)
        if use_res:
            v = _f16(v + r)
        return _scatter(c, v, slip).half()
    if c.api == "taehv":
        if c.head:
            y = v if slip == "taehv_head_without_affine" else 2 * v - 1
            return y.clamp(-1, 1)[..., :3].permute(0, 3, 1, 2).float().contiguous()
        if use_res:
            v = torch.relu(v + r)
        elif c.relu:
            v = torch.relu(v)
        return _scatter(c, v, slip).half()
    if c.form == 2:
        out = torch.full((16, c.n_total, c.H, c.W), float("nan"), dtype=torch.float16, device=dev)
        out[:, c.n0:c.n0 + c.T] = v.half().permute(3, 0, 1, 2)
        return out
    return (torch.relu(v) if c.relu else v).half()


def _assert_units(v, unit, what, name):
    u = v.double() / unit
    assert bool((u == u.round()).all()), f"{name}: {what} is not a whole number of units"
    m = float(u.abs().max())
    assert m <= EXACT_MAX, f"{name}: max |{what}| = {m} units > {EXACT_MAX}"
    return int(m)


def build(c, device=None, check64=True):
    """Operands and the bare tap sum of a case, with the exactness condition asserted: conv, conv + bias and
    conv + bias + residual are whole numbers of units of at most 2048, and the float32 tap sum equals the float64 one.
    device: where the tap loop runs (exact for integers wherever it runs); check64 = False leaves the float64 evaluation to
    the caller (the one case whose reference is evaluated on the GPU cross-checks a subsample)."""
    ops = operands(c)
    acc = conv_sum(c, ops, device=device)
    if check64:
        acc64 = conv_sum(c, ops, dtype=torch.float64, device=device)
        assert torch.equal(acc.double(), acc64), f"{c.name}: the float32 tap sum differs from the float64 one"
    unit = c.unit
    b = ops.bias.to(acc.device).float()
    m = [_assert_units(acc, unit, "conv", c.name), _assert_units(acc + b, unit, "conv + bias", c.name)]
    if ops.res.shape == acc.shape:
        m.append(_assert_units(acc + b + ops.res.to(acc.device).float(), unit, "conv + bias + residual", c.name))
    ops.max_int = max(m)
    return ops, acc


# ------------------------------------------------------------------------------------------------ which slip a case can see
def covering_slips(c):
    """The named slips whose effect a case must show (tests/test_conv_exact_cpu.py: at least 10 changed outputs each)."""
    s = []
    r = c.resample & ~GATHER
    has_bias = any(b for b, _ in c.epilogues)
    has_res = any(rr for _, rr in c.epilogues)
    if c.kh == 3:
        s += ["dx_mirrored", "dy_dx_exchanged"]
        if r != DOWN2X and not (c.api == "taehv_enc" and c.form == 1):
            s += ["pad_edge_clamp", "pad_flat_neighbour"]
        stride1 = r != DOWN2X and not (c.api == "taehv_enc" and c.form == 1)
        if stride1 and c.W > TILE_W:
            s.append("seam_column")
        # a stripe that starts at an odd image row has its tile seams between the two copies of one source row: the nearest-2x
        # upsampling makes the slip a no-op there, by construction
        if stride1 and c.H > TILE_H and not (c.window and c.window[0] % 2):
            s.append("seam_row")
    if c.kt > 1 and c.api in ("conv_cl", "conv_win", "norm_silu") and not c.zero_state:
        s.append("time_taps_reversed")
    if c.Cin >= 32:
        s += ["last_chunk_dropped", "last_chunk_twice"]
    if (r == UPSAMPLE2X and c.api in ("conv_cl", "conv_win")) or c.ups:
        s += ["ups_parity_rows", "ups_parity_cols"]
    if c.n_split:
        s.append("split_halves_exchanged")
    if r == DOWN2X:
        s.append("down2x_pad_low")
    if r == TIME_DOWN2X:
        s.append("time_down2x_early")
    if has_bias:
        s.append("bias_n_plus_4")
    if has_res:
        s.append("residual_neighbour")
    if c.window:
        s.append("window_y_in0_off_by_one")
    if c.api in ("taehv", "taehv_enc") and c.kt == 2 and not c.zero_state:
        s.append("taehv_kt2_halves_exchanged")
    if c.head:
        s.append("taehv_head_without_affine")
    return s


# ------------------------------------------------------------------------------------------------ guarded device layout
@dataclasses.dataclass
class Layout:
    x_buf: torch.Tensor         # the allocation that holds the input between guard slices of GUARD_IN
    x: torch.Tensor             # view: what the kernel is given
    w: torch.Tensor
    bias: torch.Tensor
    res: torch.Tensor
    gamma: torch.Tensor
    out_buf: torch.Tensor       # NaN everywhere; the kernel writes into `out`
    out: torch.Tensor           # view: first element = the output pointer
    out_ld: int
    res_ld: int


def lay_out(c, ops, device):
    """Place a case on `device`: the input between two guard slices of 1024, the output pre-filled with NaN inside a larger
    NaN buffer (GUARD_ROWS rows in front and behind; the narrow case also 4 guard columns per row).  The guards are part of
    live allocations: a kernel that strays by a row or a slice reads 1024s or overwrites NaNs, it does not fault."""
    x = ops.x
    if c.api == "taehv_enc" and c.form == 0:
        x_buf = torch.full((x.numel() + 128,), GUARD_IN, dtype=torch.float16)
        x_buf[64:64 + x.numel()] = x.reshape(-1)
        x_buf = x_buf.to(device)
        xv = x_buf[64:64 + x.numel()].view(x.shape)
    else:
        x_buf = torch.full((x.shape[0] + 2,) + tuple(x.shape[1:]), GUARD_IN, dtype=torch.float16)
        x_buf[1:-1] = x
        x_buf = x_buf.to(device)
        xv = x_buf[1:-1]
    nan = float("nan")
    if c.head:
        n = c.T * 3 * c.H * c.W
        out_buf = torch.full((n + 2 * GUARD_ROWS,), nan, dtype=torch.float32, device=device)
        out, out_ld = out_buf[GUARD_ROWS:GUARD_ROWS + n].view(c.T, 3, c.H, c.W), 0
    elif c.api == "taehv_enc" and c.form == 2:
        n = 16 * c.n_total * c.H * c.W
        out_buf = torch.full((n + 2 * GUARD_ROWS,), nan, dtype=torch.float16, device=device)
        out, out_ld = out_buf[GUARD_ROWS:GUARD_ROWS + n].view(16, c.n_total, c.H, c.W), 0
    else:
        frames = 2 * c.T if c.n_split else c.T
        ch = c.n_split or c.Cout
        out_ld = ch + 4 if c.narrow else ch
        rows = frames * c.H * c.W
        out_buf = torch.full((rows + 2 * GUARD_ROWS, out_ld), nan, dtype=torch.float16, device=device)
        out = out_buf[GUARD_ROWS:GUARD_ROWS + rows, :ch]
    return Layout(x_buf, xv, ops.w.to(device), ops.bias.to(device), ops.res.to(device),
                  ops.gamma.to(device) if ops.gamma is not None else None, out_buf, out, out_ld, c.Cout)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def expected_buffer(c, lay, ref):
    """A buffer shaped like lay.out_buf: the reference where the kernel writes, NaN everywhere else; and the mask of the
    elements the kernel owns."""
    exp = torch.full_like(lay.out_buf, float("nan"))
    own = torch.zeros(lay.out_buf.shape, dtype=torch.bool, device=exp.device)
    ref = ref.to(exp.device)
    if exp.dim() == 1:
        exp[GUARD_ROWS:GUARD_ROWS + ref.numel()] = ref.reshape(-1)
        own[GUARD_ROWS:GUARD_ROWS + ref.numel()] = ~torch.isnan(ref.reshape(-1))
    else:
        ch = ref.shape[-1]
        rows = ref.numel() // ch
        exp[GUARD_ROWS:GUARD_ROWS + rows, :ch] = ref.reshape(rows, ch)
        own[GUARD_ROWS:GUARD_ROWS + rows, :ch] = True
    return exp, own


def where_is(c, lay, flat):
    """Human-readable position of element `flat` of lay.out_buf."""
    if lay.out_buf.dim() == 1:
        i = flat - GUARD_ROWS
        if c.head:
            t, ch, y, x = i // (3 * c.H * c.W), i // (c.H * c.W) % 3, i // c.W % c.H, i % c.W
        else:
            ch, t, y, x = i // (c.n_total * c.H * c.W), i // (c.H * c.W) % c.n_total, i // c.W % c.H, i % c.W
    else:
        row, ch = flat // lay.out_ld - GUARD_ROWS, flat % lay.out_ld
        t, y, x = row // (c.H * c.W), row // c.W % c.H, row % c.W
    return f"(t {t}, y {y}, x {x}, channel {ch}; row {y % TILE_H}, column {x % TILE_W} of its {TILE_H} x {TILE_W} tile)"


def compare(c, lay, ref):
    """The acceptance: every element the kernel owns equals the reference bit for bit (so no NaN is left there) and every
    other element of the buffer - guard rows, guard columns, frames a call must not write - still holds its NaN.
    Returns (mismatches inside, NaNs left inside, guard elements changed, message)."""
    exp, own = expected_buffer(c, lay, ref)
    diff = _bits(lay.out_buf) != _bits(exp)
    inside = diff & own
    n_in, n_guard = int(inside.sum()), int((diff & ~own).sum())
    n_nan = int((torch.isnan(lay.out_buf) & own).sum())
    msg = ""
    if n_in:
        first = int(inside.reshape(-1).nonzero()[0])
        msg += (f"{n_in} of {int(own.sum())} outputs differ; first at {where_is(c, lay, first)}: got "
                f"{float(lay.out_buf.reshape(-1)[first])}, expected {float(exp.reshape(-1)[first])}; {n_nan} NaN left inside. ")
    if n_guard:
        first = int((diff & ~own).reshape(-1).nonzero()[0])
        msg += f"{n_guard} guard elements overwritten; first at buffer element {first} {where_is(c, lay, first)}."
    return n_in, n_nan, n_guard, msg


def unsaturated_share(ref):
    """Share of the head's outputs strictly inside (-1, 1)."""
    return float(((ref > -1) & (ref < 1)).float().mean())


def norm_silu_violation(got, conv_bias16, gamma):
    """The acceptance of rtv_rmsnorm_silu_cl (tests/test_vae_units_cpu.py: rms_violation, <= 1 passes) against float64 of the
    exact conv + bias."""
    import test_vae_units_cpu as U
    C = conv_bias16.shape[-1]
    return U.rms_violation(got.reshape(-1, C), conv_bias16.reshape(-1, C), gamma, True)

