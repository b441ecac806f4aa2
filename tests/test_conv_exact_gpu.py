"""The convolution kernels of csrc/vae_conv.hip (gather kernel in its three tile configurations, the three halo-tile forms,
row windows, the fused RMS_norm + SiLU epilogue) and the layer kernels of csrc/taehv.hip on the integer operands of
tests/conv_cases.py: the expected output is known bit for bit for every kernel form, so the acceptance is equality of every
output element with the written-out tap sum, no NaN left, every guard element untouched.  tests/test_conv_exact_cpu.py
proves that each named slip of conv_cases.SLIPS would break that equality on the cases used here.

RTV_CONV_EXACT_RECORD=<path> writes one line per case (kernel and form, largest |integer|, mismatches, guards, seconds)."""
import ctypes
import functools
import os
import time

import pytest
import torch

import conv_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
c_vp = ctypes.c_void_p
RECORD = []


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("RTV_CONV_EXACT_RECORD")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("# case | kernel and forms | largest |integer| in units | launches | mismatches | guards | seconds\n")
            f.write("".join(line + "\n" for line in RECORD))


class Tally:
    """Per-test record: every launch's acceptance is asserted at once; the totals go to the record line."""

    def __init__(self, c, kernel):
        self.c, self.kernel, self.forms, self.launches, self.t0 = c, kernel, [], 0, time.perf_counter()

    def accept(self, form, lay, ref):
        torch.cuda.synchronize()
        n_in, n_nan, n_guard, msg = K.compare(self.c, lay, ref)
        self.launches += 1
        if form not in self.forms:
            self.forms.append(form)
        assert n_in == 0 and n_nan == 0 and n_guard == 0, f"{self.c.name} [{form}]: {msg}"

    def done(self, max_int, extra=""):
        secs = time.perf_counter() - self.t0
        RECORD.append(f"{self.c.name} | {self.kernel}: {', '.join(self.forms)} | {max_int} | {self.launches} | 0 | untouched | "
                      f"{secs:.2f}{extra}")
        print(RECORD[-1])


@functools.lru_cache(maxsize=None)
def _built(c):
    """Operands, exact tap sum (conv_cases.build asserts the exactness condition) and the guarded device layout, once per case."""
    ops, acc = K.build(c)
    return ops, acc, K.lay_out(c, ops, DEV)


def _lib():
    from realtime_video_amd import _lib, taehv, vae_decoder  # noqa: F401  (registers the signatures)
    return _lib.load()


def _p(t):
    return c_vp(t.data_ptr() if t is not None else 0)


def _stream():
    return c_vp(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _zeros():
    return torch.zeros(64, dtype=torch.float16, device=DEV)


def _fresh(lay):
    lay.out_buf.fill_(float("nan"))


def _check_status(st, what):
    from realtime_video_amd import _lib
    _lib.check(st, what)


def _conv_cl(c, lay, use_bias, use_res, flags=0):
    """One rtv_conv_cl / rtv_conv_cl_win launch of a case into its NaN-filled output."""
    lib = _lib()
    _fresh(lay)
    ch = c.n_split or c.Cout
    args = (_p(lay.x), _p(lay.w), _p(lay.bias if use_bias else None), _p(lay.res if use_res else None), lay.res_ld, _p(lay.out),
            lay.out_ld, c.T, c.H, c.W, c.Cin, c.Cout, c.kt, c.kh, c.kw, c.resample | flags, c.n_split, _p(_zeros()))
    assert lay.out_ld == (ch + 4 if c.narrow else ch)
    if c.window:
        _check_status(lib.rtv_conv_cl_win(*args, *c.window, _stream()), "rtv_conv_cl_win")
    else:
        _check_status(lib.rtv_conv_cl(*args, _stream()), "rtv_conv_cl")


def _halo_mode(mode):
    class _Mode:
        def __enter__(self):
            _lib().rtv_conv_set_halo(mode)

        def __exit__(self, *a):
            _lib().rtv_conv_set_halo(1)
    return _Mode()


# (form name, rtv_conv_set_halo mode, flags, launches)
HALO_FORMS = [("persistent", 1, 0, 3), ("one wave per SIMD", 2, 0, 1), ("two waves per SIMD", 3, 0, 1), ("halo off", 0, 0, 1),
              ("RTV_CONV_GATHER", 1, K.GATHER, 1)]


def _run_forms(c, forms, tally):
    ops, acc, lay = _built(c)
    for use_bias, use_res in c.epilogues:
        ref = K.reference(c, ops, use_bias, use_res, acc=acc)
        for name, mode, flags, launches in forms:
            with _halo_mode(mode):
                for _ in range(launches):
                    _conv_cl(c, lay, use_bias, use_res, flags)
                    tally.accept(name, lay, ref)
    tally.done(ops.max_int)


@pytest.mark.parametrize("c", K.HALO_CASES, ids=lambda c: c.name)
def test_halo_layers_in_every_kernel_form(c):
    """3x3x3 layers the halo kernels take, with bias + residual, neither, bias only; under the persistent form (default, three
    launches), the one- and two-waves-per-SIMD forms, the gather kernel by rtv_conv_set_halo(0) and by RTV_CONV_GATHER."""
    _run_forms(c, HALO_FORMS, Tally(c, "rtv_conv_cl 3x3x3"))


def test_more_tiles_than_cus():
    """286 tiles on 256 CUs: several tiles per persistent workgroup, the operand stream crossing tile boundaries.  The reference
    is the same float32 tap loop evaluated on the device (exact for integers wherever it runs): 33 GFLOP, measured 1.5 s in
    float32 plus 2.5 s for the float64 evaluation on eight CPU threads against 0.6 s on the device (printed with the record line) -
    cross-checked on three row bands - top edge, first tile seam, bottom edge - against the CPU float64 loop."""
    c = K.MANY_TILES
    tally = Tally(c, "rtv_conv_cl 3x3x3")
    t0 = time.perf_counter()
    ops, acc = K.build(c, device=DEV, check64=False)           # asserts integers of at most 2048 units
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t0
    for y0, y1 in ((0, 3), (14, 19), (c.H - 3, c.H)):
        lo, hi = max(y0 - 1, 0), min(y1 + 1, c.H)             # the band's rows with the neighbours its taps read
        band = K.conv_taps(ops.x[:, lo:hi], ops.w, c.T, hi - lo, c.W, 3, 3, 3, dtype=torch.float64)
        assert torch.equal(band[:, y0 - lo:y1 - lo], acc[:, y0:y1].double().cpu())
    lay = K.lay_out(c, ops, DEV)
    for use_bias, use_res in c.epilogues:
        ref = K.reference(c, ops, use_bias, use_res, acc=acc)
        _conv_cl(c, lay, use_bias, use_res)
        tally.accept("persistent", lay, ref)
    tally.done(ops.max_int, f" (reference on the device: {t_ref:.2f} s)")


@pytest.mark.parametrize("c", K.UPS_CASES, ids=lambda c: c.name)
def test_upsample_fold(c):
    """The 3x3 conv behind the nearest-2x upsampling: folded into the halo gather (default), RTV_CONV_GATHER, halo off."""
    _run_forms(c, [HALO_FORMS[0][:3] + (1,), HALO_FORMS[4], HALO_FORMS[3]], Tally(c, "rtv_conv_cl upsample 2x + 1x3x3"))


def test_row_windows_equal_the_rows_of_the_whole_image():
    """rtv_conv_cl_win on the stripes the row-sharded decoder derives for world 2 and 3 (conv_cases.window_plan: the library's
    own row plan): every stripe equals its rows of the whole-image reference, stripes whose taps cross the stripe edge inside the
    image included; the whole image through rtv_conv_cl as well."""
    whole_ops, whole_acc, whole_lay = _built(K.WIN_WHOLE)
    whole = K.reference(K.WIN_WHOLE, whole_ops, True, False, acc=whole_acc)
    tally = Tally(K.WIN_WHOLE, "rtv_conv_cl upsample 2x + 1x3x3")
    _conv_cl(K.WIN_WHOLE, whole_lay, True, False)
    tally.accept("persistent", whole_lay, whole)
    tally.done(whole_ops.max_int)
    for c in K.window_cases():
        tally = Tally(c, f"rtv_conv_cl_win rows {c.window[0]}..{c.window[0] + c.H} from source row {c.window[1]}")
        ops, acc, lay = _built(c)
        for name, mode, flags, _ in (HALO_FORMS[0], HALO_FORMS[4]):
            _conv_cl(c, lay, True, False, flags)
            tally.accept(name, lay, whole[:, c.window[0]:c.window[0] + c.H])
        tally.done(ops.max_int)


@pytest.mark.parametrize("c", K.GATHER_CASES + [K.TIME_CONV] + K.DOWN_CASES + K.NARROW_CASES, ids=lambda c: c.name)
def test_gather_kernel_layers(c):
    """The gather kernel's three tile configurations (Cout <= 32; Cout % 96 == 0 with RTV_CONV_GATHER; 128-filter tiles), the
    1x1x1 shortcut, the decoder time_conv with its frame scatter, the encoder's stride-2 forms, and the narrow store path (the
    output a column slice with out_ld = Cout + 4: rows 8-byte but not 16-byte aligned, guard columns untouched)."""
    _run_forms(c, [("default", 1, 0, 1)], Tally(c, "rtv_conv_cl"))


@pytest.mark.parametrize("c", K.NORM_CASES, ids=lambda c: c.name)
def test_fused_rmsnorm_silu_epilogue(c):
    """rtv_conv3_norm_silu_cl: the conv + bias inside is exact here, so the output is a function of known integers - held to
    the acceptance of rtv_rmsnorm_silu_cl (rms_violation <= 1) against float64 of the exact conv + bias."""
    lib = _lib()
    ops, acc, lay = _built(c)
    conv_bias = K.reference(c, ops, True, False, acc=acc)
    tally = Tally(c, "rtv_conv3_norm_silu_cl")
    _fresh(lay)
    st = lib.rtv_conv3_norm_silu_cl(_p(lay.x), _p(lay.w), _p(lay.bias), _p(lay.gamma), _p(lay.out), lay.out_ld, c.T, c.H, c.W,
                                    c.Cin, c.Cout, 0, _p(_zeros()), _stream())
    assert st == 0
    torch.cuda.synchronize()
    got = lay.out.reshape(c.T, c.H, c.W, c.Cout).clone()
    tally.accept("persistent, fused epilogue", lay, got)                  # no NaN inside, guards untouched
    v = K.norm_silu_violation(got.cpu(), conv_bias, ops.gamma)
    assert v <= 1, f"{c.name}: rms_violation {v}"
    tally.done(ops.max_int, f" (violation {v:.3f})")


@pytest.mark.parametrize("c", K.TAEHV_CASES, ids=lambda c: c.name)
def test_taehv_decoder_layer(c):
    lib = _lib()
    ops, acc, lay = _built(c)
    use_bias, use_res = c.epilogues[0]
    ref = K.reference(c, ops, use_bias, use_res, acc=acc)
    tally = Tally(c, "rtv_taehv_conv")
    for _ in range(2):
        _fresh(lay)
        st = lib.rtv_taehv_conv(_p(lay.x), _p(lay.w), _p(lay.bias if use_bias else None), _p(lay.res if use_res else None),
                                _p(lay.out), c.T, c.H, c.W, c.Cin, c.Cout, c.kt, c.ups, c.n_split, c.relu, c.head, _p(_zeros()),
                                _stream())
        _check_status(st, "rtv_taehv_conv")
        tally.accept("layer", lay, ref)
    tally.done(ops.max_int)


@pytest.mark.parametrize("c", K.TAEHV_ENC_CASES, ids=lambda c: c.name)
def test_taehv_encoder_layer(c):
    """Form 0 on frames 1..3 of a 4-frame planar clip (the other frames hold 1024), the stride-2 forms, and the latent head into
    frames 2..5 of a 6-frame planar tensor whose other frames must keep their NaN."""
    lib = _lib()
    ops, acc, lay = _built(c)
    use_bias = c.epilogues[0][0]
    ref = K.reference(c, ops, use_bias, False, acc=acc)
    tally = Tally(c, f"rtv_taehv_enc_conv form {c.form}")
    for _ in range(2):
        _fresh(lay)
        st = lib.rtv_taehv_enc_conv(_p(lay.x), _p(lay.w), _p(lay.bias if use_bias else None), _p(lay.out), c.form, c.T, c.H, c.W,
                                    c.kt, c.n_total, c.n0, _p(_zeros()), _stream())
        _check_status(st, "rtv_taehv_enc_conv")
        tally.accept("layer", lay, ref)
    tally.done(ops.max_int)


@pytest.mark.parametrize("c", [K.HALO_CASES[0], K.UPS_CASES[0]], ids=lambda c: c.name)
def test_device_output_differs_from_every_slipped_reference(c):
    """The comparison runs on what the kernel wrote: against the reference with any one covering slip switched on, the same
    launch is reported with at least the 10 mismatches the CPU proof found (no guard involved)."""
    ops, acc, lay = _built(c)
    use_bias, use_res = c.epilogues[0]
    _conv_cl(c, lay, use_bias, use_res)
    torch.cuda.synchronize()
    assert K.compare(c, lay, K.reference(c, ops, use_bias, use_res, acc=acc))[:3] == (0, 0, 0)
    for slip in K.covering_slips(c):
        n_in, n_nan, n_guard, msg = K.compare(c, lay, K.reference(c, ops, use_bias, use_res, slip=slip))
        assert n_in >= 10 and n_nan == 0 and n_guard == 0 and "first at (t " in msg, (slip, n_in)
