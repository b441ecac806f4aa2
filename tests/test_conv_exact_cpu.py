"""CPU proof that tests/test_conv_exact_gpu.py would notice: for every case of tests/conv_cases.py the exactness condition
holds (integers of at most 2048 units, float32 tap sum == float64 tap sum, == torch's convolution on the small plain cases),
every named slip changes at least 10 output elements on every case listed as covering it, every slip is covered, and the
clamped head keeps at least a quarter of its outputs strictly inside (-1, 1)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_cases as K

MIN_CHANGED = 10
SMALL_CASES = [c for c in K.STATIC_CASES if not c.big]


@functools.lru_cache(maxsize=4)
def _built(c):
    return K.build(c)


def _full_ref(c, ops, acc=None, slip=None):
    """The reference with every epilogue term a case ever runs with."""
    use_bias = any(b for b, _ in c.epilogues)
    use_res = any(r for _, r in c.epilogues)
    return K.reference(c, ops, use_bias, use_res, slip=slip, acc=acc if slip is None else None)


def _exact_and_slips_show(c):
    ops, acc = _built(c)                                     # asserts integers <= 2048 units and float32 == float64
    assert 0 < ops.max_int <= K.EXACT_MAX
    good = _full_ref(c, ops, acc)
    assert good.dtype == (torch.float32 if c.head else torch.float16)
    good64 = K.reference(c, ops, any(b for b, _ in c.epilogues), any(r for _, r in c.epilogues), dtype=torch.float64)
    assert torch.equal(torch.nan_to_num(good.double(), nan=-7.0), torch.nan_to_num(good64.double(), nan=-7.0))
    for slip in K.covering_slips(c):
        bad = _full_ref(c, ops, slip=slip)
        changed = int((torch.nan_to_num(bad.double(), nan=-7.0) != torch.nan_to_num(good.double(), nan=-7.0)).sum())
        print(f"{c.name}: {slip}: {changed} of {good.numel()} outputs change")
        assert changed >= MIN_CHANGED, (c.name, slip, changed)


@pytest.mark.parametrize("c", SMALL_CASES, ids=lambda c: c.name)
def test_case_is_exact_and_every_covering_slip_shows(c):
    _exact_and_slips_show(c)


@pytest.mark.parametrize("world,rank", K.WINDOWS)
def test_row_window_stripe_is_exact_and_every_covering_slip_shows(world, rank):
    _exact_and_slips_show(K.window_case(world, rank))


def test_every_slip_is_covered_by_a_case():
    seen = set()
    for c in SMALL_CASES + K.window_cases():
        seen.update(K.covering_slips(c))
    assert seen == set(K.SLIPS)


def test_many_tiles_case_is_listed_with_the_slips_of_its_small_twin():
    """The 286-tile case is too large for a CPU slip proof; it is HALO_CASES[0] at another size (same channels, taps and
    epilogues), so the slips proven there are the ones it covers, and its exactness is asserted where its reference is evaluated."""
    small, big = K.HALO_CASES[0], K.MANY_TILES
    assert (small.Cin, small.Cout, small.kt, small.kh, small.kw, small.epilogues) == (big.Cin, big.Cout, big.kt, big.kh, big.kw,
                                                                                      big.epilogues)
    assert set(K.covering_slips(small)) == set(K.covering_slips(big))
    tiles = big.T * -(-big.H // K.TILE_H) * -(-big.W // K.TILE_W)
    assert tiles == 286 > 256


@pytest.mark.parametrize("c", [c for c in K.STATIC_CASES if c.api == "conv_cl" and not c.big and not c.n_split and c.T * c.H * c.W <= 5000],
                         ids=lambda c: c.name)
def test_tap_sum_equals_torch_convolution(c):
    """The written-out tap loop against torch's own convolution on the small VAE cases (float64, where any algorithm is exact)."""
    ops, acc = _built(c)
    x = ops.x.double().permute(3, 0, 1, 2)[None]                                            # [1][Cin][Tin][inH][inW]
    w = ops.w.double().reshape(c.Cout, c.kt, c.kh, c.kw, c.Cin).permute(0, 4, 1, 2, 3)
    r = c.resample & ~K.GATHER
    if r == K.UPSAMPLE2X:
        x = F.interpolate(x, scale_factor=(1, 2, 2), mode="nearest")
    if r == K.DOWN2X:
        y = F.conv3d(F.pad(x, (0, 1, 0, 1, 0, 0)), w, stride=(1, 2, 2))
    elif r == K.TIME_DOWN2X:
        y = F.conv3d(x, w, stride=(2, 1, 1))
    else:
        y = F.conv3d(F.pad(x, (c.kw // 2,) * 2 + (c.kh // 2,) * 2 + (0, 0)), w)
    assert torch.equal(y[0].permute(1, 2, 3, 0), acc.double())


@pytest.mark.parametrize("c", K.TAEHV_CASES + K.TAEHV_ENC_CASES, ids=lambda c: c.name)
def test_taehv_reference_equals_torch_convolution(c):
    """The TAEHV forms against the torch expressions the Gaussian tests of tests/test_taehv_gpu.py and
    tests/test_taehv_encoder_gpu.py use as their reference."""
    ops, acc = _built(c)
    use_bias, use_res = c.epilogues[0]
    got = K.reference(c, ops, use_bias, use_res, acc=acc)
    b = ops.bias.double() if use_bias else None
    if c.api == "taehv_enc" and c.form == 0:
        x01 = (0.5 * ops.x.float() + 0.5).half().double()[:, c.n0:c.n0 + c.T].transpose(0, 1)
        ref = F.relu(F.conv2d(x01, ops.w[:, :27].double().reshape(64, 3, 3, 3), b, padding=1)).permute(0, 2, 3, 1)
        assert torch.equal(got.double(), ref)
        return
    x = ops.x.double().permute(0, 3, 1, 2)
    w = ops.w.double().reshape(c.Cout, c.kt, 3, 3, c.Cin).permute(0, 4, 1, 2, 3)
    if c.api == "taehv_enc" and c.form == 1:
        ref = sum(F.conv2d(x[dt::c.kt], w[:, :, dt], stride=2, padding=1) for dt in range(c.kt))
        assert torch.equal(got.double(), ref.permute(0, 2, 3, 1))
        return
    if c.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    ref = sum(F.conv2d(x[dt:dt + c.T], w[:, :, dt], padding=1) for dt in range(c.kt))
    if b is not None:
        ref = ref + b[None, :, None, None]
    if use_res:
        ref = F.relu(ref + ops.res.double().permute(0, 3, 1, 2))
    elif c.relu:
        ref = F.relu(ref)
    if c.head:
        assert torch.equal(got.double(), (2 * ref - 1).clamp(-1, 1)[:, :3])
    elif c.api == "taehv_enc":                                   # form 2: planar frames n0 .. n0 + T, NaN elsewhere
        assert torch.equal(got[:, c.n0:c.n0 + c.T].double(), ref.transpose(0, 1))
        assert bool(torch.isnan(got[:, :c.n0]).all()) and bool(torch.isnan(got[:, c.n0 + c.T:]).all())
    elif c.n_split:
        ref = torch.stack([ref[:, :c.n_split], ref[:, c.n_split:]], 1).reshape(2 * c.T, c.n_split, c.H, c.W)
        assert torch.equal(got.double(), ref.permute(0, 2, 3, 1))
    else:
        assert torch.equal(got.double(), ref.permute(0, 2, 3, 1))


def test_taehv_cases_are_the_forms_of_the_gaussian_test():
    import test_taehv_gpu as G
    assert K._TAEHV_FORMS == G.FORMS


@pytest.mark.parametrize("c", K.CLAMP_CASES, ids=lambda c: c.name)
def test_clamped_head_is_mostly_unsaturated(c):
    ops, acc = _built(c)
    share = K.unsaturated_share(K.reference(c, ops, True, False, acc=acc))
    print(f"{c.name}: {share:.3f} of the outputs strictly inside (-1, 1)")
    assert share >= 0.25


def test_row_windows_are_stripes_of_the_whole_image():
    """Each stripe's reference is the corresponding rows of the whole-image reference; the stripes of a world cover the image,
    and at least one stripe per world has taps that cross its edge inside the image and a window that starts inside the input."""
    whole_ops, whole_acc = _built(K.WIN_WHOLE)
    whole = K.reference(K.WIN_WHOLE, whole_ops, True, False, acc=whole_acc)
    wins = K.window_cases()
    for c in wins:
        y_out0, y_in0, in_rows, img_rows = c.window
        assert img_rows == K.WIN_WHOLE.H and 0 <= y_in0 and y_in0 + in_rows <= img_rows // 2
        ops, acc = _built(c)
        assert torch.equal(K.reference(c, ops, True, False, acc=acc), whole[:, y_out0:y_out0 + c.H])
    for world in K.WIN_WORLDS:
        mine = [c for c in wins if c.name.startswith(f"win_world{world}_")]
        rows = set().union(*(range(c.window[0], c.window[0] + c.H) for c in mine))
        assert rows == set(range(K.WIN_WHOLE.H))
        assert any(c.window[0] > 0 and c.window[1] > 0 for c in mine)                      # interior upper edge
        assert any(c.window[0] + c.H < c.window[3] for c in mine)                          # interior lower edge


def test_guarded_layout_and_acceptance_on_the_cpu():
    """lay_out / compare on the CPU: the reference itself passes; one wrong element, one NaN left, one guard row and one guard
    column overwritten are each reported."""
    c = K.NARROW_CASES[1]
    ops, acc = _built(c)
    ref = K.reference(c, ops, True, True, acc=acc)
    lay = K.lay_out(c, ops, "cpu")
    assert lay.out_ld == c.Cout + 4 and lay.out.data_ptr() % 16 == 0 and (lay.out_ld * 2) % 16 == 8
    assert float(lay.x_buf[0].min()) == float(lay.x_buf[-1].max()) == K.GUARD_IN and torch.equal(lay.x.cpu(), ops.x)
    assert K.compare(c, lay, ref)[:3] == (c.T * c.H * c.W * c.Cout, c.T * c.H * c.W * c.Cout, 0)      # nothing written yet
    lay.out.copy_(ref.reshape(-1, c.Cout))
    assert K.compare(c, lay, ref) == (0, 0, 0, "")
    lay.out[c.W + 3, 5] += 1
    n_in, n_nan, n_guard, msg = K.compare(c, lay, ref)
    assert (n_in, n_nan, n_guard) == (1, 0, 0) and "(t 0, y 1, x 3, channel 5; row 1, column 3" in msg
    lay.out[c.W + 3, 5] = float("nan")
    assert K.compare(c, lay, ref)[:3] == (1, 1, 0)
    lay.out.copy_(ref.reshape(-1, c.Cout))
    lay.out_buf[K.GUARD_ROWS - 1, 0] = 0
    lay.out_buf[K.GUARD_ROWS + 2, c.Cout + 1] = 0
    assert K.compare(c, lay, ref)[:3] == (0, 0, 2)
