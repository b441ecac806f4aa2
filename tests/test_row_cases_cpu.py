"""CPU checks of tests/row_cases.py: the builders keep their promises, an emulation of the row kernels' arithmetic stays inside
the worst case of every bar (ratio <= 1, half the bar) on every family, every mutant of the emulation fails on the family named
for it, and every family kills a mutant.  tests/test_row_kernels_gpu.py runs the HIP kernels on the same inputs under the same
bars.  Each emulation test prints `ROW_EMU ... ratio=` (pytest -s): the largest |out - ref| over the WORST CASE."""
import functools

import pytest
import torch

import row_cases as rc
from realtime_video_amd.rope import rope_cos_sin_table

MUTANT_WIDTHS = [256, 2048, 2056]         # one pass partly filled; every wave's partial in use; the last chunk alone in a pass
GEOMS = [(5, 7), (0, 6), (9, 5)]          # (row_offset, rows_per_frame) of the modulated launches: frame boundaries inside 17 rows


def _exact_bf16(x, want):
    return torch.equal(x.double(), want.double())


# ------------------------------------------------------------------------------------------------ builders
@pytest.mark.parametrize("d", rc.LN_WIDTHS)
def test_spike_chunk_carries_the_row(d):
    nch = d // 8
    for positive in (False, True):
        x = rc.spike(d, positive=positive).double()
        assert x.shape == (nch, d)
        chunks = x.view(nch, nch, 8)
        own = chunks[torch.arange(nch), torch.arange(nch)]
        share2 = (own ** 2).sum(-1) / (x ** 2).sum(-1)
        assert float(share2.min()) >= 0.9, (d, positive, float(share2.min()))
        if positive:
            assert float(x.min()) >= 0
            share1 = own.sum(-1) / x.sum(-1)
            assert float(share1.min()) >= 0.5, (d, float(share1.min()))
    x = rc.spike(256, M=33)
    assert x.shape == (33, 256) and float(x[32, :8].abs().min()) >= rc.SPIKE            # the sweep wraps round


def test_offset_and_near_constant_rows_are_exact_in_bf16():
    for mean, spacing in ((64.0, 0.5), (1024.0, 8.0)):
        x = rc.offset(17, 2056, mean).double()
        k = (x - mean) / spacing
        assert torch.equal(k, k.round()) and float(k.abs().max()) == 3 and float(k.min()) == -3
        assert abs(float(x.mean()) - mean) < spacing
    x = rc.near_constant(17, 1536).double()
    assert torch.equal((x == 1032).sum(-1), torch.ones(17, dtype=torch.long)) and torch.equal((x == 1024).sum(-1), torch.full((17,), 1535))
    assert len({int(c) for c in (x == 1032).double().argmax(-1)}) == 17                    # a different column in every row


def test_one_pass_variance_is_wrong_on_near_constant_rows():
    """The claim of family 4: the two-pass variance in fp32 is right; the one-pass one, a difference of two numbers near 2^20
    whose fp32 spacing is 0.125, misses a variance of 0.04 and less by more than the variance itself (it comes out negative)."""
    for d in (1536, 5120, 8192):
        x = rc.near_constant(5, d)
        true = 64.0 * (d - 1) / d ** 2
        x32 = x.float()
        mean = x32.mean(-1, keepdim=True)
        two = float(((x32 - mean) ** 2).mean(-1)[0])
        one = float(((x32 * x32).mean(-1, keepdim=True) - mean * mean)[0])
        assert abs(two - true) <= 1e-3 * true
        assert abs(one - true) >= true, (d, one, true)


def test_constant_rows_are_constant_after_rounding():
    x = rc.constant(17, 2056)
    want = torch.tensor([rc.CONSTANTS[i % 7] for i in range(17)], dtype=torch.float64).view(17, 1).expand(17, 2056)
    assert _exact_bf16(x, want)
    assert float(x[0].abs().max()) == 0


def test_scaled_families_keep_their_scale():
    assert 0.5e-3 < float(rc.gaussian(17, 2048, 2, 1e-3).float().std()) < 2e-3
    assert 0.5e-10 < float(rc.gaussian(17, 2048, 3, 1e-10).float().std()) < 2e-10
    huge = rc.gaussian(17, 8192, 4, 2.0 ** 40).float()
    assert torch.isfinite((huge * huge).sum(-1)).all() and float(huge.std()) > 2.0 ** 39   # the squares stay inside fp32
    m = rc.mixed(40, 2048).double()
    sd = m.std(-1)
    for i in range(40):
        assert 0.9 < float(sd[i]) / (2.0 * 2.0 ** (i % 24 - 12)) < 1.1


def test_frame_tables_tell_frames_apart():
    t = rc.frame_tables(4, 256, 6).double()
    for f in range(4):
        assert torch.equal(t[f, 0], torch.full((256,), 16.0 * (f + 1)))
    assert t.shape == (4, 6, 256)


def test_rope_geometry_of_the_shard():
    for M in (33, 257, 1025):
        for ring in (False, True):
            g = rc.rope_geom(M, ring=ring)
            F, gh, gw = g.grid
            assert g.start_frame + F == 1024 and gw & (gw - 1) and g.row_offset > 0 and g.row_offset + M < F * gh * gw
            pf, ph, pw = rc.token_positions(M, g.grid, g.start_frame, g.row_offset)
            assert int(pw.max()) == gw - 1 and ((ph == gh - 1) & (pw == gw - 1)).any()
            assert int(pf.max()) == 1023                                                    # the table's last entry
            rows = g.cache_index()
            assert len(set(rows.tolist())) == M and int(rows.min()) >= g.cache_row0 and int(rows.max()) < g.cache_rows
            if ring:
                assert not torch.equal(rows, g.cache_row0 + g.row_offset + torch.arange(M))


@pytest.mark.parametrize("hd", [128, 192, 256])
def test_rope_table_matches_the_fp64_angles(hd):
    """The project's fp32 table against the angles of `rope64`, computed from the definition: hd = 192 (the LANE_CS = false
    instantiation) has 32 pairs on each axis, hd = 128 has 22 + 21 + 21."""
    table = rope_cos_sin_table(hd).double()
    pos = torch.arange(1024)
    ang = rc.rope_angles64(hd, pos, pos, pos)
    assert rc.axis_split(hd) == {128: (22, 21), 192: (32, 32), 256: (44, 42)}[hd]
    assert float((table[..., 0] - torch.cos(ang)).abs().max()) <= 2.0 ** -24
    assert float((table[..., 1] - torch.sin(ang)).abs().max()) <= 2.0 ** -24


# ------------------------------------------------------------------------------------------------ emulation inside the worst case
@functools.lru_cache(maxsize=None)
def _ln_fam(d):
    return rc.ln_families(d)


@functools.lru_cache(maxsize=None)
def _rms_fam(d):
    return rc.rms_families(d)


def _ln_forms(d, M, geom=0):
    """form name -> keyword arguments of ln64 / emulate_ln."""
    w, b = rc.gains(d)
    off, rpf = GEOMS[geom]
    F = (off + M - 1) // rpf + 1
    t6, t2 = rc.frame_tables(F, d, 6), rc.frame_tables(F, d, 2, seed=1)
    return {"plain": {}, "affine": dict(weight=w, bias=b),
            "mod6": dict(shift=t6[:, 0], scale=t6[:, 1], rows_per_frame=rpf, row_offset=off),
            "mod2": dict(shift=t2[:, 0], scale=t2[:, 1], rows_per_frame=rpf, row_offset=off)}


def _check(tag, out, ref, worst, limit=1.0):
    ok, ratio, where = rc.within(out, ref, worst)
    print(f"ROW_EMU {tag} ratio={ratio:.3f}")
    assert ok and ratio <= limit, f"{tag}: |out - ref| = {ratio:.3f} x the worst case at (row, column) {where}"
    return ratio


@pytest.mark.parametrize("d", rc.LN_WIDTHS)
def test_layernorm_emulation_is_inside_the_worst_case(d):
    for name, x in _ln_fam(d).items():
        for form, kw in _ln_forms(d, x.shape[0]).items():
            ref, worst = rc.ln64(x, **kw)
            _check(f"kernel=layernorm form={form} family={name} d={d}", rc.emulate_ln(x, **kw), ref, worst)


@pytest.mark.parametrize("d", rc.LN_WIDTHS)
def test_rmsnorm_emulation_is_inside_the_worst_case(d):
    w, _ = rc.gains(d, 1)
    for name, x in _rms_fam(d).items():
        ref, worst = rc.rms64(x, w)
        _check(f"kernel=rmsnorm family={name} d={d}", rc.emulate_rms(x, w), ref, worst)


def _rope_run(d, H, x, mutant=None, ring=False):
    """The emulation on the rows x (used as q, as k and, bit for bit, as v) -> (q, k rows written, references, geometry)."""
    M = x.shape[0]
    g = rc.rope_geom(M, ring=ring)
    wq, wk = rc.gains(d, 2)[0], rc.gains(d, 3)[0]
    qkv = rc.rope_qkv(x)
    kc = torch.full((g.cache_rows, d), 7.0, dtype=rc.BF16)
    vc = torch.full((g.cache_rows, d), 7.0, dtype=rc.BF16)
    q = rc.emulate_rope(qkv, wq, wk, H, g, rope_cos_sin_table(d // H), kc, vc, mutant=mutant)
    return q, kc, vc, qkv, (wq, wk), g


def _rope_check(tag, d, H, x, mutant=None, ring=False):
    """-> (ok, ratio) of the emulated launch against rope64 on q and on the cache rows the geometry names; untouched cache rows
    and V count as exact."""
    q, kc, vc, qkv, (wq, wk), g = _rope_run(d, H, x, mutant, ring)
    rows = g.cache_index()
    rq, wq_ = rc.rope64(qkv[:, :d], wq, H, g.grid, g.start_frame, g.row_offset)
    rk, wk_ = rc.rope64(qkv[:, d:2 * d], wk, H, g.grid, g.start_frame, g.row_offset)
    ok_q, ratio_q, _ = rc.within(q, rq, wq_)
    ok_k, ratio_k, _ = rc.within(kc[rows], rk, wk_)
    rest = torch.ones(g.cache_rows, dtype=torch.bool)
    rest[rows] = False
    clean = torch.equal(vc[rows], qkv[:, 2 * d:]) and bool((kc[rest] == 7).all()) and bool((vc[rest] == 7).all())
    return ok_q and ok_k and clean, max(ratio_q, ratio_k)


@pytest.mark.parametrize("d,H", rc.ROPE_SHAPES)
def test_rope_emulation_is_inside_the_worst_case(d, H):
    for name, x in rc.rope_families(d).items():
        ok, ratio = _rope_check(name, d, H, x, ring=name == "gaussian")
        print(f"ROW_EMU kernel=rope family={name} d={d} H={H} ratio={ratio:.3f}")
        assert ok and ratio <= 1.0, (name, d, H, ratio)


# ------------------------------------------------------------------------------------------------ mutants
# mutant -> the families that must fail it (at every width of MUTANT_WIDTHS, unless a width is given)
OFFSET_ROWS = ["spike", "spike_positive", "offset64", "offset1024", "near_constant"]   # rows whose mean a lost chunk moves
LN_KILLS = {"a": OFFSET_ROWS, "b": OFFSET_ROWS,
            "c": ["near_constant"], "e": ["constant", "tiny1e-3", "tiny1e-10"], "l": ["huge"], "m": ["mixed"]}
LN_TABLE_KILLS = {"d0": "mod6", "d1": "mod2", "f": "mod6"}
RMS_KILLS = {"a": ["spike"], "b": ["spike"], "e": ["constant", "tiny1e-3", "tiny1e-10"], "l": ["huge"], "m": ["mixed"]}
ROPE_KILLS = {"a": ["spike"], "b": ["spike"], "e": ["constant", "tiny1e-3"], "g": ["gaussian"], "h": ["gaussian"], "i": ["gaussian"],
              "j": ["gaussian"], "k": ["gaussian"], "l": ["huge"], "m": ["mixed"]}


def _ln_fails(x, mutant, kw):
    ref, worst = rc.ln64(x, **kw)
    return not rc.within(rc.emulate_ln(x, mutant=mutant, **kw), ref, worst)[0]


@pytest.mark.parametrize("d", MUTANT_WIDTHS)
def test_layernorm_mutants_fail_on_their_families(d):
    killed = {name: set() for name in _ln_fam(d)}
    for mutant, names in LN_KILLS.items():
        for name in names:
            if (mutant == "b" and d < 1544) or (mutant == "c" and d < 1536):
                continue                             # wave 3 holds no chunk of so short a row; the one-pass sums are still exact
            x = _ln_fam(d)[name]
            for form, kw in _ln_forms(d, x.shape[0]).items():
                assert _ln_fails(x, mutant, kw), f"mutant {mutant} ({rc.MUTANTS[mutant]}) passes on {name}, {form}, d = {d}"
            killed[name].add(mutant)
    for name, x in _ln_fam(d).items():                                   # family 8: the tables under every family of 17 rows
        if x.shape[0] != 17:
            continue
        for geom in range(len(GEOMS)):
            forms = _ln_forms(d, 17, geom)
            for mutant, form in LN_TABLE_KILLS.items():
                if (mutant == "d0" and GEOMS[geom][0] == 0) or (mutant == "f" and name in ("constant", "tiny1e-10")):
                    continue                                           # no offset to ignore; n = 0 (or 1e-7) times any scale is sh_f
                assert _ln_fails(x, mutant, forms[form]), f"mutant {mutant} ({rc.MUTANTS[mutant]}) passes on {name}, {form}, d = {d}"
                if name == "gaussian":
                    killed[name].add(mutant)                           # the other families are held to a mutant of their own
    idle = [n for n, k in killed.items() if not k]
    assert not idle, f"families that kill no mutant: {idle}"


def test_gaussian_rows_miss_a_chunk_dropped_from_the_sum_of_squares():
    """Why the spike sweep: at d = 5120 a chunk dropped from sum x^2 moves every output of a Gaussian row by 0.08 %, a fifth of
    u, inside the RMSNorm bar (as inside any bar of u or more); on the spike rows it is an O(1) error in a known row.  (The
    LayerNorm bar does see it on Gaussian rows, through the mean: the elements next to the mean are held to t32.)"""
    w, _ = rc.gains(5120, 1)
    for x, fails in ((rc.gaussian(17, 5120, 5), False), (rc.spike(5120, seed=1), True)):
        ref, worst = rc.rms64(x, w)
        ok, ratio, (row, _) = rc.within(rc.emulate_rms(x, w, mutant="a"), ref, worst)
        assert ok != fails, ratio
    assert row == 5120 // 8 - 1                                         # the row whose spike is the dropped chunk


@pytest.mark.parametrize("d", MUTANT_WIDTHS)
def test_rmsnorm_mutants_fail_on_their_families(d):
    w, _ = rc.gains(d, 1)
    killed = {name: set() for name in _rms_fam(d)}
    for mutant, names in RMS_KILLS.items():
        for name in names:
            if mutant == "b" and d < 1544:
                continue
            x = _rms_fam(d)[name]
            ref, worst = rc.rms64(x, w)
            assert not rc.within(rc.emulate_rms(x, w, mutant=mutant), ref, worst)[0], \
                f"mutant {mutant} ({rc.MUTANTS[mutant]}) passes on {name}, d = {d}"
            killed[name].add(mutant)
    idle = [n for n, k in killed.items() if not k and n != "gaussian"]     # the Gaussian rows are the RoPE mutants' family
    assert not idle, idle


@pytest.mark.parametrize("d,H", [(256, 2), (2048, 16), (1536, 8)])
def test_rope_mutants_fail_on_their_families(d, H):
    fam = rc.rope_families(d)
    killed = {name: set() for name in fam}
    for mutant, names in ROPE_KILLS.items():
        for name in names:
            if mutant == "b" and d < 1544:
                continue
            x = fam[name]
            ok, _ = _rope_check(name, d, H, x, mutant=mutant, ring=mutant == "k")
            assert not ok, f"mutant {mutant} ({rc.MUTANTS[mutant]}) passes on {name}, d = {d}, {H} heads"
            killed[name].add(mutant)
    idle = [n for n, k in killed.items() if not k and n != "tiny1e-10"]    # sigma 1e-10 with eps omitted is RMSNorm's and LayerNorm's
    assert not idle, idle


def test_every_mutant_has_a_family():
    named = set(LN_KILLS) | set(LN_TABLE_KILLS) | set(RMS_KILLS) | set(ROPE_KILLS)
    assert named == set(rc.MUTANTS), sorted(set(rc.MUTANTS) - named)
