"""CPU checks of tests/t5_cases.py: what the builders promise (a lead of at least 12 nats, a target weight of at least 1 - 1e-5, no
score beyond 80 nats, every relative distance covered), that the emulation of each kernel of the text encoder passes its bar on every
input of tests/test_t5_kernels_gpu.py - within the worst case for the row kernels - and that every named mutant fails at least one
input; the binding of include/rtv_hip_t5_units.h and the launchers' refusals, which need no device."""
import ctypes
import math
import os

import pytest
import torch

import attn_cases as ac
import row_cases as rc
import t5_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return list(tc.attention_cases())


@pytest.fixture(scope="module")
def sweep():
    return list(tc.sweep_cases())


# ------------------------------------------------------------------------------------------------ attention: builder promises
def _promises(case):
    """(smallest target weight, smallest lead in nats, largest |score| over the valid keys) of the rows that name targets."""
    n = case.valid
    s = ac.scores64(case.q[None, :n], case.k[None, :n], 1.0, None, case.bias())[0]                 # [H, n, n]
    top = float(s.abs().max())
    tg = case.targets
    if tg is None:
        return 1.0, math.inf, top
    tgh = tg.permute(1, 0, 2)                                                                      # [H, n, T]
    named = (tgh >= 0).all(-1)
    if not bool(named.any()):
        return 1.0, math.inf, top
    hit = torch.zeros_like(s, dtype=torch.bool).scatter_(-1, tgh.clamp(min=0), True) & named.unsqueeze(-1)
    p = torch.softmax(s, -1)
    weight = float((p * hit).sum(-1)[named].min())
    rest = s.masked_fill(hit, -math.inf).amax(-1)
    lead = float((s.masked_fill(~hit, -math.inf).amax(-1) - rest)[named].min()) if n > tg.shape[-1] else math.inf
    return weight, lead, top


def test_attention_builders_keep_their_promises(cases, sweep):
    worst = {"weight": 1.0, "lead": math.inf, "score": 0.0}
    for case in cases + sweep:
        assert case.rows % 32 == 0 and case.valid <= case.rows and case.valid <= case.max_len, case.name
        assert case.table.shape == (case.H, 2 * case.max_len - 1) and case.table.dtype == torch.float32
        assert bool(torch.isfinite(case.v.float()).all()) and bool(torch.isfinite(case.q.float()).all()), case.name   # the contract
        assert bool(torch.isfinite(case.k[:case.valid].float()).all()), case.name
        weight, lead, top = _promises(case)
        assert weight >= 1 - 1e-5, f"{case.name}: target weight {weight}"
        assert lead >= 12.0, f"{case.name}: lead {lead:.2f} nats"
        assert top <= 80.0, f"{case.name}: score {top:.1f} nats"
        worst.update(weight=min(worst["weight"], weight), lead=min(worst["lead"], lead), score=max(worst["score"], top))
    print(f"T5 BUILDERS: smallest target weight {worst['weight']:.8f}, smallest lead {worst['lead']:.2f} nats, largest |score| "
          f"{worst['score']:.1f} nats")


def test_attention_shapes_cover_what_the_issue_names(cases):
    valids = {c.valid for c in cases}
    assert valids >= {1, 31, 32, 33, 63, 64, 65, 300, 512, 48}
    assert {c.H for c in cases} >= {1, 3, 4, 64}
    for v in (1, 31, 32, 33, 63, 64, 65, 300, 512):
        lens = {c.max_len for c in cases if c.valid == v and c.rows == tc.roundup32(v)}
        assert 512 in lens and tc.roundup32(v) in lens, (v, lens)
    assert any(c.valid == 48 and c.max_len == 48 and c.rows == 64 for c in cases)                  # the finding's case
    assert any(c.rows == tc.roundup32(c.valid) + 64 for c in cases)                                # two blocks wider than needed
    fams = {c.family for c in cases}
    assert fams == {"one_hot", "gaussian", "content_vs_bias", "mask_edge", "running_max"}
    assert any(bool(torch.isnan(c.k[c.valid:].float()).all()) for c in cases if c.family == "mask_edge")


def test_every_distance_is_some_rows_target(sweep):
    for valid, H, L in tc.SWEEP_SHAPES:
        seen = set()
        for case in (c for c in sweep if (c.valid, c.H, c.max_len) == (valid, H, L)):
            tg = case.targets[..., 0]
            rows = torch.arange(valid).view(-1, 1).expand_as(tg)
            seen |= set((tg - rows)[tg >= 0].tolist())
            spikes = (case.table == tc.SPIKE).sum(1)
            assert bool((spikes == 1).all()) and len({int(r.argmax()) for r in case.table}) == min(H, 2 * valid - 1)   # one per head, all different
        assert seen == set(range(-(valid - 1), valid)), (valid, H, L)


def test_attention_references_are_the_known_answers():
    c = tc.one_hot(65, 3, 96, seed=1)
    ref, _ = c.reference()
    want = torch.gather(c.v[:65].double(), 0, c.targets.expand(-1, -1, 64))
    assert float((ref[0] - want).abs().max()) <= 1e-4
    b = tc.bias_one_hot(65, 3, 96, [-64, 0, 17])
    ref, _ = b.reference()
    for h, r in enumerate((-64, 0, 17)):
        i = torch.arange(max(0, -r), min(65, 65 - r))
        assert float((ref[0, i, h] - b.v[i + r, h].double()).abs().max()) <= 1e-9
    t = tc.content_vs_bias(300, 4, 320)
    ref, _ = t.reference()
    named = (t.targets >= 0).all(-1)
    assert int(named.sum()) >= 4 * 280
    mean = 0.5 * (torch.gather(t.v[:300].double(), 0, t.targets[..., :1].clamp(min=0).expand(-1, -1, 64)) +
                  torch.gather(t.v[:300].double(), 0, t.targets[..., 1:].clamp(min=0).expand(-1, -1, 64)))
    assert float((ref[0] - mean)[named].abs().max()) <= 1e-9                                       # an exact tie
    for late in (True, False):
        m = tc.running_max(300, 3, 512, late)
        s = ac.scores64(m.q[None, :300], m.k[None, :300], 1.0, None, m.bias())[0] * tc.LOG2E
        blocks = torch.stack([s[..., j:j + 32].amax(-1) for j in range(0, 300, 32)], -1)
        run = torch.cummax(blocks, -1).values
        grows = ((run[..., 1:] - run[..., :-1]) > 1.0).sum(-1)
        assert int(grows.min()) == 9 if late else int(grows.max()) == 0
        assert bool((m.targets >= 288).all()) if late else bool((m.targets < 32).all())


# ------------------------------------------------------------------------------------------------ attention: emulation and mutants
def test_emulated_attention_is_within_the_bound(cases, sweep):
    worst = {}
    for case in cases + sweep:
        out = tc.emulate_attention(case)
        assert bool(torch.isfinite(out.float()).all()), f"{case.name}: a padding query row is not finite"
        ok, ratio, idx = case.within(out)
        worst[case.family] = max(worst.get(case.family, 0.0), ratio)
        assert ok, f"{case.name}: ratio {ratio:.2f} at (batch, row, head, dim) {idx}"
    print("T5 EMULATION attention, largest |out - ref| / (u ref_abs) per family: " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= ac.BOUND_FACTOR


def test_wide_launch_is_the_tight_launch_on_the_valid_rows():
    valid, H, L, rows = tc.WIDE
    wide, tight = tc.one_hot(valid, H, L, rows, seed=valid + H), tc.one_hot(valid, H, L, seed=valid + H)
    assert wide.rows == tight.rows + 64
    again = tc.AttnCase(tight.name, tight.family, wide.q[:valid], wide.k[:valid], wide.v[:valid], wide.table, valid, L, wide.targets)
    assert torch.equal(tc.emulate_attention(wide)[:valid], tc.emulate_attention(again)[:valid])


@pytest.mark.parametrize("mutant", list(tc.ATTN_MUTANTS))
def test_every_attention_mutant_fails_some_case(cases, sweep, mutant):
    pool = cases + [c for c in sweep if c.valid in (33, 65)]
    caught = []
    for case in pool:
        ok, ratio, _ = case.within(tc.emulate_attention(case, mutant))
        if not ok:
            caught.append((ratio, case.name))
    assert caught, f"mutant '{mutant}' ({tc.ATTN_MUTANTS[mutant]}) passes every case"
    ratio, name = max(caught)
    print(f"T5 MUTANT attention {mutant}: fails {len(caught)} of {len(pool)} cases, worst ratio {ratio:.1f} ({name})")
    assert ratio >= 3.0 * ac.BOUND_FACTOR


def test_l_from_rounded_p_stays_inside_the_bar(cases):
    """The one named error the bar cannot see (t5_cases docstring: 3 u P|V| at worst).  Kept as a test so that the limit is on record."""
    worst = 0.0
    for case in cases:
        ok, ratio, _ = case.within(tc.emulate_attention(case, "l_rounded"))
        worst = max(worst, ratio)
        assert ok, case.name
    print(f"T5 MUTANT attention l_rounded: inside the bar everywhere, largest ratio {worst:.2f} of {ac.BOUND_FACTOR}")
    assert worst <= 3.0 * (1 + 2 * tc.U) + 0.01


# ------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("d", tc.RMS_WIDTHS)
def test_emulated_rmsnorm_is_within_the_worst_case(d):
    w = rc.gains(d, 1)[0]
    for out_f32 in (False, True):
        worst = {}
        for family, x in tc.rms_families(d).items():
            assert float(x.abs().max()) ** 2 * d < 3.0e38, family                                  # the squares' sum stays inside fp32
            ref, bar = tc.rms64(x, w, tc.EPS, out_f32)
            assert bool(torch.isfinite(ref).all())
            ok, ratio, where = rc.within(tc.emulate_rms(x, w, tc.EPS, out_f32), ref, bar)
            worst[family] = ratio
            assert ok and ratio <= 1.0, f"rmsnorm out_f32={out_f32}, {family}, d = {d}: {ratio:.2f} x the worst case at {where}"
        print(f"T5 EMULATION rmsnorm d={d} out_f32={out_f32}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("mutant", list(tc.RMS_MUTANTS))
def test_every_rmsnorm_mutant_fails_some_row(mutant):
    caught = 0.0
    for d in tc.RMS_WIDTHS:
        w = rc.gains(d, 1)[0]
        for out_f32 in (False, True):
            for family, x in tc.rms_families(d).items():
                ref, bar = tc.rms64(x, w, tc.EPS, out_f32)
                ok, ratio, _ = rc.within(tc.emulate_rms(x, w, tc.EPS, out_f32, mutant), ref, bar)
                if not ok:
                    caught = max(caught, ratio)
    print(f"T5 MUTANT rmsnorm {mutant}: worst ratio {caught:.1f}")
    assert caught >= 3.0 * tc.MARGIN, f"mutant '{mutant}' ({tc.RMS_MUTANTS[mutant]}) is not caught"


def test_rms_depth_counts_the_kernels_structure():
    assert [tc.rms_depth(d) for d in (64, 1024, 1088, 4096)] == [15, 15, 20, 30]


# ------------------------------------------------------------------------------------------------ GEGLU
@pytest.mark.parametrize("rows,dff", tc.GEGLU_SHAPES[:2])
def test_emulated_geglu_is_within_the_worst_case(rows, dff):
    gf = tc.geglu_rows(rows, dff)
    g = gf[:, :dff].float()
    assert float(g.min()) == -12.0 and float(g.max()) == 12.0 and bool((g == 0).any()) and bool(torch.signbit(g[g == 0]).any())
    ref, bar = tc.geglu64(gf)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) < 2.0 ** 30
    ok, ratio, where = rc.within(tc.emulate_geglu(gf), ref, bar)
    print(f"T5 EMULATION geglu {rows}x{dff}: {ratio:.2f} x the worst case")
    assert ok and ratio <= 1.0, (ratio, where)
    # the absolute term is what carries the negative tail: without it the same output fails
    tight = tc.U * ref.abs() + 4.0 * tc.U32 * ref.abs()
    assert not rc.within(tc.emulate_geglu(gf), ref, tight)[0]


@pytest.mark.parametrize("mutant", list(tc.GEGLU_MUTANTS))
def test_every_geglu_mutant_fails(mutant):
    gf = tc.geglu_rows(3, 10240)
    ref, bar = tc.geglu64(gf)
    ok, ratio, _ = rc.within(tc.emulate_geglu(gf, mutant), ref, bar)
    print(f"T5 MUTANT geglu {mutant}: ratio {ratio:.1f}")
    assert not ok and ratio >= 3.0 * tc.MARGIN


def test_grid_stride_shapes_reach_the_second_iteration():
    rows, dff = tc.GEGLU_SHAPES[-1]
    assert rows * dff // 8 > 4096 * 256 and rows <= 1024 and dff <= 10240
    assert tc.ADD_SIZES[-1] // 8 > 4096 * 256 and all(n % 8 == 0 for n in tc.ADD_SIZES)


# ------------------------------------------------------------------------------------------------ embed, add
def test_embed_and_add_cases_hold_the_edges():
    for d in tc.EMBED_WIDTHS:
        ids, table, want = tc.embed_case(d)
        assert ids.dtype == torch.int32 and {0, 49, -1, 50, tc.INT_MAX, tc.INT_MIN} <= set(ids.tolist())
        assert torch.equal(want[2], table[0].float()) and torch.equal(want[4], table[49].float()) and torch.equal(want[63], table[0].float())
        assert not torch.equal(table[0], table[1])
    x, y, want = tc.add_case(8 * 1000)
    assert torch.equal(want.double(), (x.double() + y.double()).float().double())                  # one correctly rounded fp32 addition


# ------------------------------------------------------------------------------------------------ the encoder chain
def test_encoder_chain_restates_the_oracle_and_its_native_form_is_close():
    from oracle import t5_oracle as to
    cfg = dict(to.TINY_T5)
    w = to.make_t5_weights(cfg, seed=0)
    ids, mask = to.t5_inputs(cfg, L=48, lens=(29, 48))
    ref = to.encoder(w, ids[1:2], mask[1:2], cfg)[0]
    assert float((tc.encoder_chain(w, ids[1], cfg, torch.float32) - ref).abs().max()) <= 1e-4
    gold = tc.encoder_chain(w, ids[1], cfg)
    err = tc.rel_l2(tc.encoder_chain(w, ids[1], cfg, torch.float32, native=True), gold)
    assert 1e-4 < err < 1e-2, err
    deep = dict(cfg, **tc.DEEP_T5)
    wd = tc.bf16_checkpoint(to.make_t5_weights(deep, seed=5))
    assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in wd.values())
    assert not torch.equal(to.make_t5_weights(deep, seed=5)["norm.weight"], wd["norm.weight"])     # why the helper exists
    idd, _ = to.t5_inputs(deep, seed=13, L=tc.DEEP_TEXT_LEN, lens=tc.DEEP_LENS)
    for b, n in enumerate(tc.DEEP_LENS):
        e = tc.rel_l2(tc.encoder_chain(wd, idd[b, :n], deep, torch.float32, native=True), tc.encoder_chain(wd, idd[b, :n], deep))
        print(f"T5 DEEP 24 layers of TINY_T5, {n} tokens: bf16-rounding emulation vs the fp64 chain rel-L2 {e:.3e}")
        assert e < 5e-2


# ------------------------------------------------------------------------------------------------ binding and refusals
def test_binding_has_the_unit_entry_points():
    from realtime_video_amd import _lib
    P = _lib.T5_UNITS_PROTOTYPES
    vp, i, st = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    assert P == {"rtv_t5_embed": (i, [vp, vp, vp, i, i, i, i, st]),
                 "rtv_t5_rmsnorm": (i, [vp, vp, vp, i, i, ctypes.c_float, i, st]),
                 "rtv_t5_add": (i, [vp, vp, ctypes.c_size_t, st]),
                 "rtv_t5_geglu": (i, [vp, vp, i, i, st]),
                 "rtv_t5_attention": (i, [vp, vp, vp, vp, i, i, i, i, st])}
    lib = _lib.load()
    for name, (restype, argtypes) in P.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert not set(P) & set(_lib.PROTOTYPES)                           # a header of its own: rtv_hip.h is unchanged
    text = open(os.path.join(ROOT, "realtime_video_amd", "csrc", "Makefile")).read()
    assert "../../include/rtv_hip_t5_units.h" in text


def test_launchers_refuse_bad_arguments_before_any_launch():
    from realtime_video_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def refused(what, status):
        msg = lib.rtv_last_error().decode()
        assert status != 0 and what in msg, (what, status, msg)

    refused("t5_embed: null", lib.rtv_t5_embed(None, p, p, 32, 1, 64, 10, None))
    refused("t5_embed: need rows", lib.rtv_t5_embed(p, p, p, 32, 33, 64, 10, None))
    refused("t5_embed: dim", lib.rtv_t5_embed(p, p, p, 32, 1, 60, 10, None))
    refused("t5_embed: table and x", lib.rtv_t5_embed(p, p, odd, 32, 1, 64, 10, None))
    refused("t5_rmsnorm: null", lib.rtv_t5_rmsnorm(p, None, p, 1, 64, 1e-6, 0, None))
    refused("t5_rmsnorm: need rows", lib.rtv_t5_rmsnorm(p, p, p, 1, 66, 1e-6, 0, None))
    refused("t5_rmsnorm: out_f32", lib.rtv_t5_rmsnorm(p, p, p, 1, 64, 1e-6, 2, None))
    refused("t5_rmsnorm: x must", lib.rtv_t5_rmsnorm(odd, p, p, 1, 64, 1e-6, 0, None))
    refused("t5_rmsnorm: x must", lib.rtv_t5_rmsnorm(p, p, ctypes.c_void_p(base + 8), 1, 64, 1e-6, 1, None))
    refused("t5_add: n must", lib.rtv_t5_add(p, p, 12, None))
    refused("t5_add: x and y", lib.rtv_t5_add(p, odd, 8, None))
    refused("t5_geglu: need rows", lib.rtv_t5_geglu(p, p, 1, 68, None))
    refused("t5_geglu: gf and h", lib.rtv_t5_geglu(odd, p, 1, 64, None))
    refused("t5_attention: rows", lib.rtv_t5_attention(p, p, p, p, 48, 48, 1, 64, None))
    refused("t5_attention: need 0 < valid", lib.rtv_t5_attention(p, p, p, p, 64, 65, 1, 128, None))
    refused("t5_attention: need 0 < valid", lib.rtv_t5_attention(p, p, p, p, 64, 0, 1, 128, None))
    refused("t5_attention: need 0 < valid", lib.rtv_t5_attention(p, p, p, p, 64, 49, 1, 48, None))
    refused("t5_attention: num_heads", lib.rtv_t5_attention(p, p, p, p, 64, 48, 0, 48, None))
    refused("t5_attention: qk must", lib.rtv_t5_attention(odd, p, p, p, 64, 48, 1, 48, None))
    refused("t5_attention: null", lib.rtv_t5_attention(p, p, p, None, 64, 48, 1, 48, None))
