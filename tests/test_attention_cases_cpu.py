"""CPU checks of tests/attn_cases.py: what the builders promise, that an emulation of the attention kernels' arithmetic passes
`within_bound` on every input of tests/test_attention_peaked_gpu.py, and that mutants of the emulation - the single-key errors
the peaked inputs exist to expose - fail it by a factor of at least 3.  The mutants are what shows that the GPU tests can fail.
"""
import math

import pytest
import torch

import attn_cases as ac

DTYPES = [torch.bfloat16, torch.float16]
MUTANT_FACTOR = 3.0          # a mutant's worst ratio must reach 3 x the bar, i.e. 12 in units of u * ref_abs


def _ids(dt):
    return str(dt).replace("torch.", "")


@pytest.fixture(scope="module")
def specs():
    cache = {}

    def _get(dtype):
        if dtype not in cache:
            cache[dtype] = list(ac.all_specs(dtype))
        return cache[dtype]
    return _get


def _emulate(spec, slack=8.0, **kw):
    k, v = spec.window()
    return ac.emulate(spec.q, k, v, spec.dtype, spec.mask(), spec.bias(), slack, **kw)


def _ratio(spec, out):
    ref, ref_abs = spec.reference()
    return ac.within_bound(out, ref, ref_abs, spec.dtype)


# ------------------------------------------------------------------------------------------------ builder promises
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_builders_keep_their_promises(specs, dtype):
    """Target weight >= 1 - 1e-5 in fp64, a lead of at least 12 nats over the best other visible key, no scaled score beyond
    80 nats (the fp32 exponent has room) - for every input of the GPU file; and a decoy row, were it read, would beat the key it is
    matched to by at least 12 nats."""
    worst = {"weight": 1.0, "lead": math.inf, "score": 0.0, "decoy": math.inf, "floor": 0.0}
    for spec in specs(dtype):
        k, _ = spec.window()
        s = ac.scores64(spec.q, k, ac.SCALE, spec.mask(), spec.bias())                     # [B, H, Lq, Lkv]
        B, H, Lq, Lkv = s.shape
        T = spec.answer or spec.targets.shape[-1]
        tg = spec.targets[..., :T].permute(1, 0, 2).unsqueeze(0).expand(B, -1, -1, -1)     # [B, H, Lq, T]
        hit = torch.zeros_like(s, dtype=torch.bool).scatter_(-1, tg, True)
        p = torch.softmax(s, -1)
        weight = float((p * hit).sum(-1).min())
        lead = float((s.masked_fill(~hit, -math.inf).amax(-1) - s.masked_fill(hit, -math.inf).amax(-1)).min()) if Lkv > T else math.inf
        top = float(s.masked_fill(torch.isinf(s), 0).abs().max())
        if dtype == torch.float16:
            # an f16 P below 2^-14 of the reference point (at worst the row maximum itself) is subnormal or flushed: an absolute
            # error of min(P, 2^-25) per key that `u * ref_abs` does not cover.  No single key's term may take more than half of
            # the 1e-6 floor of the bound (a decoy row of 100s that other rows see as an ordinary key would: 3e-6); the signed sum
            # over the N(0, 1) rows is what the emulation test below measures.
            _, v = spec.window()
            rel = torch.exp(s - s.amax(-1, keepdim=True))
            lost = torch.where(rel < 2.0 ** -14, rel.clamp(max=2.0 ** -25), torch.zeros_like(rel))
            worst["floor"] = max(worst["floor"], float((lost * v.double().abs().amax(-1).permute(0, 2, 1).unsqueeze(2)).max()))
        kc, _ = spec.caches()
        for row, t in spec.decoy_rows:                         # a decoy, if read, beats the key it is matched to by >= 12 nats
            sd = torch.einsum("bqhd,bhd->bhq", spec.q.double(), kc[:, row].double()) * ac.SCALE
            st = torch.einsum("bqhd,bhd->bhq", spec.q.double(), k[:, t].double()) * ac.SCALE
            mine = (spec.targets[..., 0] == t).t().unsqueeze(0).expand_as(sd)
            if bool(mine.any()):
                worst["decoy"] = min(worst["decoy"], float((sd - st)[mine].min()))
        assert weight >= 1 - 1e-5, f"{spec.name}: target weight {weight}"
        assert lead >= 12.0, f"{spec.name}: lead {lead:.2f} nats"
        assert top <= 80.0, f"{spec.name}: score {top:.1f} nats"
        worst.update(weight=min(worst["weight"], weight), lead=min(worst["lead"], lead), score=max(worst["score"], top))
    assert worst["decoy"] >= 12.0 and worst["floor"] <= 5e-7
    print(f"BUILDERS {_ids(dtype)}: smallest target weight {worst['weight']:.8f}, smallest lead {worst['lead']:.2f} nats, "
          f"largest |score| {worst['score']:.1f} nats, smallest lead of a decoy over the key it shadows {worst['decoy']:.2f} nats, "
          f"largest single-key f16 subnormal-P term {worst['floor']:.2e}")


def test_builder_references_are_the_known_answers():
    """one_hot answers v[target]; tie answers the mean of the tied V rows; the counted tie answers (v_a + n v_dup) / (n + 1)."""
    c = ac.one_hot(300, 200, 2, 1, torch.bfloat16, perm_seed=1)
    ref, _ = ac.attn_ref64(c.q, c.k, c.v)
    want = ac._gather_keys(c.v.double(), c.targets[..., 0])
    assert float((ref - want).abs().max()) <= 1e-5
    assert all(len(set(c.targets[:200, h, 0].tolist())) == 200 for h in range(2))      # Lq >= Lkv: every key is a target
    t = ac.tie(64, 200, [(3, 70, 199)], 2, 1, torch.bfloat16)
    ref, _ = ac.attn_ref64(t.q, t.k, t.v)
    assert float((ref - t.v[:, [3, 70, 199]].double().mean(1, keepdim=True)).abs().max()) <= 1e-5
    s = ac.spec_counted("tie", 63, 63, 7)
    ref, _ = s.reference()
    a = int(s.targets[0, 0, 1])
    want = (s.v_base[:, a].double() + 7 * s.v_base[:, 63].double()) / 8
    assert float((ref - want.unsqueeze(1)).abs().max()) <= 1e-5


def test_staircase_maximum_jumps_late_and_early():
    c = ac.staircase(300, 1100, 2, 1, torch.bfloat16, seed=1100)
    s = ac.scores64(c.q, c.k)[0]                                                       # [H, Lq, Lkv] nats
    got = torch.gather(s, -1, c.targets.permute(1, 0, 2))                              # by falling gain
    assert float((got - torch.tensor([64.0, 48.0, 32.0, 16.0])).abs().max()) <= 0.5    # 16-bit rounding of q
    tile_max = torch.stack([s[..., j:j + ac.KT].amax(-1) for j in range(0, 1100, ac.KT)], -1) * math.log2(math.e)
    run = torch.cummax(tile_max, -1).values
    jumps = ((run[..., 1:] - run[..., :-1]) > 8).sum(-1)                               # rescales after the first tile
    assert int(jumps[:, 0::2].min()) >= 2 and int(jumps[:, 1::2].max()) == 0
    assert bool((c.targets[0::2, :, 0] >= 1088).all()) and bool((c.targets[1::2, :, 0] < 64).all())


# ------------------------------------------------------------------------------------------------ emulation
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_emulated_kernel_arithmetic_is_within_the_bound(specs, dtype):
    """16-bit P, fp32 row sum of the unrounded exponentials, reference point 8 below (and, second run, at) the row maximum in the
    log2 domain; the split inputs also through the split emulation and its merge."""
    worst = {}
    for spec in specs(dtype):
        runs = [("slack8", _emulate(spec, 8.0)), ("slack0", _emulate(spec, 0.0))]
        if spec.name.startswith("split"):
            S = int(spec.name.rsplit("S", 1)[1].rstrip("]"))
            runs.append(("split", _emulate(spec, 8.0, ranges=ac.split_ranges(spec.Lkv, S))))
        for tag, out in runs:
            ok, ratio, idx = _ratio(spec, out)
            fam = spec.name.split("[")[0]
            worst[fam] = max(worst.get(fam, 0.0), ratio)
            assert ok, f"{spec.name} {tag}: ratio {ratio:.2f} at (batch, row, head, dim) {idx}"
    print(f"EMULATION {_ids(dtype)}: largest |out - ref| / (u ref_abs) per family: " +
          ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= ac.BOUND_FACTOR


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_emulation_on_diffuse_data_uses_a_fraction_of_the_bound(dtype):
    spec = ac.spec_gaussian(dtype=dtype)
    ok, ratio, _ = _ratio(spec, _emulate(spec))
    print(f"EMULATION {_ids(dtype)} gaussian 520x1100: ratio {ratio:.3f} of a bar of {ac.BOUND_FACTOR}")
    assert ok and ratio <= 2.0            # the derived worst case, without the margin


# ------------------------------------------------------------------------------------------------ mutants
def _mutant_window(spec, seg0, seg1):
    """The emulation reading other cache rows than the window's."""
    m = ac.Spec(spec.name, spec.q, spec.k_base, spec.v_base, seg0, seg1)
    k, v = m.window()
    return ac.emulate(spec.q, k, v, spec.dtype)


def _mutants(dtype):
    causal = ac.spec_causal(300, 520, 96, 37, dtype)
    k, v = causal.window()
    lim = ac.causal_limits(300, 520, 96, 37).view(1, 1, -1, 1)
    kv = torch.arange(520).view(1, 1, 1, -1)
    yield "limit <= for <", causal, ac.emulate(causal.q, k, v, dtype, kv <= lim)
    yield "limit minus one", causal, ac.emulate(causal.q, k, v, dtype, kv < lim - 1)
    far = ac.spec_causal(300, 520, 96, 37, dtype, far=True)
    k, v = far.window()
    yield "limit <= for <, target far from the limit", far, ac.emulate(far.q, k, v, dtype, kv <= lim)
    for Lq, Lkv in ((257, 65), (520, 1100)):
        out = ac.spec_outside(Lq, Lkv, dtype)
        yield f"window longer by one row ({Lkv} keys)", out, _mutant_window(out, (3, Lkv + 1), (0, 0))
        yield f"window shorter by one row ({Lkv} keys)", out, _mutant_window(out, (3, Lkv - 1), (0, 0))
        yield f"window one row early ({Lkv} keys)", out, _mutant_window(out, (2, Lkv), (0, 0))
    ring = ac.spec_two_ranges((3, 77), (200, 1003), dtype=dtype)
    yield "second range starting one row early", ring, _mutant_window(ring, (3, 77), (199, 1003))
    yield "first range longer by one row", ring, _mutant_window(ring, (3, 78), (200, 1002))
    for n in (2, 3, 7):
        tied = ac.spec_counted("tie", 63, 63, n, dtype=dtype)
        k, v = tied.window()
        b = tied.bias()
        yield f"counted key n + 1, n = {n}", tied, ac.emulate(tied.q, k, v, dtype, bias=b * math.log(n + 1) / math.log(n))
        yield f"counted key n - 1, n = {n}", tied, ac.emulate(tied.q, k, v, dtype, bias=b * (math.log(n - 1) / math.log(n)))
        yield f"counted key natural log for log2, n = {n}", tied, ac.emulate(tied.q, k, v, dtype, bias_log2=b)
    beside = ac.spec_counted("beside", 200, 200, 7, dtype=dtype)
    k, v = beside.window()
    leak = beside.bias().clone()
    leak[..., int(beside.targets[0, 0, 0])] = leak[..., 200]               # the even rows' real target gets + log n as well
    yield "counted key's log n leaking into the target's column", beside, ac.emulate(beside.q, k, v, dtype, bias=leak)
    hot = ac.spec_split("one_hot", 1100, 5, dtype=dtype)
    k, v = hot.window()
    vs = v.clone()
    vs[:, [3 * 64 + 16 + 1, 3 * 64 + 16 + 9]] = v[:, [3 * 64 + 16 + 9, 3 * 64 + 16 + 1]]
    yield "two V rows of one 16-key step swapped", hot, ac.emulate(hot.q, k, vs, dtype)
    rg = ac.split_ranges(1100, 5)
    yield "combine weights with the maxima of two ranges exchanged", hot, ac.emulate(hot.q, k, v, dtype, ranges=rg, swap_maxima=(1, 3))
    yield "a split range that drops its last key", hot, ac.emulate(hot.q, k, v, dtype, ranges=[(lo, hi - (i == 1)) for i, (lo, hi) in enumerate(rg)])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_mutants_fail_the_bound_by_a_factor_of_three(dtype):
    rows = []
    for name, spec, out in _mutants(dtype):
        ok, ratio, idx = _ratio(spec, out)
        rows.append((name, ratio, ok, idx))
        print(f"MUTANT {_ids(dtype)} {name}: ratio {ratio:.1f} = {ratio / ac.BOUND_FACTOR:.1f} x the bar, worst (batch, row, head, dim) {idx}")
    for name, ratio, ok, _ in rows:
        assert not ok and ratio >= MUTANT_FACTOR * ac.BOUND_FACTOR, f"mutant '{name}' is not caught: ratio {ratio:.2f}"


def test_within_bound_reports_the_worst_element_and_refuses_nan():
    ref = torch.ones(1, 3, 2, 4, dtype=torch.float64)
    out = ref.clone()
    assert ac.within_bound(out, ref, ref, torch.bfloat16)[0]
    out[0, 2, 1, 3] += 5 * 2.0 ** -8
    ok, ratio, idx = ac.within_bound(out, ref, ref, torch.bfloat16)
    assert not ok and idx == (0, 2, 1, 3) and abs(ratio - 5.0) < 1e-3
    out[0, 2, 1, 3] = 1 + 3.9 * 2.0 ** -8
    assert ac.within_bound(out, ref, ref, torch.bfloat16)[0] and not ac.within_bound(out, ref, ref, torch.float16)[0]
    out[0, 1, 0, 0] = math.nan
    ok, ratio, idx = ac.within_bound(out, ref, ref, torch.bfloat16)
    assert not ok and math.isinf(ratio) and idx == (0, 1, 0, 0)
