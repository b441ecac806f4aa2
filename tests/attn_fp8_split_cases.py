"""Restatement of the KV split of the fp8 attention kernel (include/rtv_hip_attn_fp8_cp.h, "THE SPLIT") and the inputs of
tests/test_attn_fp8_split_gpu.py: the storage-tile list of a workgroup and its cut into ranges, the arithmetic of
attn_fp8_cases.emulate on the tiles of one range - left as the partial (m, l, unnormalised O) -, and the merge.  Plain torch.
tests/test_attn_fp8_split_cpu.py checks it, and three mutants of it, against the bound of tests/attn_fp8_cases.py on exactly the
inputs the kernel gets."""
import math
from dataclasses import replace

import torch

import attn_cases as ac
import attn_fp8_cases as fc
from attn_cases import KT, SCALE

QT = 256                       # query rows per workgroup of attn_fwd_fp8_kernel
SPLITS = (2, 3, 5, 16)
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------------------ the tile rule
def tile_list(seg0, seg1, limit=None):
    """Storage tiles a workgroup walks: those of [row0, row0 + limit) (limit: its largest causal key limit, default n0), then those
    of [row1, row1 + n1).  -> [(tile, first physical row, end physical row, key index of the first row)], rows clipped to the tile."""
    (r0, n0), (r1, n1) = seg0, seg1
    out, base = [], 0
    for a, b, nb in ((r0, r0 + (n0 if limit is None else limit), n0), (r1, r1 + n1, n1)):
        if b > a:
            for T in range(a >> 6, ((b - 1) >> 6) + 1):
                lo = max(a, T * KT)
                out.append((T, lo, min(b, (T + 1) * KT), base + lo - a))
        base += nb
    return out


def window_tiles(seg0, seg1):
    """Storage tiles the window touches: what rtv_attn_fwd_fp8_split clamps kv_splits to."""
    return len(tile_list(seg0, seg1))


def clamp_splits(seg0, seg1, S):
    return max(1, min(S, window_tiles(seg0, seg1)))


def split_tile_range(ntiles, s, S, d_hi=0):
    """Tiles [ntiles s / S, ntiles (s + 1) / S) of a workgroup's list.  d_hi: the mutant that moves every inner boundary's END by
    d_hi tiles (-1: the boundary tile is dropped, +1: it is worked on twice)."""
    lo, hi = ntiles * s // S, ntiles * (s + 1) // S
    if s < S - 1:
        hi = max(lo, min(ntiles, hi + d_hi))
    return lo, hi


def key_ranges(seg0, seg1, S):
    """(first key, last key) of the window per range of a dense launch (every workgroup has the whole list); None: an empty range."""
    tiles = tile_list(seg0, seg1)
    S = clamp_splits(seg0, seg1, S)
    out = []
    for s in range(S):
        lo, hi = split_tile_range(len(tiles), s, S)
        out.append((tiles[lo][3], tiles[hi - 1][3] + tiles[hi - 1][2] - tiles[hi - 1][1] - 1) if hi > lo else None)
    return out


# ------------------------------------------------------------------------------------------------ emulation
def emulate_partial(launch, k8, v8t, rows, tiles, slack=8.0):
    """attn_fp8_cases.emulate's arithmetic for the query rows `rows` (a slice) on the storage tiles `tiles` (entries of tile_list),
    stopped in front of the normalisation -> (m [H, q], l [H, q], O [q, H, D]) fp32; m in each row's scaled log2 domain.  No tile,
    or a row that sees no key of them: (-1e30, 0, 0)."""
    dev = k8.device
    q = launch.q[rows].to(dev)
    nq, H = q.shape[0], q.shape[1]
    if not tiles:
        return torch.full((H, nq), -1e30), torch.zeros(H, nq), torch.zeros(nq, H, ac.D)
    phys = torch.cat([torch.arange(T * KT, (T + 1) * KT, device=dev) for T, _, _, _ in tiles])
    lo = torch.tensor([a for _, a, _, _ in tiles], device=dev).repeat_interleave(KT)
    hi = torch.tensor([b for _, _, b, _ in tiles], device=dev).repeat_interleave(KT)
    base = torch.tensor([kb for _, _, _, kb in tiles], device=dev).repeat_interleave(KT)
    inside = (phys >= lo) & (phys < hi)
    key = phys - lo + base
    qc, s_q = fc.quantize_q(q)
    kcodes = fc.decode(k8[phys.clamp(max=launch.cache_rows - 1)]).float()
    vcodes = fc.decode(fc.gather_v(v8t, phys)).float()
    vcodes = torch.where(inside.view(-1, 1, 1), vcodes, torch.zeros_like(vcodes))
    c = s_q * torch.tensor(SCALE * fc.LOG2E * launch.k_scale, dtype=torch.float32)
    s = torch.einsum("qhd,khd->hqk", fc.decode(qc).float(), kcodes) * c.permute(1, 0, 2)
    lim = launch.limits()[rows].to(dev)
    vis = inside.view(1, 1, -1) & (key.view(1, 1, -1) < lim.view(1, -1, 1))
    s = torch.where(vis, s, torch.full_like(s, -math.inf))
    mx = s.amax(-1)
    m = torch.where(torch.isinf(mx), torch.full_like(mx, -1e30), mx - slack)
    p = torch.exp2(s - m.unsqueeze(-1))
    return m, p.sum(-1), torch.einsum("hqk,khd->qhd", p.to(fc.E4M3).float(), vcodes)


def emulate_split(launch, k8, v8t, S, slack=8.0, unit_weights=False, d_hi=0, apply_v_scale=True):
    """The split launch: per workgroup (256 query rows) its own tile list, cut into the clamped S ranges, emulate_partial per range,
    then the merge m = max m_s, w_s = 2^(m_s - m), O = v_scale sum w_s O_s / sum w_s l_s, rounded once to bf16.
    Mutants: unit_weights (w_s = 1), d_hi (split_tile_range), apply_v_scale=False."""
    Lq = launch.q.shape[0]
    S = clamp_splits(launch.seg0, launch.seg1, S)
    lim = launch.limits()
    out = torch.empty(launch.q.shape, dtype=BF16)
    for q0 in range(0, Lq, QT):
        rows = slice(q0, min(q0 + QT, Lq))
        tiles = tile_list(launch.seg0, launch.seg1, int(lim[rows].max()) if launch.causal_block > 0 else None)
        parts = [emulate_partial(launch, k8, v8t, rows, tiles[slice(*split_tile_range(len(tiles), s, S, d_hi))], slack) for s in range(S)]
        ms = torch.stack([p[0] for p in parts])
        w = torch.ones_like(ms) if unit_weights else torch.exp2(ms - ms.amax(0))
        l = sum(w[i] * parts[i][1] for i in range(S))
        o = sum(w[i].permute(1, 0).unsqueeze(-1) * parts[i][2] for i in range(S))
        vs = torch.tensor(launch.v_scale if apply_v_scale else 1.0, dtype=torch.float32)
        out[rows] = (o * (vs / l).permute(1, 0).unsqueeze(-1)).to(BF16).cpu()
    return out


# ------------------------------------------------------------------------------------------------ the inputs of the GPU file
WINDOWS = [((37, 200), (0, 0)), ((3, 1100), (0, 0)), ((600, 500), (2, 300)), ((1000, 1), (10, 130))]
FAMILIES = ("one_hot", "tie2", "tie3", "staircase")
LQ = 300                                                   # two query tiles, the second one partial
CAUSAL = [(520, 1100, cb, off) for cb in (96, 520) for off in (0, 37, 580)]
HEAD_MAPS = (5, 8)                                          # H % 8 != 0 and == 0: the two workgroup -> head maps


def _place(name, case, seg0, seg1):
    """A Spec whose cache holds the window of `case` at seg0 + seg1 and zeros elsewhere (the GPU test poisons the rest)."""
    (r0, n0), (r1, n1) = seg0, seg1
    B, _, H, _ = case.k.shape
    kc = torch.zeros(B, max(r0 + n0, r1 + n1) + KT + 8, H, ac.D, dtype=case.k.dtype)
    vc = torch.zeros_like(kc)
    kc[:, r0:r0 + n0], vc[:, r0:r0 + n0] = case.k[:, :n0], case.v[:, :n0]
    if n1:
        kc[:, r1:r1 + n1], vc[:, r1:r1 + n1] = case.k[:, n0:], case.v[:, n0:]
    return ac.Spec(name, case.q, kc, vc, seg0, seg1, targets=case.targets)


def spec_window(family, seg0, seg1, S, H=2):
    """one_hot: the first and the last key of every range are some query's target.  tie2 / tie3: bit-identical keys in two / three
    different ranges (first, middle, last).  staircase: attn_cases.staircase over the window.  None: the window cannot hold it (a
    staircase needs four key tiles, tie3 three non-empty ranges)."""
    Lkv = seg0[1] + seg1[1]
    rg = [r for r in key_ranges(seg0, seg1, S) if r is not None]
    name = f"split8[{family},{seg0}+{seg1},S{S},H{H}]"
    if family == "one_hot":
        case = ac.one_hot(LQ, Lkv, H, 1, BF16, perm_seed=500 + Lkv + S, cover=[e for r in rg for e in r])
    elif family == "staircase":
        if (Lkv + KT - 1) // KT < 4:
            return None
        case = ac.staircase(LQ, Lkv, H, 1, BF16, seed=Lkv + S)
    else:
        n = 3 if family == "tie3" else 2
        if len(rg) < n:
            return None
        pick = [rg[0], rg[len(rg) // 2], rg[-1]] if n == 3 else [rg[0], rg[-1]]
        groups = [tuple(min(lo + 5, hi) for lo, hi in pick), tuple(hi for lo, hi in pick)]
        case = ac.tie(LQ, Lkv, groups, H, 1, BF16, seed=Lkv + S)
    return _place(name, case, seg0, seg1)


def all_cases():
    """(spec, S) of every launch of the GPU file."""
    for seg0, seg1 in WINDOWS:
        for family in FAMILIES:
            for S in SPLITS:
                spec = spec_window(family, seg0, seg1, S)
                if spec is not None:
                    yield spec, S
    for Lq, Lkv, cb, off in CAUSAL:
        spec = ac.spec_causal(Lq, Lkv, cb, off, BF16)
        for S in SPLITS:
            yield spec, S
    for H in HEAD_MAPS:
        yield spec_window("one_hot", (3, 1100), (0, 0), 3, H), 3
    for S in SPLITS:
        yield ac.spec_gaussian(), S
