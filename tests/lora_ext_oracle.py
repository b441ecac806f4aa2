"""float64 oracles of the extended LoRA merges (include/rtv_hip_lora_ext.h), their torch fp32 emulations, and the synthetic
adapters the parser and model tests share.  The criterion is lora_oracle.criterion: |W - ref| <= half a bf16 ulp of ref +
2^-16 * mag, and at least 99.9 % of the elements equal bf16(ref).

Dense form     ref = base + sum_t (scale_t * B_t @ A_t + diff_scale_t * diff_t)
               mag = |base| + sum_t (|scale_t| * |B_t| @ |A_t| + |diff_scale_t| * |diff_t|)
DoRA           V = base + factor * B @ A,  g[n] = mag_vec[n] / ||V[n]||_2 (over the input width),  ref = base + strength * (g V - base)
               mag = |base| + |strength| * (|g| * (|base| + |factor| * |B| @ |A|) + |base|)
               a row with ||V[n]|| == 0, or strength == 0, is base.

No published adapter file was at hand: the key styles below restate the trainers' conventions (kohya / musubi-tuner, diffusers /
PEFT, ComfyUI's `.diff` / `.diff_b`, LyCORIS / PEFT DoRA) on synthetic tensors."""
import re

import torch

import lora_oracle as lo

BF = torch.bfloat16
DIFF_STD = 0.01
# N, K, rank, strength
SHAPES = [(72, 136, 4, 1.0), (160, 392, 80, 0.7), (128, 512, 256, -0.5), (64, 13824, 16, 1.0), (72, 136, 24, 0.25)]


def make_inputs(N, K, ranks, seed):
    """lora_oracle.make_inputs with the rows of base and of every B scaled by 2^(n % 5) (a norm taken over the wrong axis is then
    an O(1) error), plus mag = bf16(||base||_row * (1 + 0.1 N(0,1))) and diff ~ 0.01 N(0,1): (base, [(A, B)], mag, diff)."""
    base, ab = lo.make_inputs(N, K, ranks, seed)
    rows = torch.exp2((torch.arange(N) % 5).float())[:, None]
    base = (base.float() * rows).to(BF)
    ab = [(A, (B.float() * rows).to(BF)) for A, B in ab]
    g = torch.Generator().manual_seed(seed + 1000)
    mag = (base.double().norm(dim=1) * (1 + 0.1 * torch.randn(N, generator=g).double())).to(BF)
    diff = (DIFF_STD * torch.randn(N, K, generator=g)).to(BF)
    return base, ab, mag, diff


def _d(x):
    return x.detach().cpu().double()


def merge_ex_oracle(base, terms):
    """terms [(A, B, scale, diff, diff_scale)], A / B or diff may be None -> (ref, mag), float64."""
    ref = _d(base)
    mag = ref.abs()
    for A, B, scale, diff, diff_scale in terms:
        if A is not None:
            ref = ref + float(scale) * (_d(B) @ _d(A))
            mag = mag + abs(float(scale)) * (_d(B).abs() @ _d(A).abs())
        if diff is not None:
            ref = ref + float(diff_scale) * _d(diff)
            mag = mag + abs(float(diff_scale)) * _d(diff).abs()
    return ref, mag


def dora_oracle(base, A, B, factor, mag_vec, strength):
    base, A, B, m = _d(base), _d(A), _d(B), _d(mag_vec).reshape(-1)
    V = base + float(factor) * (B @ A)
    nrm = V.norm(dim=1)
    g = torch.where(nrm > 0, m / nrm.clamp(min=1e-300), torch.zeros_like(nrm))[:, None]
    live = (nrm > 0)[:, None] & (float(strength) != 0.0)
    ref = torch.where(live, base + float(strength) * (g * V - base), base)
    mag = base.abs() + abs(float(strength)) * (g.abs() * (base.abs() + abs(float(factor)) * (B.abs() @ A.abs())) + base.abs())
    return ref, mag


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def ex_emulation(base, terms):
    """The kernel's arithmetic in torch fp32: the scaled low-rank sums in term order, then the scaled diffs in term order, one
    rounding; a zero total keeps the bits of base."""
    tot = torch.zeros(base.shape, dtype=torch.float32)
    for A, B, scale, _, _ in terms:
        if A is not None:
            tot = tot + _f32(scale) * (B.float() @ A.float())
    dsum = torch.zeros(base.shape, dtype=torch.float32)
    for _, _, _, diff, diff_scale in terms:
        if diff is not None:
            dsum = dsum + _f32(diff_scale) * diff.float()
    tot = tot + dsum
    return torch.where(tot == 0, base, (base.float() + tot).to(BF))


def dora_emulation(base, A, B, factor, mag_vec, strength, tile=128):
    """The kernel's arithmetic in torch fp32: the row norm from `tile`-column partial sums (a pairwise tree inside a tile), the
    partials added in the kernel's fixed order."""
    N, K = base.shape
    b = base.float()
    V = b + _f32(factor) * (B.float() @ A.float())
    sq = torch.zeros(N, -(-K // tile) * tile, dtype=torch.float32)
    sq[:, :K] = V * V
    sq = sq.reshape(N, -1, tile)
    while sq.shape[-1] > 1:
        sq = sq[..., 0::2] + sq[..., 1::2]
    tiles = sq.shape[1]
    per = (tiles + 3) // 4
    runs = []
    for q in range(4):          # four runs of consecutive tiles, each in tile order, then the four sums in order
        run = torch.zeros(N, dtype=torch.float32)
        for t in range(q * per, min((q + 1) * per, tiles)):
            run = run + sq[:, t, 0]
        runs.append(run)
    total = ((runs[0] + runs[1]) + runs[2]) + runs[3]
    nrm = total.sqrt()
    g = torch.where(nrm > 0, mag_vec.float().reshape(-1) / nrm, torch.zeros_like(nrm))[:, None]
    delta = _f32(strength) * (g * V - b)
    keep = (delta == 0) | (nrm == 0)[:, None] | (float(strength) == 0.0)
    return torch.where(keep, base, (b + delta).to(BF))


# ------------------------------------------------------------------ synthetic adapters
LINEARS = ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o", "cross_attn.q", "cross_attn.k", "cross_attn.v", "cross_attn.o",
           "ffn.0", "ffn.2")
TOP_LINEARS = ("text_embedding.0", "text_embedding.2", "time_embedding.0", "time_embedding.2", "time_projection.1", "head.head")
NORMS = ("self_attn.norm_q", "self_attn.norm_k", "cross_attn.norm_q", "cross_attn.norm_k", "norm3")
PREFIXES = ("", "diffusion_model.", "model.diffusion_model.", "model.", "transformer.")
STYLES = ("canonical", "diffusers", "kohya")
# the diffusers Wan conversion, written out once more and independently of realtime_video_amd/lora.py
_TO_DIFFUSERS = [(r"\.self_attn\.", ".attn1."), (r"\.cross_attn\.", ".attn2."), (r"\.(attn[12])\.q$", r".\1.to_q"),
                 (r"\.(attn[12])\.k$", r".\1.to_k"), (r"\.(attn[12])\.v$", r".\1.to_v"), (r"\.(attn[12])\.o$", r".\1.to_out.0"),
                 (r"\.ffn\.0$", ".ffn.net.0.proj"), (r"\.ffn\.2$", ".ffn.net.2"), (r"^(blocks\.\d+)\.norm3$", r"\1.norm2"),
                 (r"^text_embedding\.0$", "condition_embedder.text_embedder.linear_1"),
                 (r"^text_embedding\.2$", "condition_embedder.text_embedder.linear_2"),
                 (r"^time_embedding\.0$", "condition_embedder.time_embedder.linear_1"),
                 (r"^time_embedding\.2$", "condition_embedder.time_embedder.linear_2"),
                 (r"^time_projection\.1$", "condition_embedder.time_proj"), (r"^head\.head$", "proj_out")]


def to_diffusers(target):
    for pat, rep in _TO_DIFFUSERS:
        target = re.sub(pat, rep, target)
    return target


def all_targets(num_layers=2):
    """(every Linear, every norm target) of a model with `num_layers` blocks, canonical names."""
    linears = list(TOP_LINEARS) + [f"blocks.{i}.{n}" for i in range(num_layers) for n in LINEARS]
    norms = [f"blocks.{i}.{n}" for i in range(num_layers) for n in NORMS]
    return linears, norms


def full_adapter(shapes, rank=4, seed=31, num_layers=2, dora=("blocks.0.self_attn.k", "blocks.1.cross_attn.v", "blocks.1.ffn.0"),
                 dense=("blocks.0.ffn.2", "blocks.1.self_attn.q", "head.head"), base=None):
    """A canonical-spelling adapter over every kind of target of `shapes` (CausalWanModel.state_dict_shapes()): a low-rank pair on
    every Linear (alpha = rank / 2 on the ffn, with B twice as large), `.diff_b` on every bias, `.diff` on every norm weight,
    `.diff_b` on norm3, a full-matrix `.diff` on the Linears of `dense`, a DoRA vector on those of `dora` (near the row norms of
    `base`, the model's state dict, when given).  Keys are `target.part` with part in A / B / alpha / diff / diff_b / dora:
    `spell` turns them into a key style."""
    g = torch.Generator().manual_seed(seed)
    linears, norms = all_targets(num_layers)
    sd = {}
    for t in linears:
        out_f, in_f = shapes[t + ".weight"]
        alpha = ".ffn." in t
        sd[t + ".A"] = (lo.AB_STD * torch.randn(rank, in_f, generator=g)).to(BF)
        sd[t + ".B"] = ((2 if alpha else 1) * lo.AB_STD * torch.randn(out_f, rank, generator=g)).to(BF)
        if alpha:
            sd[t + ".alpha"] = torch.tensor(rank / 2.0)
        sd[t + ".diff_b"] = (DIFF_STD * torch.randn(out_f, generator=g)).to(BF)
        if t in dense:
            sd[t + ".diff"] = (DIFF_STD * torch.randn(out_f, in_f, generator=g)).to(BF)
        if t in dora:
            rows = base[t + ".weight"].double().norm(dim=1) if base is not None else torch.full((out_f,), 0.02 * in_f ** 0.5).double()
            sd[t + ".dora"] = (rows * (1 + 0.1 * torch.randn(out_f, generator=g).double())).to(BF)
    for t in norms:
        d = shapes[t + ".weight"][0]
        sd[t + ".diff"] = (DIFF_STD * torch.randn(d, generator=g)).to(BF)
        if t.endswith("norm3"):
            sd[t + ".diff_b"] = (DIFF_STD * torch.randn(d, generator=g)).to(BF)
    return sd


def spell(adapter, style, prefix="", dora_key=None, column=False):
    """The adapter of full_adapter in a key style: "canonical" (lora_A / lora_B, PEFT's DoRA key), "diffusers" (the diffusers names,
    lora_A / lora_B, `.lora_magnitude_vector.weight`) or "kohya" (`lora_unet_` + flattened canonical name, lora_down / lora_up,
    `.dora_scale`).  column=True stores the DoRA vectors as [out, 1]."""
    parts = {"canonical": {"A": ".lora_A.weight", "B": ".lora_B.weight", "dora": ".lora_magnitude_vector"},
             "diffusers": {"A": ".lora_A.weight", "B": ".lora_B.weight", "dora": ".lora_magnitude_vector.weight"},
             "kohya": {"A": ".lora_down.weight", "B": ".lora_up.weight", "dora": ".dora_scale"}}[style]
    out = {}
    for key, v in adapter.items():
        target, part = key.rsplit(".", 1)
        name = {"canonical": target, "diffusers": to_diffusers(target), "kohya": "lora_unet_" + target.replace(".", "_")}[style]
        suffix = (dora_key if part == "dora" and dora_key else parts.get(part, "." + part))
        out[prefix + name + suffix] = v.reshape(-1, 1) if part == "dora" and column else v
    return out


def merged_state_dict(sd, adapter, scale):
    """{state-dict key: (ref, mag)} of the float64 merge of full_adapter's `adapter` at strength `scale` into the state dict `sd`,
    for every tensor the adapter touches."""
    out = {}
    targets = sorted({k.rsplit(".", 1)[0] for k in adapter})
    for t in targets:
        get = lambda part: adapter.get(f"{t}.{part}")          # noqa: E731
        A, B, alpha, diff, diff_b, dora = (get(p) for p in ("A", "B", "alpha", "diff", "diff_b", "dora"))
        w = sd[t + ".weight"]
        factor = float(alpha) / A.shape[0] if alpha is not None else 1.0
        if dora is not None:
            out[t + ".weight"] = dora_oracle(w, A, B, factor, dora, scale)
        elif A is not None or diff is not None:
            d2 = diff.reshape(1, -1) if diff is not None and w.ndim == 1 else diff
            ref, mag = merge_ex_oracle(w.reshape(1, -1) if w.ndim == 1 else w, [(A, B, scale * factor, d2, scale)])
            out[t + ".weight"] = (ref.reshape(w.shape), mag.reshape(w.shape))
        if diff_b is not None:
            b = sd[t + ".bias"]
            ref, mag = merge_ex_oracle(b.reshape(1, -1), [(None, None, 0.0, diff_b.reshape(1, -1), scale)])
            out[t + ".bias"] = (ref.reshape(-1), mag.reshape(-1))
    return out
