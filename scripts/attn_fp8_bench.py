"""fp8 self-attention (enable_fp8_attention, include/rtv_hip_attn_fp8.h) against the bf16 attention it is an option to, in one
process with the modes alternating.  Writes profiles/r15_attn_fp8.json (or --out) with

  attention_ms    (a) the attention kernel alone at 40 heads: rtv_attn_fwd_fp8 on a ready shadow against the default bf16 dispatch of
                  rtv_attn_fwd_win, 4680 query rows x {9360, 14040, 32760} keys, plus the block-causal 4680 x 4680 launch of the
                  KV-recompute pass (blocks of 1560 tokens).  Device-event time per launch, median / min / max of --rounds rounds and
                  the spread between the first and the second half of the rounds of one mode; TF/s counts 4 Lq Lkv 128 H flop.
  quantiser       (b) rtv_attn_quantize_kv on 4680 rows x 40 heads (reads 95.8 MB of bf16 K and V, writes 47.9 MB of codes) against
                  copy_ of the same 95.8 MB; both as bytes moved per second, and their ratio (the target is 1).
  block_ms        (c) five 40-layer forwards at a 9360-row window = the DiT work of one block, fp8 attention on and off, with bf16
                  Linears and with enable_fp8(); host clock around a device synchronise.

The bf16 numbers are the parent commit's: with the mode off every launch is the one the parent issues (the off path is unchanged),
measured here in the same run."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realtime_video_amd import ops                                   # noqa: E402
from realtime_video_amd.causal_model import CausalWanModel           # noqa: E402
from realtime_video_amd.wan_wrapper import WanDiffusionWrapper       # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
M, D, FFN, HEADS, FS = 4680, 5120, 13824, 40, 1560


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(xs):
    half = len(xs) // 2
    out = {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": xs}
    if half >= 2:
        a, b = statistics.median(xs[:half]), statistics.median(xs[half:])
        out["first_vs_second_half_pct"] = 100.0 * (b - a) / a
    return out


def alternate(fns, rounds, iters):
    for f in fns.values():
        event_ms(f, 2)
    samples = {m: [] for m in fns}
    for _ in range(rounds):
        for m, f in fns.items():
            samples[m].append(event_ms(f, iters))
    return {m: summary(v) for m, v in samples.items()}


def attention_section(rounds):
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.randn(1, M, HEADS, 128, device=DEV, generator=g).to(BF)
    out = {}
    for name, lkv, cb in (("4680x9360", 9360, 0), ("4680x14040", 14040, 0), ("4680x32760", 32760, 0), ("4680x4680_block_causal_1560", 4680, FS)):
        k, v = (torch.randn(1, lkv, HEADS, 128, device=DEV, generator=g).to(BF) for _ in range(2))
        k8, v8t = ops.attn_fp8_shadow(lkv, HEADS, DEV)
        ops.attn_quantize_kv(k[0], v[0], k8, v8t)
        o16, o8 = torch.empty_like(q), torch.empty_like(q[0])
        q_off = lkv - M
        if cb:
            bf16 = lambda: ops.attn_fwd(q, k, v, out=o16, causal_block=cb, q_offset=q_off)                       # noqa: E731
        else:
            bf16 = lambda: ops.attn_fwd_win(q, k, v, (0, lkv), out=o16)                                        # noqa: E731
        fp8 = lambda: ops.attn_fwd_fp8(q[0], k8, v8t, (0, lkv), out=o8, causal_block=cb, q_offset=q_off)         # noqa: E731
        res = alternate({"bf16": bf16, "fp8": fp8}, rounds, 10)
        flop = 4.0 * M * lkv * 128 * HEADS * (0.5 * (1 + FS / lkv) if cb else 1.0)      # block-causal: the visible share of the keys
        for m in res:
            res[m]["tflops_at_median"] = flop / (res[m]["median"] * 1e-3) / 1e12
        res["fp8_vs_bf16_pct"] = 100.0 * (res["fp8"]["median"] - res["bf16"]["median"]) / res["bf16"]["median"]
        res["output_rel_l2_fp8_vs_bf16"] = float((o8.float() - o16[0].float()).norm() / o16[0].float().norm())
        out[name] = res
        del k, v, k8, v8t
    return out


def quantiser_section(rounds):
    g = torch.Generator(device=DEV).manual_seed(1)
    k, v = (torch.randn(M, HEADS, 128, device=DEV, generator=g).to(BF) for _ in range(2))
    k8, v8t = ops.attn_fp8_shadow(M, HEADS, DEV)
    amax = torch.zeros(2, device=DEV)
    src = torch.cat([k.flatten(), v.flatten()])
    dst = torch.empty_like(src)
    res = alternate({"quantize_kv": lambda: ops.attn_quantize_kv(k, v, k8, v8t), "quantize_kv_amax": lambda: ops.attn_quantize_kv(k, v, k8, v8t, amax=amax),
                     "copy": lambda: dst.copy_(src)}, rounds, 20)
    in_bytes = src.numel() * 2
    moved = {"quantize_kv": in_bytes + k8.numel() + v8t.numel(), "quantize_kv_amax": in_bytes + k8.numel() + v8t.numel(), "copy": 2 * in_bytes}
    for m in res:
        res[m]["bytes_moved"] = moved[m]
        res[m]["gb_per_s_at_median"] = moved[m] / (res[m]["median"] * 1e-3) / 1e9
    res["quantiser_rate_over_copy_rate"] = res["quantize_kv"]["gb_per_s_at_median"] / res["copy"]["gb_per_s_at_median"]
    res["quantiser_time_over_copy_time"] = res["quantize_kv"]["median"] / res["copy"]["median"]
    return res


class Rig:
    """A 14B-shaped model (bf16 or fp8 Linears) with its caches, primed to a 9360-row attention window; fp8 attention toggles."""

    def __init__(self, fp8_linears, layers):
        self.model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                                    device=DEV).init_random_weights(seed=0)
        if fp8_linears:
            self.model.enable_fp8()
        self.wr = WanDiffusionWrapper(self.model, timestep_shift=5.0)
        g = torch.Generator().manual_seed(2)
        self.lat = torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV)
        self.cond = {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]}
        self.t = torch.tensor([[500.0, 500.0, 500.0]], device=DEV)
        self.kv = [{"k": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV),
                    "global_end_index": 0, "local_end_index": 0} for _ in range(layers)]
        self.ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
                    "is_init": False} for _ in range(layers)]
        self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=0)
        self.forward()
        torch.cuda.synchronize()

    def forward(self):
        return self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=M)[0]

    def block_ms(self, fp8_attention):
        if fp8_attention:
            self.model.enable_fp8_attention()
        else:
            self.model.disable_fp8_attention()
        self.forward()                       # untimed: the forward after a switch refills the shadows from the bf16 caches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            self.forward()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def block_section(rounds, layers):
    out = {}
    for lin in ("bf16_linears", "fp8_linears"):
        rig = Rig(lin == "fp8_linears", layers)
        for a in (False, True):
            rig.block_ms(a)
        samples = {"bf16_attention": [], "fp8_attention": []}
        for _ in range(rounds):
            for m in samples:
                samples[m].append(rig.block_ms(m == "fp8_attention"))
        res = {m: summary(v) for m, v in samples.items()}
        res["fp8_vs_bf16_attention_pct"] = 100.0 * (res["fp8_attention"]["median"] - res["bf16_attention"]["median"]) / res["bf16_attention"]["median"]
        rig.model.disable_fp8_attention()
        a = rig.forward().float()
        rig.model.enable_fp8_attention()
        b = rig.forward().float()
        res["output_rel_l2_fp8_vs_bf16_attention"] = float((a - b).norm() / a.norm())
        res["amax_k_v_over_layers"] = [float(x) for x in rig.model.fp8_attention_amax().max(0).values]
        out[lin] = res
        del rig
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="attention,quantiser,block")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_attn_fp8.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    assert args.rounds >= 5, "at least five rounds"
    ops.ensure_gemm_workspace(DEV)
    res = {"device": torch.cuda.get_device_name(0), "layers": args.layers, "rounds": args.rounds,
           "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS},
           "baseline": "the bf16 entries are the parent commit's numbers: with the mode off every launch is the one the parent issues, "
                       "measured in this run, in this process, alternating with the fp8 mode"}
    sections = args.sections.split(",")
    if "attention" in sections:
        res["attention_ms"] = attention_section(args.rounds)
    if "quantiser" in sections:
        res["quantiser"] = quantiser_section(args.rounds)
    if "block" in sections:
        res["block_ms"] = block_section(args.rounds, args.layers)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)

    def brief(o):
        return {k: brief(v) for k, v in o.items() if k != "samples"} if isinstance(o, dict) else o
    print(json.dumps(brief(res), default=str))


if __name__ == "__main__":
    main()
