"""Per-Linear precision policies (CausalWanModel.set_linear_precision, rtv_dit_config.use_fp8 == 7) beside bf16, fp8 per row and MXFP4
on a 14B-shaped DiT with synthetic weights, in one process and interleaved (scripts/mxfp6_bench.py with policies for modes; the
comparison points are the other configurations of the same run, never an earlier file).  Writes profiles/r21_mixed_precision.json
(or --out) with

  block_ms      five forwards back to back at a 9360-row window = the DiT work of one block (KV recompute + 4 denoising steps; no
                VAE, no text encoder) per configuration, host clock around a device synchronise: median, min and max of --rounds
                rounds, configurations alternating, the spread (max - min) / median and the drift between the two halves of the
                rounds of ONE configuration (what the box does to an unchanged program).
  depth_error   rel-L2 of one denoising forward against the bf16 forward of the same weights at --depths layers and at --layers.
  uniform_check the policy {"default": "mxfp4"} against enable_mxfp4(): the same launches, so the difference of their medians is
                reported beside the repeat spread of the two; `within_spread` says whether it is inside it.

Configurations: bf16, fp8_row, mxfp4 (the enable_* calls), mxfp4_policy (the uniform policy) and
  a  {"default": "fp8_row", "ffn0": "mxfp4", "ffn2": "mxfp4"}
  b  a with the six top-level Linears in bf16
  c  {"default": "mxfp4", "o": "fp8_row", "co": "fp8_row"}"""
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
M, D, FFN, HEADS = 4680, 5120, 13824, 40
POLICY_A = {"default": "fp8_row", "ffn0": "mxfp4", "ffn2": "mxfp4"}
POLICIES = {"a": POLICY_A,
            "b": dict(POLICY_A, **{k: "bf16" for k in ("text0", "text2", "time0", "time2", "tproj", "head")}),
            "c": {"default": "mxfp4", "o": "fp8_row", "co": "fp8_row"},
            "mxfp4_policy": {"default": "mxfp4"}}
CONFIGS = ("bf16", "fp8_row", "mxfp4", "mxfp4_policy", "a", "b", "c")


def summary(xs):
    half = len(xs) // 2
    med = statistics.median(xs)
    out = {"median": med, "min": min(xs), "max": max(xs), "spread_pct": 100.0 * (max(xs) - min(xs)) / med, "samples": xs}
    if half >= 2:
        a, b = statistics.median(xs[:half]), statistics.median(xs[half:])
        out["first_vs_second_half_pct"] = 100.0 * (b - a) / a
    return out


def configure(model, config):
    if config == "fp8_row":
        model.enable_fp8("row")
    elif config == "mxfp4":
        model.enable_mxfp4()
    elif config in POLICIES:
        model.set_linear_precision(POLICIES[config])
        assert model._cfg.use_fp8 == 7
    return model


class Rig:
    """A 14B-shaped model in one configuration with its caches, primed to a 9360-row attention window."""

    def __init__(self, config, layers):
        self.model = configure(CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                                              device=DEV).init_random_weights(seed=0), config)
        self.wr = WanDiffusionWrapper(self.model, timestep_shift=5.0)
        g = torch.Generator().manual_seed(2)
        self.lat = torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV)
        self.cond = {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]}
        self.t = torch.tensor([[500.0, 500.0, 500.0]], device=DEV)
        self.kv = [{"k": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV),
                    "global_end_index": 0, "local_end_index": 0} for _ in range(layers)]
        self.ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
                    "is_init": False} for _ in range(layers)]
        self.first = self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=0)[0].float()
        self.forward()
        torch.cuda.synchronize()

    def forward(self):
        return self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=M)[0]

    def block_ms(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            self.forward()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def interleaved(fns, rounds):
    for f in fns.values():
        f()
    samples = {m: [] for m in fns}
    for _ in range(rounds):
        for m, f in fns.items():
            samples[m].append(f())
    return {m: summary(v) for m, v in samples.items()}


def depth_error(rigs):
    """rel-L2 of the first denoising forward (cache offset 0: no history of the configuration's own K / V) against the bf16 rig's."""
    ref = rigs["bf16"].first
    return {m: float((r.first - ref).norm() / ref.norm()) for m, r in rigs.items() if m != "bf16"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--depths", default="1,8")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_mixed_precision.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    ops.ensure_gemm_workspace(DEV)
    res = {"device": torch.cuda.get_device_name(0), "weights": "synthetic (init_random_weights)", "configs": list(CONFIGS),
           "policies": POLICIES, "layers": args.layers, "rounds": args.rounds,
           "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS}, "depth_error_vs_bf16": {}}

    for depth in [int(d) for d in args.depths.split(",") if d]:
        rigs = {c: Rig(c, depth) for c in CONFIGS}
        res["depth_error_vs_bf16"][str(depth)] = depth_error(rigs)
        print(f"depth {depth}: {res['depth_error_vs_bf16'][str(depth)]}", file=sys.stderr, flush=True)
        del rigs
        torch.cuda.empty_cache()

    rigs = {c: Rig(c, args.layers) for c in CONFIGS}
    res["depth_error_vs_bf16"][str(args.layers)] = depth_error(rigs)
    res["uniform_policy_output_equals_enable_mxfp4"] = bool(torch.equal(rigs["mxfp4_policy"].first, rigs["mxfp4"].first))
    res["block_ms"] = interleaved({c: r.block_ms for c, r in rigs.items()}, args.rounds)
    blk = res["block_ms"]
    for c in CONFIGS[1:]:
        res[f"{c}_vs_bf16_block_pct"] = 100.0 * (blk[c]["median"] / blk["bf16"]["median"] - 1)
    diff = 100.0 * (blk["mxfp4_policy"]["median"] / blk["mxfp4"]["median"] - 1)
    spread = max(blk["mxfp4_policy"]["spread_pct"], blk["mxfp4"]["spread_pct"])
    res["uniform_check"] = {"mxfp4_policy_vs_enable_mxfp4_pct": diff, "repeat_spread_pct": spread, "within_spread": abs(diff) <= spread}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    brief = {"block_ms": {c: round(v["median"], 2) for c, v in blk.items()},
             "spread_pct": {c: round(v["spread_pct"], 2) for c, v in blk.items()}, "uniform_check": res["uniform_check"],
             "uniform_policy_output_equals_enable_mxfp4": res["uniform_policy_output_equals_enable_mxfp4"],
             "depth_error_vs_bf16": res["depth_error_vs_bf16"]}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
