"""K smoothing of the fp8 attention shadow (enable_fp8_attention(smooth_k=True); include/rtv_hip_attn_fp8_center.h) beside the plain
fp8 attention mode on a 14B-shaped DiT, in one process and interleaved.  Writes profiles/r20_attn_fp8_center.json (or --out;
sections already in that file are kept, so --only can run the parts in several visits) with

  quantiser_us  device-event time of rtv_attn_quantize_kv and rtv_attn_quantize_kv_centered alone, 40 heads, on the 4680 rows one
                forward writes and on a whole-cache refill of 9360 and of 32760 rows; median, min and max of --rounds rounds, the two
                alternating, and the spread between the two halves of the rounds of ONE variant (what the box does to an unchanged
                program).  The centred quantiser moves 512 bytes more per workgroup: anything beyond that spread is ALU.
  recentre_ms   one recentre of a 40-layer model at both cache sizes: per layer the column means (rtv_attn_kv_center) and the
                centred refill of the whole shadow, 40 times, device events.
  block_ms      five forwards back to back at a 9360-row window = the DiT work of one block (KV recompute + 4 denoising steps; no
                VAE, no text encoder) with fp8 attention, smooth_k off and on (recentred once), host clock around a device
                synchronise, same statistics.
  depth_error   rel-L2 of the second denoising forward (9360-row window, behind the recentre) against the bf16 forward of the same
                weights at --depths layers (14B width), plain against smoothed, once on the usual random weights ("random") and
                once with every 8th entry of each layer's norm_k.weight times 16 ("norm_k_x16").  No real checkpoint is involved."""
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
MODES = ("fp8_attn", "fp8_attn_smooth_k")


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


def interleaved(fns, rounds, sample):
    for f in fns.values():
        sample(f)
    samples = {m: [] for m in fns}
    for _ in range(rounds):
        for m, f in fns.items():
            samples[m].append(sample(f))
    return {m: summary(v) for m, v in samples.items()}


class Cache:
    """One layer's bf16 cache of `cache_rows` rows with its shadow, a centre and the mean workspace."""

    def __init__(self, cache_rows):
        g = torch.Generator(device=DEV).manual_seed(cache_rows)
        self.rows = cache_rows
        self.k, self.v = (torch.randn(cache_rows, HEADS, 128, device=DEV, generator=g).to(BF) for _ in range(2))
        self.k8, self.v8t = ops.attn_fp8_shadow(cache_rows, HEADS, DEV)
        self.amax = torch.zeros(2, device=DEV)
        self.ws = torch.empty(ops.attn_kv_center_workspace_bytes(cache_rows, HEADS) // 4, dtype=torch.float32, device=DEV)
        self.center = ops.attn_kv_center(self.k, (0, cache_rows), workspace=self.ws)

    def quantise(self, rows, center):
        ops.attn_quantize_kv(self.k, self.v, self.k8, self.v8t, self.rows - rows, rows, amax=self.amax, center=center)

    def recentre(self, layers):
        for _ in range(layers):
            ops.attn_kv_center(self.k, (0, self.rows), out=self.center, workspace=self.ws)
            self.quantise(self.rows, self.center)


def scale_norm_k(model):
    """every 8th entry of each layer's norm_k.weight times 16, in place"""
    for l in range(model.num_layers):
        model._tensors[f"L{l}.norm_k_w"][::8] *= 16
    return model


class Rig:
    """A 14B-shaped model with caches of its own per mode: `first` is the denoising forward at cache offset 0, `second` the one at
    offset M over the 9360-row window - behind the recentre when the mode smooths."""

    def __init__(self, model, mode):
        self.model, layers = model, model.num_layers
        model.disable_fp8_attention()
        if mode != "bf16":
            model.enable_fp8_attention(smooth_k=mode.endswith("smooth_k"))
        self.mode = mode
        self.wr = WanDiffusionWrapper(model, timestep_shift=5.0)
        g = torch.Generator().manual_seed(2)
        self.lat = torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV)
        self.cond = {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]}
        self.t = torch.tensor([[500.0, 500.0, 500.0]], device=DEV)
        self.kv = [{"k": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV),
                    "global_end_index": 0, "local_end_index": 0} for _ in range(layers)]
        self.ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
                    "is_init": False} for _ in range(layers)]
        self.first = self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=0)[0].float()
        if mode.endswith("smooth_k"):
            model.fp8_attention_recenter(self.kv)
        self.second = self.forward().float()
        torch.cuda.synchronize()

    def select(self):
        """Put the shared model into this rig's mode (the epoch bumps: the next forward refills this rig's shadows once)."""
        self.model.disable_fp8_attention()
        if self.mode != "bf16":
            self.model.enable_fp8_attention(smooth_k=self.mode.endswith("smooth_k"))
        self.forward()

    def forward(self):
        return self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=M)[0]

    def block_ms(self):
        self.select()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            self.forward()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def build(layers, scaled):
    model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                           device=DEV).init_random_weights(seed=0)
    return scale_norm_k(model) if scaled else model


def depth_error(model):
    ref = Rig(model, "bf16").second
    out = {}
    for mode in MODES:
        out[mode] = float((Rig(model, mode).second - ref).norm() / ref.norm())
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--depths", default="1,8,40")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--only", default="quantiser,recentre,depth,block", help="comma-separated sections to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_attn_fp8_center.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    ops.ensure_gemm_workspace(DEV)
    only = set(args.only.split(","))
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res.update({"device": torch.cuda.get_device_name(0), "modes": list(MODES),
                "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS}})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    if only & {"quantiser", "recentre"}:
        res["quantiser_rounds"] = args.rounds
        for cache_rows in (9360, 32760):
            c = Cache(cache_rows)
            if "quantiser" in only:
                for rows in ((M, 9360) if cache_rows == 9360 else (32760,)):
                    fns = {"plain": lambda r=rows: c.quantise(r, None), "centred": lambda r=rows: c.quantise(r, c.center)}
                    r = interleaved(fns, args.rounds, lambda f: 1e3 * event_ms(f, 20))
                    r["centred_vs_plain_pct"] = 100.0 * (r["centred"]["median"] / r["plain"]["median"] - 1)
                    res.setdefault("quantiser_us", {})[f"rows{rows}"] = r
            if "recentre" in only:
                c.recentre(args.layers)
                res.setdefault("recentre_ms", {})[f"rows{cache_rows}"] = dict(
                    summary([event_ms(lambda: c.recentre(args.layers), 1) for _ in range(args.rounds)]), layers=args.layers)
            del c
            torch.cuda.empty_cache()
            save()
    depths = [int(d) for d in args.depths.split(",") if d] if "depth" in only else []
    if "block" in only and args.layers not in depths:
        depths.append(args.layers)
    for depth in depths:
        for kind in ("random", "norm_k_x16"):
            if "depth" not in only and kind != "random":
                continue
            model = build(depth, kind != "random")
            if "depth" in only:
                res.setdefault("depth_error_vs_bf16", {"random": {}, "norm_k_x16": {}})[kind][str(depth)] = depth_error(model)
                save()
            if "block" in only and depth == args.layers and kind == "random":
                rigs = {mode: Rig(model, mode) for mode in MODES}
                res["layers"], res["block_rounds"] = args.layers, args.rounds
                res["block_ms"] = interleaved({m: r.block_ms for m, r in rigs.items()}, args.rounds, lambda f: f())
                res["smooth_k_vs_plain_block_pct"] = 100.0 * (res["block_ms"][MODES[1]]["median"] / res["block_ms"][MODES[0]]["median"] - 1)
                save()
                del rigs
            del model
            torch.cuda.empty_cache()
    brief = {"quantiser_us": {d: {m: round(v["median"], 1) for m, v in r.items() if isinstance(v, dict)} | {"pct": round(r["centred_vs_plain_pct"], 2)}
                              for d, r in res.get("quantiser_us", {}).items()},
             "recentre_ms": {d: round(v["median"], 2) for d, v in res.get("recentre_ms", {}).items()},
             "block_ms": {m: round(v["median"], 2) for m, v in res.get("block_ms", {}).items()},
             "depth_error_vs_bf16": res.get("depth_error_vs_bf16", {})}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
