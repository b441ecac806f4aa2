"""MXFP6 Linears (enable_mxfp6(), include/rtv_hip_mxfp6.h) beside bf16, the two fp8 modes and MXFP4 on a 14B-shaped DiT, in one
process and interleaved (scripts/mxfp4_bench.py with a fifth mode; the comparison points are the other modes of the same run, never
an earlier file).  Writes profiles/r17_mxfp6.json (or --out) with

  gemm_us       per-shape device-event time of the projection GEMM alone (operands quantised beforehand) for the four layer
                shapes at M = 4680 and at the 585-row shard: bf16 (rtv_gemm), fp8 per tensor, fp8 per row, MXFP4, MXFP6; median, min and
                max of --rounds rounds, modes alternating, and the spread between the two halves of the rounds of ONE mode (what the
                box does to an unchanged program).
  block_ms      five forwards back to back at a 9360-row window = the DiT work of one block (KV recompute + 4 denoising steps; no
                VAE, no text encoder) in the same five modes, host clock around a device synchronise, same statistics.
  depth_error   rel-L2 of one denoising forward against the bf16 forward of the same weights at --depths layers (14B width), for
                the two fp8 modes, MXFP4 and MXFP6: what the quantisation costs, beside what it buys."""
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
MODES = ("bf16", "fp8_tensor", "fp8_row", "mxfp4", "mxfp6")
SHAPES = {"qkv": (3 * D, D), "o": (D, D), "ffn_in": (FFN, D), "ffn_out": (D, FFN)}      # name -> (N, K)


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


def gemm_fns(m, n, k):
    """{mode: callable running the GEMM of x [m, k] and w [n, k] into a preallocated output}."""
    g = torch.Generator(device=DEV).manual_seed(m + n + k)
    x = torch.randn(m, k, device=DEV, generator=g).to(BF)
    w = (torch.randn(n, k, device=DEV, generator=g) * k ** -0.5).to(BF)
    out = torch.empty(m, n, dtype=BF, device=DEV)
    xt, st = ops.quantize_fp8(x)
    wt, swt = CausalWanModel._quantize_fp8(w)
    xr, sr = ops.quantize_fp8_rows(x)
    wr, swr = CausalWanModel._quantize_fp8_rows(w)
    xc, xs = ops.quantize_mxfp4(x)
    wc, ws = ops.quantize_mxfp4(w)
    xc6, xs6 = ops.quantize_mxfp6(x)
    wc6, ws6 = ops.quantize_mxfp6(w)
    return {"bf16": lambda: ops.gemm(x, w, out=out),
            "fp8_tensor": lambda: ops.gemm_fp8(xt, st, wt, swt, out=out),
            "fp8_row": lambda: ops.gemm_fp8_rows(xr, sr, wr, swr, out=out),
            "mxfp4": lambda: ops.gemm_mxfp4(xc, xs, wc, ws, out=out),
            "mxfp6": lambda: ops.gemm_mxfp6(xc6, xs6, wc6, ws6, out=out)}


def enable(model, mode):
    if mode == "fp8_tensor":
        model.enable_fp8()
    elif mode == "fp8_row":
        model.enable_fp8("row")
    elif mode == "mxfp4":
        model.enable_mxfp4()
    elif mode == "mxfp6":
        model.enable_mxfp6()
    return model


class Rig:
    """A 14B-shaped model in one mode with its caches, primed to a 9360-row attention window."""

    def __init__(self, mode, layers):
        self.model = enable(CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                                           device=DEV).init_random_weights(seed=0), mode)
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


def interleaved(fns, rounds, sample):
    for f in fns.values():
        sample(f)
    samples = {m: [] for m in fns}
    for _ in range(rounds):
        for m, f in fns.items():
            samples[m].append(sample(f))
    return {m: summary(v) for m, v in samples.items()}


def depth_error(rigs):
    """rel-L2 of the first denoising forward (cache offset 0: no history of the mode's own K / V) against the bf16 rig's."""
    ref = rigs["bf16"].first
    return {m: float((r.first - ref).norm() / ref.norm()) for m, r in rigs.items() if m != "bf16"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--depths", default="1,8")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_mxfp6.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    ops.ensure_gemm_workspace(DEV)
    res = {"device": torch.cuda.get_device_name(0), "modes": list(MODES), "layers": args.layers, "rounds": args.rounds,
           "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS}, "gemm_us": {}, "depth_error_vs_bf16": {}}

    for m in (M, M // 8):
        for name, (n, k) in SHAPES.items():
            r = interleaved(gemm_fns(m, n, k), args.rounds, lambda f: 1e3 * event_ms(f, 10))
            for mode in MODES:
                r[mode]["tflops"] = 2.0 * m * n * k / r[mode]["median"] * 1e-6
            res["gemm_us"][f"{name}_M{m}"] = r
            print(f"gemm {name} M={m}: " + " ".join(f"{mode} {r[mode]['median']:.1f}" for mode in MODES), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()

    for depth in [int(d) for d in args.depths.split(",") if d]:
        rigs = {mode: Rig(mode, depth) for mode in MODES}
        res["depth_error_vs_bf16"][str(depth)] = depth_error(rigs)
        print(f"depth {depth}: {res['depth_error_vs_bf16'][str(depth)]}", file=sys.stderr, flush=True)
        del rigs
        torch.cuda.empty_cache()

    rigs = {mode: Rig(mode, args.layers) for mode in MODES}
    res["depth_error_vs_bf16"][str(args.layers)] = depth_error(rigs)
    res["block_ms"] = interleaved({m: r.block_ms for m, r in rigs.items()}, args.rounds, lambda f: f())
    for mode in MODES[1:]:
        res[f"{mode}_vs_bf16_block_pct"] = 100.0 * (res["block_ms"][mode]["median"] / res["block_ms"]["bf16"]["median"] - 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    brief = {"gemm_us": {s: {m: round(v[m]["median"], 1) for m in MODES} for s, v in res["gemm_us"].items()},
             "block_ms": {m: round(v["median"], 2) for m, v in res["block_ms"].items()}, "depth_error_vs_bf16": res["depth_error_vs_bf16"]}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
