"""The block Hadamard rotation of the MXFP4 / MXFP6 quantisers (enable_mxfp4(rotate=True) / enable_mxfp6(rotate=True);
include/rtv_hip_mx_rotate.h) beside the unrotated modes on a 14B-shaped DiT, in one process and interleaved.  Writes
profiles/r18_mx_rotate.json (or --out; sections already in that file are kept, so --only can run the parts in several visits) with

  quantiser_us  device-event time of the row quantiser and of the LayerNorm-fused quantiser alone at M = 4680, d = 5120 (both) and
                d = 13824 (the row quantiser: the fused one ends at 8192), rotated against unrotated, both formats; median, min and
                max of --rounds rounds, variants alternating, and the spread between the two halves of the rounds of ONE variant
                (what the box does to an unchanged program).  The rotation moves no byte more: anything beyond that spread is ALU.
  block_ms      five forwards back to back at a 9360-row window = the DiT work of one block (KV recompute + 4 denoising steps; no
                VAE, no text encoder) in modes 3, 5, 4 and 6, host clock around a device synchronise, same statistics.
  depth_error   rel-L2 of one denoising forward against the bf16 forward of the same weights at --depths layers (14B width) for the
                four modes, once on the usual random weights ("random") and once with outlier channels injected ("outliers": every
                32nd entry of each layer's modulation scale rows and of norm3.weight times 32, so the LayerNorm outputs in front of
                qkv / ffn.0 / cross-q carry them).  No real checkpoint is involved."""
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
MODES = ("mxfp4", "mxfp4_rot", "mxfp6", "mxfp6_rot")                  # rtv_dit_config.use_fp8 3, 5, 4, 6


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


def quantiser_fns(d):
    """{variant: callable} of the row quantisers on x [M, d] into preallocated outputs, and of the fused ones where d allows."""
    g = torch.Generator(device=DEV).manual_seed(d)
    x = torch.randn(M, d, device=DEV, generator=g).to(BF)
    emod = (torch.randn(3, 6, d, device=DEV, generator=g) * 0.5).to(BF)
    fns = {}
    for name in ("mxfp4", "mxfp6"):
        quantize = getattr(ops, "quantize_" + name)
        codes, scales = quantize(x)
        for rot, kw in (("", {}), ("_rot", dict(rotate_shift=ops.MX_ROT_ACT_SHIFT))):
            fns[f"quantize_{name}{rot}"] = lambda q=quantize, kw=kw, c=codes, s=scales: q(x, codes=c, scales=s, **kw)
            if d <= 8192:
                ln = getattr(ops, f"layernorm_modulate_{name}{rot}")
                fns[f"layernorm_modulate_{name}{rot}"] = lambda ln=ln: ln(x, 1e-6, shift=emod[0, 0], scale=emod[0, 1], frame_stride=6 * d,
                                                                          rows_per_frame=M // 3)
    return fns


def inject_outliers(model):
    """every 32nd entry of each layer's modulation scale rows (1: attention, 4: ffn) and of norm3.weight times 32, in place"""
    for row in (1, 4):
        model._tensors["modulation"][:, row, ::32] *= 32
    for l in range(model.num_layers):
        model._tensors[f"L{l}.norm3_w"][::32] *= 32
    return model


def enable(model, mode):
    if mode != "bf16":
        getattr(model, "enable_" + mode.split("_")[0])(rotate=mode.endswith("_rot"))
    return model


class Rig:
    """A 14B-shaped model in one mode with its caches, primed to a 9360-row attention window."""

    def __init__(self, mode, layers, outliers=False, prime=True):
        model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                               device=DEV).init_random_weights(seed=0)
        self.model = enable(inject_outliers(model) if outliers else model, mode)
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
        if prime:
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


def depth_error(layers, outliers):
    """rel-L2 of the first denoising forward (cache offset 0: no history of the mode's own K / V) against the bf16 model's; one
    model at a time, so that 40 layers of five modes never sit in memory together"""
    ref = Rig("bf16", layers, outliers, prime=False).first
    out = {}
    for mode in MODES:
        out[mode] = float((Rig(mode, layers, outliers, prime=False).first - ref).norm() / ref.norm())
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--depths", default="1,8,40")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--only", default="quantiser,depth,block", help="comma-separated sections to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_mx_rotate.json"))
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

    if "quantiser" in only:
        res["quantiser_rounds"] = args.rounds
        res["quantiser_us"] = {}
        for d in (D, FFN):
            r = interleaved(quantiser_fns(d), args.rounds, lambda f: 1e3 * event_ms(f, 20))
            for name, v in r.items():
                base = r[name.replace("_rot", "")]["median"]
                v["vs_unrotated_pct"] = 100.0 * (v["median"] / base - 1)
            res["quantiser_us"][f"d{d}"] = r
            torch.cuda.empty_cache()
        save()
    if "depth" in only:
        res.setdefault("depth_error_vs_bf16", {"random": {}, "outliers": {}})
        for depth in [int(d) for d in args.depths.split(",") if d]:
            for kind in ("random", "outliers"):
                res["depth_error_vs_bf16"][kind][str(depth)] = depth_error(depth, kind == "outliers")
                save()
    if "block" in only:
        rigs = {mode: Rig(mode, args.layers) for mode in MODES}
        res["layers"], res["block_rounds"] = args.layers, args.rounds
        res["block_ms"] = interleaved({m: r.block_ms for m, r in rigs.items()}, args.rounds, lambda f: f())
        for name in ("mxfp4", "mxfp6"):
            res[f"{name}_rot_vs_{name}_block_pct"] = 100.0 * (res["block_ms"][name + "_rot"]["median"] / res["block_ms"][name]["median"] - 1)
        save()
    brief = {"quantiser_us": {d: {m: round(v["median"], 1) for m, v in r.items()} for d, r in res.get("quantiser_us", {}).items()},
             "block_ms": {m: round(v["median"], 2) for m, v in res.get("block_ms", {}).items()},
             "depth_error_vs_bf16": res.get("depth_error_vs_bf16", {})}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
