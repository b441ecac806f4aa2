"""fp8 self-attention: the shadow mode (enable_fp8_attention(): bf16 KV cache + e4m3 shadow) against the e4m3-only cache
(enable_fp8_attention(bf16_cache=False), include/rtv_hip_attn_fp8_only.h) on ONE 14B-shaped DiT, in one process.  Writes
profiles/r23_attn_fp8_only.json (or --out) with, for the 9360- and the 32760-row attention window,

  memory     per mode, with only that mode's KV cache alive: the bytes of the cache tensors, torch.cuda.max_memory_allocated over
             priming and one block, and the same above what was allocated before the cache existed (weights, workspaces, text caches).
             The memory is the claim of the mode.
  block_ms   five forwards back to back whose key window is the whole window = the DiT work of one block (no VAE, no text
             encoder), host clock around a device synchronise; median, min and max of --rounds rounds, modes alternating, plus the
             spread between the first and the second half of the rounds of ONE mode (what the box does to an unchanged program).
             The time is reported against the shadow mode of the same binary; no figure is promised.

Both modes compute the same bits (tests/test_attn_fp8_only_model_gpu.py); `outputs_equal` repeats that check at this shape."""
import argparse
import gc
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
MODES = ("shadow", "only")


def summary(xs):
    half = len(xs) // 2
    out = {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": xs}
    if half >= 2:
        a, b = statistics.median(xs[:half]), statistics.median(xs[half:])
        out["first_vs_second_half_pct"] = 100.0 * (b - a) / a
    return out


class Rig:
    """The shared model in one mode with a KV cache of `window` rows of its kind; every forward rewrites the last M rows and
    attends all `window` rows."""

    def __init__(self, model, wr, mode, window, inputs, ca):
        self.model, self.wr, self.mode, self.window = model, wr, mode, window
        self.lat, self.cond, self.t = inputs
        self.ca = ca
        L = model.num_layers
        self.enter()
        if mode == "only":
            self.kv = model.new_fp8_kv_cache(window, DEV)
        else:
            self.kv = [{"k": torch.zeros(1, window, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, window, HEADS, 128, dtype=BF, device=DEV),
                        "global_end_index": 0, "local_end_index": 0} for _ in range(L)]
        for c in self.kv:                                            # the rows in front of the block count as written (zeros)
            c["global_end_index"] = c["local_end_index"] = window - M
        self.forward()                                               # (shadow mode: allocates and fills the shadows)
        torch.cuda.synchronize()

    def enter(self):
        """Switch the shared model to this rig's mode.  The shadow mode refills its shadows from the whole bf16 cache in the first
        forward behind a switch: that forward runs here, outside every timing."""
        self.model.enable_fp8_attention(bf16_cache=self.mode != "only")
        if hasattr(self, "kv"):
            self.forward()

    def cache_bytes(self):
        return sum(t.numel() * t.element_size() for c in self.kv for t in c.values() if torch.is_tensor(t))

    def forward(self):
        return self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=self.window - M)[0]

    def block_ms(self):
        self.enter()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            self.forward()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--windows", default="9360,32760")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_attn_fp8_only.json"))
    args = ap.parse_args()
    windows = [int(w) for w in args.windows.split(",") if w]
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    ops.ensure_gemm_workspace(DEV)
    model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=args.layers, text_dim=4096, freq_dim=256,
                           device=DEV).init_random_weights(seed=0)
    wr = WanDiffusionWrapper(model, timestep_shift=5.0)
    g = torch.Generator().manual_seed(2)
    inputs = (torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV),
              {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]}, torch.tensor([[500.0, 500.0, 500.0]], device=DEV))
    ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
           "is_init": False} for _ in range(args.layers)]
    Rig(model, wr, "shadow", M, inputs, ca)                          # workspaces, text caches and maxima exist from here on
    res = {"device": torch.cuda.get_device_name(0), "layers": args.layers, "rounds": args.rounds,
           "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS}, "windows": {}}
    for window in windows:
        out = {"memory": {}, "block_ms": {}}
        for mode in MODES:                                           # memory: one mode's cache alive at a time
            gc.collect()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            rig = Rig(model, wr, mode, window, inputs, ca)
            rig.block_ms()
            peak = torch.cuda.max_memory_allocated()
            out["memory"][mode] = {"cache_bytes": rig.cache_bytes(), "max_memory_allocated": peak, "max_above_baseline": peak - base,
                                   "baseline_allocated": base}
            del rig
        gc.collect()
        rigs = {mode: Rig(model, wr, mode, window, inputs, ca) for mode in MODES}
        for r in rigs.values():
            r.block_ms()
        samples = {m: [] for m in rigs}
        for _ in range(args.rounds):
            for m, r in rigs.items():
                samples[m].append(r.block_ms())
        out["block_ms"] = {m: summary(v) for m, v in samples.items()}
        s, o = out["block_ms"]["shadow"]["median"], out["block_ms"]["only"]["median"]
        out["only_vs_shadow_block_pct"] = 100.0 * (o - s) / s
        out["only_vs_shadow_cache_bytes"] = out["memory"]["only"]["cache_bytes"] / out["memory"]["shadow"]["cache_bytes"]
        outs = []
        for r in rigs.values():
            r.enter()
            outs.append(r.forward().clone())
        out["outputs_equal"] = bool(torch.equal(*outs))
        res["windows"][str(window)] = out
        del rigs, outs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "shape"}, default=str)[:4000])


if __name__ == "__main__":
    main()
