"""The e4m3-only KV cache under the row exchange of context parallelism with the exchange carrying codes
(enable_fp8_attention(bf16_cache=False, context_parallel="codes"), include/rtv_hip_attn_fp8_only_cp.h) beside the shadow mode under
the same exchange (context_parallel=True, include/rtv_hip_attn_fp8_cp.h), which is the yardstick: one process, ONE GPU, eight ranks
in lockstep (SimulatedContextParallel(8, "rows"): eight times a rank's work, no communication), the 14B shape, windows of 9 360 and
32 760 rows, the two modes alternating.  Writes profiles/r27_attn_fp8_only_cp.json (or --out) with

  memory          per window and mode: bytes of the KV cache dicts, and the peak allocation of two forwards above what was allocated
                  before the cache (weights, workspaces and the text caches are in that baseline after the warm-up).
  block_ms        per window: five 40-layer forwards back to back = the DiT work of one block, host clock around a device
                  synchronise, median / min / max of --rounds rounds and per mode the spread between the two halves of its rounds
                  (what the box does to an unchanged program).
  kernel_us       the stage kernels of one rank's 585 rows and the commit of the 4680 gathered rows alone, device events, beside a
                  copy_ that moves the same bytes and beside what the shadow mode runs in their place (rtv_attn_quantize_kv on the
                  4680 gathered bf16 rows).
  exchange_bytes  received per rank and layer by the all-gather, computed from the shapes - nothing here ran on more than one GPU.

No speed-up is claimed, no real checkpoint is involved.  Without a GPU the script fails."""
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
from realtime_video_amd import ops                                                      # noqa: E402
from realtime_video_amd.causal_model import CausalWanModel                              # noqa: E402
from realtime_video_amd.parallel import SimulatedContextParallel, attn_kv_splits_for    # noqa: E402
from realtime_video_amd.rope import rope_cos_sin_table                                  # noqa: E402
from realtime_video_amd.wan_wrapper import WanDiffusionWrapper                          # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
M, D, FFN, HEADS, WORLD = 4680, 5120, 13824, 40, 8
GRID = (3, 30, 52)
WINDOWS = (9360, 32760)
MODES = ("shadow_cp", "compact_cp")


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
    for i in range(rounds):
        for m, f in fns.items():
            samples[m].append(sample(f))
        print(f"round {i + 1}/{rounds}: " + " ".join(f"{m}={v[-1]:.1f}" for m, v in samples.items()), file=sys.stderr, flush=True)
    return {m: summary(v) for m, v in samples.items()}


def kernel_section(rounds, iters):
    S = M // WORLD
    g = torch.Generator(device=DEV).manual_seed(1)
    qkv = torch.randn(S, 3 * D, device=DEV, generator=g).to(BF)
    wk = torch.ones(D, dtype=BF, device=DEV)
    cs = rope_cos_sin_table(128).to(DEV)
    kv8 = ops.attn_fp8_staging(M, HEADS, WORLD, DEV)
    kv8.random_(0, 120)                                              # (codes below 0x78: no NaN code; the movers do not look at them)
    k8, v8t = ops.attn_fp8_shadow(M, HEADS, DEV)
    kc, vc = (torch.randn(M, HEADS, 128, device=DEV, generator=g).to(BF) for _ in range(2))
    amax = torch.zeros(2, dtype=torch.float32, device=DEV)
    # copies that move the same bytes: stage reads 2 S d bf16 and writes 2 S d codes (6 S d bytes = a copy_ of 3 S d bytes);
    # commit reads and writes 2 M d bytes (a copy_ of 2 M d bytes)
    a_stage, b_stage = (torch.empty(3 * S * D, dtype=torch.uint8, device=DEV) for _ in range(2))
    a_commit, b_commit = (torch.empty(2 * M * D, dtype=torch.uint8, device=DEV) for _ in range(2))
    fns = {
        "stage_one_rank": lambda: ops.attn_fp8_stage_kv8(qkv, kv8, 0, HEADS, wk, cs, GRID, 0, amax=amax),
        "copy_stage_bytes": lambda: b_stage.copy_(a_stage),
        "commit_block": lambda: ops.attn_fp8_commit_kv8(kv8, k8, v8t, 0),
        "copy_commit_bytes": lambda: b_commit.copy_(a_commit),
        "shadow_quantize_block": lambda: ops.attn_quantize_kv(kc, vc, k8, v8t, 0, M, amax=amax),
    }
    r = interleaved(fns, rounds, lambda f: 1e3 * event_ms(f, iters))
    r["bytes"] = {"stage_one_rank": 6 * S * D, "commit_block": 4 * M * D, "shadow_quantize_block": 6 * M * D}
    return r


def new_caches(model, mode, layers, window):
    if mode == "compact_cp":
        kv = model.new_fp8_kv_cache(window, DEV)
        for c in kv:
            c["k8"].random_(0, 120)
            c["v8t"].random_(0, 120)
        return kv
    gd = torch.Generator(device=DEV).manual_seed(3)
    return [{"k": torch.randn(1, window, HEADS, 128, device=DEV, generator=gd).to(BF), "v": torch.randn(1, window, HEADS, 128, device=DEV, generator=gd).to(BF),
             "global_end_index": 0, "local_end_index": 0} for _ in range(layers)]


def cache_bytes(kv):
    return sum(t.numel() * t.element_size() for c in kv for t in c.values() if torch.is_tensor(t))


class Rig:
    """One mode of the sharded forward on the shared model: selecting it puts the model into the mode (the fp8 epoch bumps: the shadow
    mode's next forward refills its shadows once, outside the timed window)."""

    def __init__(self, model, wr, inputs, ca, kv, mode, splits, start):
        self.model, self.wr, self.inputs, self.ca, self.kv, self.mode, self.start = model, wr, inputs, ca, kv, mode, start
        self.cp = SimulatedContextParallel(WORLD, "rows", attn_kv_splits=splits)

    def select(self):
        m = self.model
        m.context_parallel, m.use_hip_graphs = self.cp, False
        m.disable_fp8_attention()
        if self.mode == "compact_cp":
            m.enable_fp8_attention(bf16_cache=False, context_parallel="codes")
        else:
            m.enable_fp8_attention(context_parallel=True)
        self.forward()
        self.forward()

    def forward(self):
        lat, cond, t = self.inputs
        for c in self.kv:
            c["global_end_index"] = c["local_end_index"] = self.start
        return self.wr(lat, cond, t, self.kv, self.ca, current_start=self.start)[0]

    def block_ms(self):
        self.select()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            self.forward()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def model_sections(layers, rounds, windows):
    model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                           device=DEV).init_random_weights(seed=0)
    wr = WanDiffusionWrapper(model, timestep_shift=5.0)
    g = torch.Generator().manual_seed(2)
    inputs = (torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV), {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]},
              torch.tensor([[500.0, 500.0, 500.0]], device=DEV))
    ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
           "is_init": False} for _ in range(layers)]
    warm = new_caches(model, "shadow_cp", layers, M)
    wr(*inputs, warm, ca, current_start=0)                                       # fills the text caches, unsharded
    planned = attn_kv_splits_for(WORLD, HEADS)
    # warm-up of both modes on a one-block cache: the eight workspaces, the split partials and the staging buffer exist from here on
    for mode in MODES:
        kv = warm if mode == "shadow_cp" else new_caches(model, mode, layers, M)
        Rig(model, wr, inputs, ca, kv, mode, planned, 0).select()
        del kv
    del warm
    memory, block = {}, {}
    for window in windows:
        memory[str(window)] = {}
        for mode in MODES:                                                       # each mode's cache alone
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            kv = new_caches(model, mode, layers, window)
            Rig(model, wr, inputs, ca, kv, mode, planned, window - M).select()
            torch.cuda.synchronize()
            memory[str(window)][mode] = {"cache_bytes": cache_bytes(kv), "peak_allocated_above_baseline": torch.cuda.max_memory_allocated() - base,
                                         "baseline_allocated": base}
            del kv
        gc.collect()
        torch.cuda.empty_cache()
        rigs = {mode: Rig(model, wr, inputs, ca, new_caches(model, mode, layers, window), mode, planned, window - M) for mode in MODES}
        r = interleaved({m: rig.block_ms for m, rig in rigs.items()}, rounds, lambda f: f())
        r["compact_vs_shadow_pct"] = 100.0 * (r["compact_cp"]["median"] / r["shadow_cp"]["median"] - 1)
        block[str(window)] = r
        del rigs
    return {"layers": layers, "world": WORLD, "exchange": "rows", "attn_kv_splits": planned, "hip_graphs": False, "rounds": rounds}, memory, block


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5, help="repeats per mode (at least five)")
    ap.add_argument("--iters", type=int, default=20, help="launches per kernel sample")
    ap.add_argument("--windows", default=",".join(str(w) for w in WINDOWS))
    ap.add_argument("--only", default="kernel,model", help="comma-separated sections to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_attn_fp8_only_cp.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this is a measurement: it needs the GPU")
    if args.rounds < 5:
        raise SystemExit("at least five repeats")
    ops.ensure_gemm_workspace(DEV)
    only = set(args.only.split(","))
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res.update({"device": torch.cuda.get_device_name(0), "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS, "world": WORLD},
                "gpus": 1, "real_checkpoint": False})
    # received per rank and layer by the all-gather of the row exchange: (world - 1) / world of the block's K and V rows
    res["exchange_bytes_per_rank_and_layer"] = {"computed_from_shapes": True, "shadow_cp_bf16_rows": 2 * M * D * 2 * (WORLD - 1) // WORLD,
                                                "compact_cp_codes": 2 * M * D * (WORLD - 1) // WORLD}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    if "kernel" in only:
        res["kernel_rounds"], res["kernel_iters"] = args.rounds, args.iters
        res["kernel_us"] = kernel_section(args.rounds, args.iters)
        save()
    if "model" in only:
        res["setup"], res["memory"], res["block_ms"] = model_sections(args.layers, args.rounds, [int(w) for w in args.windows.split(",")])
        save()
    brief = {"kernel_us": {m: round(v["median"], 1) for m, v in res.get("kernel_us", {}).items() if "median" in v},
             "block_ms": {w: {m: round(v["median"], 1) if isinstance(v, dict) else round(v, 2) for m, v in r.items()} for w, r in res.get("block_ms", {}).items()},
             "memory_GB": {w: {m: {k: round(v / 1e9, 2) for k, v in d.items()} for m, d in r.items()} for w, r in res.get("memory", {}).items()}}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
