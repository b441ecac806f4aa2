"""The KV split of the fp8 attention kernel and the fp8 context-parallel phases (include/rtv_hip_attn_fp8_cp.h) beside their bf16
counterparts, in one process, the variants alternating.  Writes profiles/r22_attn_fp8_cp.json (or --out; sections already in that
file are kept, so --only can run the parts in several visits) with

  kernel_us   (a) rtv_attn_fwd_fp8_split against rtv_attn_fwd_split (bf16) on the two launches of a context-parallel rank of the 14B
              model at 8 ranks - Lq = 4680 x H = 5 (head exchange) and Lq = 585 x H = 40 (row exchange) - over 9360, 18720 and 32760
              keys, S = 1, 2, 4 ranges: device events, median / min / max of --rounds rounds, and per variant the spread between the
              two halves of its rounds (what the box does to an unchanged program).
  block_ms    (b) five 40-layer forwards back to back = the DiT work of one block, under SimulatedContextParallel(8) (all eight
              ranks in lockstep on ONE GPU: eight times a rank's work, no communication), both exchanges, fp8 attention against
              bf16 attention, S from parallel.attn_kv_splits_for and S = 1, over a window of --window rows; host clock around a
              device synchronise, same statistics.  No run on more than one GPU and no real checkpoint is involved."""
import argparse
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
from realtime_video_amd.wan_wrapper import WanDiffusionWrapper                          # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
M, D, FFN, HEADS, WORLD = 4680, 5120, 13824, 40, 8
LAUNCHES = ((4680, 5), (585, 40))
KEYS = (9360, 18720, 32760)
SPLITS = (1, 2, 4)


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
    out = {}
    for Lq, H in LAUNCHES:
        for Lkv in KEYS:
            g = torch.Generator(device=DEV).manual_seed(Lq + Lkv)
            q = torch.randn(Lq, H, 128, device=DEV, generator=g).to(BF)
            k, v = (torch.randn(Lkv, H, 128, device=DEV, generator=g).to(BF) for _ in range(2))
            k8, v8t = ops.attn_fp8_shadow(Lkv, H, DEV)
            ops.attn_quantize_kv(k, v, k8, v8t)
            o8, o16 = torch.empty_like(q), torch.empty_like(q)
            ws = torch.empty(max(SPLITS) * H * Lq * 130, dtype=torch.float32, device=DEV)
            fns = {}
            for S in SPLITS:
                fns[f"fp8_S{S}"] = lambda S=S: ops.attn_fwd_fp8(q, k8, v8t, (0, Lkv), out=o8, kv_splits=S, workspace=ws)
                fns[f"bf16_S{S}"] = lambda S=S: ops.attn_fwd_split(q[None], k[None], v[None], (0, Lkv), kv_splits=S, out=o16[None], workspace=ws)
            r = interleaved(fns, rounds, lambda f: 1e3 * event_ms(f, iters))
            for S in SPLITS:
                r[f"fp8_vs_bf16_S{S}_pct"] = 100.0 * (r[f"fp8_S{S}"]["median"] / r[f"bf16_S{S}"]["median"] - 1)
            r["rel_l2_fp8_vs_bf16"] = float((o8.float() - o16.float()).norm() / o16.float().norm())
            out[f"Lq{Lq}_H{H}_keys{Lkv}"] = r
            del q, k, v, k8, v8t, ws
            torch.cuda.empty_cache()
    return out


class Rig:
    """One variant of the sharded forward on the shared model and caches: selecting it puts the model into its mode (the fp8 epoch
    bumps: the next forward refills the shadows once, outside the timed window)."""

    def __init__(self, model, caches, exchange, fp8, splits, graphs):
        self.model, self.caches, self.fp8 = model, caches, fp8
        self.cp = SimulatedContextParallel(WORLD, exchange, attn_kv_splits=splits)
        self.graphs = graphs

    def select(self):
        m = self.model
        m.context_parallel, m.use_hip_graphs = self.cp, self.graphs
        m.disable_fp8_attention()
        if self.fp8:
            m.enable_fp8_attention(context_parallel=True)
        self.forward()
        self.forward()
        self.forward()      # (with graphs: eager, capture, replay)

    def forward(self):
        wr, lat, cond, t, kv, ca, start = self.caches
        for c in kv:
            c["global_end_index"] = c["local_end_index"] = start
        return wr(lat, cond, t, kv, ca, current_start=start)[0]

    def block_ms(self):
        self.select()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            self.forward()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)


def block_section(layers, window, rounds, graphs):
    model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                           device=DEV).init_random_weights(seed=0)
    wr = WanDiffusionWrapper(model, timestep_shift=5.0)
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV)
    cond = {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]}
    t = torch.tensor([[500.0, 500.0, 500.0]], device=DEV)
    gd = torch.Generator(device=DEV).manual_seed(3)
    kv = [{"k": torch.randn(1, window, HEADS, 128, device=DEV, generator=gd).to(BF), "v": torch.randn(1, window, HEADS, 128, device=DEV, generator=gd).to(BF),
           "global_end_index": 0, "local_end_index": 0} for _ in range(layers)]
    ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
           "is_init": False} for _ in range(layers)]
    wr(lat, cond, t, kv, ca, current_start=0)                                   # fills the text caches, unsharded
    caches = (wr, lat, cond, t, kv, ca, window - M)
    planned = attn_kv_splits_for(WORLD, HEADS)
    out = {"layers": layers, "window_rows": window, "world": WORLD, "attn_kv_splits_for": planned, "hip_graphs": bool(graphs), "rounds": rounds}
    for exchange in ("heads", "rows"):
        rigs = {f"{'fp8' if fp8 else 'bf16'}_S{S}": Rig(model, caches, exchange, fp8, S, graphs)
                for S in sorted({1, planned}) for fp8 in (True, False)}
        r = interleaved({m: rig.block_ms for m, rig in rigs.items()}, rounds, lambda f: f())
        for S in sorted({1, planned}):
            r[f"fp8_vs_bf16_S{S}_pct"] = 100.0 * (r[f"fp8_S{S}"]["median"] / r[f"bf16_S{S}"]["median"] - 1)
        out[exchange] = r
        model._graphs.clear()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--window", type=int, default=32760, help="rows of the KV cache = keys of the attention window (c = 9: 32760)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20, help="launches per kernel sample")
    ap.add_argument("--graphs", action="store_true", help="replay the sharded forwards as hipGraphs (takes the host out of block_ms)")
    ap.add_argument("--only", default="kernel,block", help="comma-separated sections to run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_attn_fp8_cp.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    ops.ensure_gemm_workspace(DEV)
    only = set(args.only.split(","))
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res.update({"device": torch.cuda.get_device_name(0), "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS}})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    if "kernel" in only:
        res["kernel_rounds"], res["kernel_iters"] = args.rounds, args.iters
        res["kernel_us"] = kernel_section(args.rounds, args.iters)
        save()
    if "block" in only:
        res["block_ms"] = block_section(args.layers, args.window, args.rounds, args.graphs)
        save()
    brief = {"kernel_us": {k: {m: round(v["median"], 1) if isinstance(v, dict) else round(v, 2) for m, v in r.items()} for k, r in res.get("kernel_us", {}).items()},
             "block_ms": {x: {m: round(v["median"], 1) if isinstance(v, dict) else round(v, 2) for m, v in r.items()}
                          for x, r in res.get("block_ms", {}).items() if isinstance(r, dict)}}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
