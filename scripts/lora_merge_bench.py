"""The LoRA merge kernel (rtv_lora_merge) beside a plain copy, on one GPU in one process.

Per matrix shape of the 14B model (5120 x 5120, 13824 x 5120, 5120 x 13824) and rank 16 / 64 / 256:
  * merge_ms = one rtv_lora_merge of base into W with one adapter,
  * copy_ms  = W.copy_(base) on the same buffers,
from device events around `iters` back-to-back calls, the two alternating for `rounds` rounds; the median of the rounds is
reported next to all rounds, and ratio = merge_ms / copy_ms.  Every call takes the next of `pool` buffer pairs, sized so that one
pass over the pool moves more than the 256 MB of the last-level cache: both kernels stream from and to HBM, as they do in a model.

whole_model: the re-merge of every LoRA-able matrix of the 14B model (40 layers x {q, k, v row blocks of qkv_w, o, cross q / k /
v / o, ffn.0, ffn.2}, 14.05 G parameters) as the model issues it - one launch per matrix or row block, in place (base == W is not
used: every matrix has a base copy, as in CausalWanModel) - over the buffers of `--layers` layers taken in turn, and the same
traffic as copies.

    python scripts/lora_merge_bench.py [--iters 10] [--rounds 5] [--out profiles/r12_lora_merge.json]

--ext: the extended merges (include/rtv_hip_lora_ext.h) instead, into --ext-out (profiles/r19_lora_ext.json).  Per matrix shape and
rank 16 / 64, alternating in every round on the same buffers:
  * merge         = rtv_lora_merge with one adapter (the kernel the extended ones are measured against),
  * ex_lowrank    = rtv_lora_merge_ex with the same pair and no diff (the same arithmetic through the new kernel),
  * ex_diff       = rtv_lora_merge_ex with the pair and a dense [N, K] diff (reads 2 N K bytes more),
  * ex_diff_only  = rtv_lora_merge_ex with the diff alone,
  * dora          = rtv_lora_merge_dora (two launches: base and the low-rank operands are read twice),
  * copy          = W.copy_(base).
The diffs rotate through the pool like the bases, so they stream from HBM too.  No threshold: the numbers are recorded.

    python scripts/lora_merge_bench.py --ext [--iters 10] [--rounds 5] [--ext-out profiles/r19_lora_ext.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIM, FFN, LAYERS = 5120, 13824, 40
SHAPES = [(DIM, DIM), (FFN, DIM), (DIM, FFN)]
RANKS = [16, 64, 256]
BF = torch.bfloat16


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(fns, iters, rounds):
    """{name: [ms per call, one per round]}: the candidates alternate inside every round."""
    for fn in fns.values():
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(events(fn, iters))
    return out


def rnd(*shape, std):
    return (std * torch.randn(*shape, device="cuda", dtype=torch.float32)).to(BF)


def extended(args, lora):
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "shapes": []}
    for N, K in SHAPES:
        pool = max(2, -(-(1 << 30) // (4 * N * K)))
        bases = [rnd(N, K, std=0.02) for _ in range(pool)]
        diffs = [rnd(N, K, std=0.01) for _ in range(pool)]
        outs = [torch.empty(N, K, dtype=BF, device="cuda") for _ in range(pool)]
        ws = torch.empty(lora.dora_workspace_bytes(N, K), dtype=torch.uint8, device="cuda")
        mag = (bases[0].float().norm(dim=1)).to(BF)
        for rank in RANKS[:2]:
            A, B = rnd(rank, K, std=0.05), rnd(N, rank, std=0.05)
            runs = interleaved({
                "merge": lambda i: lora.merge(bases[i % pool], outs[i % pool], [(A, B, 0.7)]),
                "ex_lowrank": lambda i: lora.merge_ex(bases[i % pool], outs[i % pool], [(A, B, 0.7, None, 0.0)]),
                "ex_diff": lambda i: lora.merge_ex(bases[i % pool], outs[i % pool], [(A, B, 0.7, diffs[i % pool], 0.7)]),
                "ex_diff_only": lambda i: lora.merge_ex(bases[i % pool], outs[i % pool], [(None, None, 0.0, diffs[i % pool], 0.7)]),
                "dora": lambda i: lora.merge_dora(bases[i % pool], outs[i % pool], A, B, 0.5, mag, 0.7, ws),
                "copy": lambda i: outs[i % pool].copy_(bases[i % pool])}, args.iters, args.rounds)
            med = {k: statistics.median(v) for k, v in runs.items()}
            nk = float(N) * K
            moved = {"merge": 4 * nk, "ex_lowrank": 4 * nk, "ex_diff": 6 * nk, "ex_diff_only": 6 * nk, "dora": 6 * nk, "copy": 4 * nk}
            row = {"N": N, "K": K, "rank": rank, "pool": pool}
            for k in runs:
                row[k + "_ms"] = med[k]
                row[k + "_gbps"] = moved[k] / med[k] / 1e6
                if k != "merge":
                    row[k + "_over_merge"] = med[k] / med["merge"]
            row["rounds_ms"] = runs
            result["shapes"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "rounds_ms"}), flush=True)
        del bases, diffs, outs
    os.makedirs(os.path.dirname(os.path.abspath(args.ext_out)), exist_ok=True)
    with open(args.ext_out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.ext_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=2, help="layers' worth of buffers the whole-model pass rotates over")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_lora_merge.json"))
    ap.add_argument("--ext", action="store_true", help="time rtv_lora_merge_ex / rtv_lora_merge_dora beside rtv_lora_merge instead")
    ap.add_argument("--ext-out", default=os.path.join(ROOT, "profiles", "r19_lora_ext.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lora_merge_bench needs a GPU"
    from realtime_video_amd import lora
    torch.manual_seed(0)
    if args.ext:
        return extended(args, lora)
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "shapes": []}
    for N, K in SHAPES:
        pool = max(2, -(-(1 << 30) // (4 * N * K)))          # a pass over the pool reads + writes more than 1 GiB
        bases = [rnd(N, K, std=0.02) for _ in range(pool)]
        outs = [torch.empty(N, K, dtype=BF, device="cuda") for _ in range(pool)]
        for rank in RANKS:
            A, B = rnd(rank, K, std=0.05), rnd(N, rank, std=0.05)
            ad = [(A, B, 0.7)]
            runs = interleaved({"merge": lambda i: lora.merge(bases[i % pool], outs[i % pool], ad),
                                "copy": lambda i: outs[i % pool].copy_(bases[i % pool])}, args.iters, args.rounds)
            m, c = statistics.median(runs["merge"]), statistics.median(runs["copy"])
            moved = 4.0 * N * K + 2.0 * rank * (N + K)
            row = {"N": N, "K": K, "rank": rank, "pool": pool, "merge_ms": m, "copy_ms": c, "ratio": m / c,
                   "merge_gbps": moved / m / 1e6, "copy_gbps": 4.0 * N * K / c / 1e6, "merge_rounds_ms": runs["merge"],
                   "copy_rounds_ms": runs["copy"]}
            result["shapes"].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("rounds_ms")}), flush=True)
        del bases, outs
    # whole model: per layer 3 + 5 launches over [5120, 5120] (row blocks of qkv_w; o, cq, ck, cv, co), ffn.0 and ffn.2
    per_layer = [(DIM, DIM)] * 8 + [(FFN, DIM), (DIM, FFN)]
    bufs = [[(rnd(N, K, std=0.02), torch.empty(N, K, dtype=BF, device="cuda")) for N, K in per_layer] for _ in range(args.layers)]
    result["whole_model"] = []
    for rank in RANKS[:2]:
        ads = [[(rnd(rank, K, std=0.05), rnd(N, rank, std=0.05), 0.7)] for N, K in per_layer]

        def remerge(_):
            for l in range(LAYERS):
                for (base, out), ad in zip(bufs[l % args.layers], ads):
                    lora.merge(base, out, ad)

        def copies(_):
            for l in range(LAYERS):
                for base, out in bufs[l % args.layers]:
                    out.copy_(base)

        runs = interleaved({"merge": remerge, "copy": copies}, 1, args.rounds)
        m, c = statistics.median(runs["merge"]), statistics.median(runs["copy"])
        row = {"rank": rank, "layers": LAYERS, "launches": LAYERS * len(per_layer), "parameters": LAYERS * sum(n * k for n, k in per_layer),
               "buffer_layers": args.layers, "remerge_ms": m, "copy_ms": c, "ratio": m / c, "remerge_rounds_ms": runs["merge"],
               "copy_rounds_ms": runs["copy"]}
        result["whole_model"].append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("rounds_ms")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
