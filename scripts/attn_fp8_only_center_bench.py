"""K smoothing on the e4m3-only KV cache (enable_fp8_attention(bf16_cache=False, smooth_k="codes"),
include/rtv_hip_attn_fp8_only_center.h), measured in one process with the variants alternating.  Writes
profiles/r25_attn_fp8_only_center.json (or --out) with

  rope_k8    rtv_qk_norm_rope_k8_centered against rtv_qk_norm_rope_k8 at d = 5120, M = 4680: microseconds per launch (device events
             around --launches launches), median / min / max of --rounds rounds, and the bytes moved per second.
  recentre   one recentre of --layers layers at 9360 and 32760 rows - per layer the mean of the codes, the move of the rows, the copy
             of the centre - against a device copy of the same code bytes and against what the shadow mode pays for a recentre: the
             mean of the bf16 keys plus the centred refill of the shadows from the bf16 cache.
  block_ms   five forwards back to back whose key window is the whole 9360-row window = the DiT work of one block: the compact mode
             under non-zero centres ("codes") against the plain compact mode ("only") and the shadow mode under smooth_k=True
             ("smooth"), host clock around a device synchronise.

Every figure comes with the spread between the first and the second half of its rounds (what the machine does to an unchanged
program).  No speed is claimed: the file records what came out."""
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
from realtime_video_amd.rope import rope_cos_sin_table               # noqa: E402
from realtime_video_amd.wan_wrapper import WanDiffusionWrapper       # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
M, D, FFN, HEADS = 4680, 5120, 13824, 40
GRID = (3, 30, 52)


def summary(xs):
    half = len(xs) // 2
    out = {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": xs}
    if half >= 2:
        a, b = statistics.median(xs[:half]), statistics.median(xs[half:])
        out["first_vs_second_half_pct"] = 100.0 * (b - a) / a
    return out


def device_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def alternate(variants, rounds, launches):
    for fn in variants.values():
        device_us(fn, 3)
    samples = {n: [] for n in variants}
    for _ in range(rounds):
        for n, fn in variants.items():
            samples[n].append(device_us(fn, launches))
    return {n: summary(v) for n, v in samples.items()}


def bench_rope(rounds, launches):
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(M, 3 * D, generator=g).to(BF).to(DEV)
    wq, wk = (torch.randn(D, generator=g).mul(0.1).add(1).to(BF).to(DEV) for _ in range(2))
    cs = rope_cos_sin_table(128).to(DEV)
    k8 = torch.zeros(2 * M, HEADS, 128, dtype=torch.uint8, device=DEV)
    q = torch.empty(M, D, dtype=BF, device=DEV)
    amax = torch.zeros(2, device=DEV)
    center = torch.randn(HEADS, 128, generator=g).to(DEV)
    out = alternate({
        "plain": lambda: ops.qk_norm_rope_k8(qkv, k8, M, HEADS, wq, wk, cs, GRID, 3, q_out=q, amax=amax),
        "centred": lambda: ops.qk_norm_rope_k8_centered(qkv, k8, M, HEADS, wq, wk, cs, GRID, 3, center, q_out=q, amax=amax)}, rounds, launches)
    nbytes = 7.0 * M * D                                            # q read and written as bf16, k read as bf16 and written as codes
    for v in out.values():
        v["TB_per_s"] = nbytes / (v["median"] * 1e-6) / 1e12
    out["centred_vs_plain_pct"] = 100.0 * (out["centred"]["median"] - out["plain"]["median"]) / out["plain"]["median"]
    return out


def bench_recentre(rows, layers, rounds):
    g = torch.Generator(device=DEV).manual_seed(rows)
    kc = [torch.randn(rows, HEADS, 128, generator=g, device=DEV, dtype=BF) for _ in range(layers)]
    vc = [torch.randn(rows, HEADS, 128, generator=g, device=DEV, dtype=BF) for _ in range(layers)]
    for k in kc:
        k[:, :, ::8] += 8.0
    sh = [ops.attn_fp8_shadow(rows, HEADS, DEV) for _ in range(layers)]
    scratch = torch.empty_like(sh[0][0])
    c_a, c_b = torch.zeros(layers, HEADS, 128, device=DEV), torch.zeros(layers, HEADS, 128, device=DEV)
    ws = torch.empty(max(ops.attn_kv_center_workspace_bytes(rows, HEADS), 16) // 4, device=DEV)
    amax = torch.zeros(layers, 2, device=DEV)
    for l in range(layers):
        ops.attn_quantize_kv(kc[l], vc[l], *sh[l], 0, rows)

    def codes():                                                     # what fp8_attention_recenter issues on compact dicts
        for l in range(layers):
            ops.attn_k8_center(sh[l][0], (0, rows), c_old=c_a[l], out=c_b[l], workspace=ws)
            ops.attn_k8_recenter(sh[l][0], c_a[l], c_b[l], 0, rows, amax=amax[l])
            c_a[l].copy_(c_b[l])

    def copy():
        for l in range(layers):
            scratch.copy_(sh[l][0])

    def shadow():                                                    # the shadow mode: the bf16 mean, then the centred refill
        for l in range(layers):
            ops.attn_kv_center(kc[l], (0, rows), out=c_b[l], workspace=ws)
            ops.attn_quantize_kv(kc[l], vc[l], *sh[l], 0, rows, amax=amax[l], center=c_b[l])

    out = alternate({"codes": codes, "copy_of_the_codes": copy, "shadow_mean_and_refill": shadow}, rounds, 1)
    nbytes = float(layers) * rows * HEADS * 128
    out["code_bytes"] = nbytes
    out["codes"]["TB_per_s_read_plus_written"] = 3.0 * nbytes / (out["codes"]["median"] * 1e-6) / 1e12      # mean: read; move: read + write
    out["copy_of_the_codes"]["TB_per_s_read_plus_written"] = 2.0 * nbytes / (out["copy_of_the_codes"]["median"] * 1e-6) / 1e12
    out["codes_vs_copy"] = out["codes"]["median"] / out["copy_of_the_codes"]["median"]
    out["codes_vs_shadow"] = out["codes"]["median"] / out["shadow_mean_and_refill"]["median"]
    return out


class Rig:
    """The shared model in one mode with a KV cache of `window` rows of its kind; every forward rewrites the last M rows and attends
    all `window` rows.  The centres are the model's, shared by the modes: the "smooth" rig, built first, sets them with a recentre
    behind its first forward; the "codes" rig installs the same ones in front of its first row, so all its rows are coded once."""

    def __init__(self, model, wr, mode, window, inputs, ca):
        self.model, self.wr, self.mode, self.window = model, wr, mode, window
        self.lat, self.cond, self.t = inputs
        self.ca = ca
        self.enter()
        if mode in ("only", "codes"):
            self.kv = model.new_fp8_kv_cache(window, DEV)
        else:
            self.kv = [{"k": torch.zeros(1, window, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, window, HEADS, 128, dtype=BF, device=DEV),
                        "global_end_index": 0, "local_end_index": 0} for _ in range(model.num_layers)]
        if mode == "codes":                                          # (before its first row: nothing to move, no second rounding)
            model.fp8_attention_set_centers(model._fp8_attention.center.clone(), self.kv)
        for c in self.kv:
            c["global_end_index"] = c["local_end_index"] = window - M
        self.forward()
        if mode == "smooth":
            model.fp8_attention_recenter(self.kv)
            assert bool(model._fp8_attention.center.any())
            self.forward()
        torch.cuda.synchronize()

    def enter(self):
        """Switch the shared model to this rig's mode.  The shadow mode refills its shadows from the whole bf16 cache in the first
        forward behind a switch: that forward runs here, outside every timing."""
        self.model.enable_fp8_attention(bf16_cache=self.mode == "smooth", smooth_k={"codes": "codes", "smooth": True}.get(self.mode, False))
        if hasattr(self, "kv"):
            self.forward()

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


def bench_blocks(layers, rounds, window):
    ops.ensure_gemm_workspace(DEV)
    model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                           device=DEV).init_random_weights(seed=0)
    wr = WanDiffusionWrapper(model, timestep_shift=5.0)
    g = torch.Generator().manual_seed(2)
    inputs = (torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV),
              {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]}, torch.tensor([[500.0, 500.0, 500.0]], device=DEV))
    ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
           "is_init": False} for _ in range(layers)]
    rigs = {mode: Rig(model, wr, mode, window, inputs, ca) for mode in ("smooth", "only", "codes")}
    for r in rigs.values():
        r.block_ms()
    samples = {m: [] for m in rigs}
    for _ in range(rounds):
        for m, r in rigs.items():
            samples[m].append(r.block_ms())
    out = {m: summary(v) for m, v in samples.items()}
    for other in ("only", "smooth"):
        out[f"codes_vs_{other}_pct"] = 100.0 * (out["codes"]["median"] - out[other]["median"]) / out[other]["median"]
    out["window"] = window
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--windows", default="9360,32760")
    ap.add_argument("--parts", default="rope,recentre,blocks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_attn_fp8_only_center.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    parts = args.parts.split(",")
    res = {"device": torch.cuda.get_device_name(0), "layers": args.layers, "rounds": args.rounds,
           "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS}}
    if os.path.exists(args.out):                                     # the parts may be measured in separate runs
        with open(args.out) as f:
            res = {**json.load(f), **res}
    if "rope" in parts:
        res["rope_k8_us"] = bench_rope(args.rounds, args.launches)
    if "recentre" in parts:
        res["recentre_us"] = {}
        for rows in [int(w) for w in args.windows.split(",") if w]:
            res["recentre_us"][str(rows)] = bench_recentre(rows, args.layers, args.rounds)
            gc.collect()
            torch.cuda.empty_cache()
    if "blocks" in parts:
        res["block_ms"] = bench_blocks(args.layers, args.rounds, 9360)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "shape"}, default=str)[:6000])


if __name__ == "__main__":
    main()
