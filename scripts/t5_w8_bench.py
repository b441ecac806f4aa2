"""The text encoder on e4m3 weights (WanTextEncoder.enable_fp8_weights, include/rtv_hip_t5_w8.h) against the bf16 encoder, one process,
random weights of the real architecture.  Writes profiles/r24_t5_w8.json (or the path given):
  * encode time per prompt length for both encoders, alternating, REPEATS windows each: median, min, max; a length counts as faster
    only when the medians differ by more than the larger of the two min-max spreads;
  * per Linear shape of a layer at 32 / 64 / 128 rows: rtv_gemm_w8, rtv_gemm (bf16, as the encoder launches it) and a device copy of
    the code bytes (the streaming yardstick), each over a rotation of weight copies larger than the last-level cache;
  * resident weight bytes before and after.
usage: t5_w8_bench.py [out.json] [--layers N]     (--layers: a shallower model for a rehearsal; the record says so)"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realtime_video_amd import _lib, ops  # noqa: E402
from realtime_video_amd.text_encoder import UMT5_XXL, WanTextEncoder  # noqa: E402

LENGTHS = (20, 77, 128, 256, 512)
ROWS = (32, 64, 128)
REPEATS = 7
ROTATION_BYTES = 1 << 30          # weight copies a timed loop walks through: four times the 256 MB last-level cache
DEV = "cuda"


def windows(fns, iters):
    """REPEATS timed windows of `iters` calls for every function, alternating between them; milliseconds per call."""
    for f in fns.values():
        f(0)
        f(1)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                f(i)
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / iters * 1e3)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms)}


def encode_times(enc16, enc8):
    rec = {}
    for n in LENGTHS:
        g = torch.Generator().manual_seed(n)
        ids = torch.randint(2, UMT5_XXL["vocab"], (1, 512), generator=g)
        mask = torch.zeros(1, 512, dtype=torch.long)
        mask[0, :n] = 1
        t = windows({"bf16": lambda i: enc16.encode_ids(ids, mask), "w8": lambda i: enc8.encode_ids(ids, mask)}, iters=10)
        a, b = summary(t["bf16"]), summary(t["w8"])
        gain = a["median_ms"] - b["median_ms"]
        rec[str(n)] = {"rows": (n + 31) // 32 * 32, "bf16": a, "w8": b, "gain_ms": gain,
                       "w8_faster_beyond_spread": gain > max(a["spread_ms"], b["spread_ms"])}
        print(f"{n:4d} tokens: bf16 {a['median_ms']:.3f} ms (spread {a['spread_ms']:.3f})  w8 {b['median_ms']:.3f} ms "
              f"(spread {b['spread_ms']:.3f})  gain {gain:.3f} ms", flush=True)
    return rec


def gemm_times():
    c = UMT5_XXL
    shapes = {"qk": (2 * c["dim_attn"], c["dim"]), "v_o": (c["dim"], c["dim_attn"]), "gate_fc1": (2 * c["dim_ffn"], c["dim"]),
              "fc2": (c["dim"], c["dim_ffn"])}
    lib = _lib.load()
    rec = {}
    for name, (N, K) in shapes.items():
        copies = max(2, -(-ROTATION_BYTES // (2 * N * K)))
        w16 = [(torch.randn(N, K, device=DEV) * K ** -0.5).to(torch.bfloat16) for _ in range(copies)]
        q8 = [ops.quantize_fp8_rows(w) for w in w16]
        dst = torch.empty(N * K, dtype=torch.uint8, device=DEV)
        for M in ROWS:
            a = torch.randn(M, K, device=DEV).to(torch.bfloat16)
            out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            ws = torch.empty(max(16, lib.rtv_gemm_w8_workspace_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            vp = ctypes.c_void_p

            def bf16(i):
                _lib.call("rtv_gemm", vp(a.data_ptr()), K, vp(w16[i % copies].data_ptr()), K, vp(out.data_ptr()), N, M, N, K, vp(0), 0,
                          vp(0), 0, 0, 0, vp(0), 0, 0, 0, st)

            def w8(i):
                q, s = q8[i % copies]
                ops.gemm_w8(a, q, s, out=out, workspace=ws)

            def copy(i):
                dst.copy_(q8[i % copies][0].view(torch.uint8).reshape(-1))

            t = {k: summary(v) for k, v in windows({"bf16": bf16, "w8": w8, "copy_of_code_bytes": copy}, iters=4 * copies).items()}
            for k, nbytes in (("bf16", 2 * N * K), ("w8", N * K)):
                t[k]["weight_GB_per_s"] = nbytes / t[k]["median_ms"] / 1e6
            t["copy_of_code_bytes"]["read_GB_per_s"] = N * K / t["copy_of_code_bytes"]["median_ms"] / 1e6
            t["segments"] = lib.rtv_gemm_w8_segments(N, K)
            rec[f"{name}_N{N}_K{K}_M{M}"] = t
            print(f"{name} N={N} K={K} M={M}: w8 {t['w8']['median_ms'] * 1e3:.1f} us ({t['w8']['weight_GB_per_s']:.0f} GB/s of codes)  "
                  f"bf16 {t['bf16']['median_ms'] * 1e3:.1f} us ({t['bf16']['weight_GB_per_s']:.0f} GB/s)  copy "
                  f"{t['copy_of_code_bytes']['median_ms'] * 1e3:.1f} us", flush=True)
        del w16, q8
    return rec


def main():
    args = sys.argv[1:]
    layers = UMT5_XXL["num_layers"]
    if "--layers" in args:
        i = args.index("--layers")
        layers = int(args[i + 1])
        del args[i:i + 2]
    path = args[0] if args else os.path.join(ROOT, "profiles", "r24_t5_w8.json")
    if not torch.cuda.is_available():
        raise SystemExit("t5_w8_bench needs a GPU: nothing here can be measured without one")
    enc16 = WanTextEncoder(device=DEV, num_layers=layers).init_random_weights(seed=0)
    enc8 = WanTextEncoder(device=DEV, num_layers=layers).init_random_weights(seed=0)
    before = enc8.weight_bytes()
    enc8.enable_fp8_weights()
    torch.cuda.synchronize()
    rec = {"device": torch.cuda.get_device_properties(0).name, "num_layers": layers, "repeats": REPEATS,
           "weight_bytes": {"bf16": before, "w8": enc8.weight_bytes()}, "encode": encode_times(enc16, enc8)}
    del enc16, enc8
    torch.cuda.empty_cache()
    rec["gemm"] = gemm_times()
    rec["faster_at_every_length_up_to_128"] = all(v["w8_faster_beyond_spread"] for n, v in rec["encode"].items() if int(n) <= 128)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", path, "| faster at every length <= 128 tokens beyond the spread:", rec["faster_at_every_length_up_to_128"])


if __name__ == "__main__":
    main()
