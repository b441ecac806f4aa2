"""fp8 Linears: per-tensor scales (enable_fp8("tensor")) against per-row scales (enable_fp8("row")) on a 14B-shaped DiT, in one
process and interleaved.  Writes profiles/r13_fp8_rows.json (or --out) with

  quant_ms_per_layer   device-event time of what stands between the bf16 activations and the e4m3 GEMM operands of one layer at
                       M = 4680: tensor mode = 3 LayerNorms + 6 x (memset, absmax, quantise); row mode = 3 LayerNorm-fused
                       quantisers + 3 row quantisers.  Standalone launches on buffers of the layer's shapes (the input was last
                       touched by the previous launch, as in the forward), median of --rounds rounds, modes alternating.
  stream_ops           kernels + memsets of ONE forward (denoising step, 9360-row attention window), counted from a profiler trace of
                       that forward (`count`; null with the reason in `method` where the tracer does not work), and the
                       quantisation operations among them as the launch sequence of csrc/dit_forward.hip gives them.
  block_ms             five forwards back to back at a 9360-row window = the DiT work of one block (KV recompute + 4 denoising
                       steps; no VAE, no text encoder), host clock around a device synchronise; median, min and max of --rounds
                       rounds, modes alternating, plus the spread between the first and the second half of the rounds of ONE mode
                       (what the box does to an unchanged program).

--modes tensor runs on a checkout that predates the row mode (the unchanged mode's own baseline on the same box)."""
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
M, D, FFN, HEADS, FS = 4680, 5120, 13824, 40, 1560


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


def quant_layer_fns(modes):
    """{mode: callable running one layer's LayerNorm + quantisation launches}."""
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(M, D, device=DEV, generator=g).to(BF)
    h = torch.randn(M, FFN, device=DEV, generator=g).to(BF)
    emod = (0.5 * torch.randn(3, 6, D, device=DEV, generator=g)).to(BF)
    wgt, bias = torch.ones(D, device=DEV, dtype=BF), torch.zeros(D, device=DEV, dtype=BF)
    xn = torch.empty_like(x)
    q, qh = (torch.empty(M, k, dtype=torch.float8_e4m3fn, device=DEV) for k in (D, FFN))
    mod = dict(shift=emod[0, 0], scale=emod[0, 1], frame_stride=6 * D, rows_per_frame=FS)

    def tensor():
        for kw in (mod, dict(weight=wgt, bias=bias), mod):           # qkv, cross-q, ffn.0: LayerNorm, then the quantiser
            ops.layernorm_modulate(x, 1e-6, out=xn, **kw)
            ops.quantize_fp8(xn, out=q)
        for _ in range(2):                                           # o, cross-o
            ops.quantize_fp8(x, out=q)
        ops.quantize_fp8(h, out=qh)                                  # ffn.2

    def row():
        for kw in (mod, dict(weight=wgt, bias=bias), mod):
            ops.layernorm_modulate_fp8_rows(x, 1e-6, **kw)
        for _ in range(2):
            ops.quantize_fp8_rows(x, out=q)
        ops.quantize_fp8_rows(h, out=qh)

    return {m: f for m, f in (("tensor", tensor), ("row", row)) if m in modes}


class Rig:
    """A 14B-shaped model in one fp8 mode with its caches, primed to a 9360-row attention window."""

    def __init__(self, mode, layers):
        self.model = CausalWanModel(dim=D, ffn_dim=FFN, num_heads=HEADS, num_layers=layers, text_dim=4096, freq_dim=256,
                                    device=DEV).init_random_weights(seed=0)
        if mode == "row":
            self.model.enable_fp8("row")
        else:
            self.model.enable_fp8()
        self.wr = WanDiffusionWrapper(self.model, timestep_shift=5.0)
        g = torch.Generator().manual_seed(2)
        self.lat = torch.randn(1, 3, 16, 60, 104, generator=g).to(BF).to(DEV)
        self.cond = {"prompt_embeds": [torch.randn(64, 4096, generator=g).to(BF).to(DEV)]}
        self.t = torch.tensor([[500.0, 500.0, 500.0]], device=DEV)
        self.kv = [{"k": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 9360, HEADS, 128, dtype=BF, device=DEV),
                    "global_end_index": 0, "local_end_index": 0} for _ in range(layers)]
        self.ca = [{"k": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV), "v": torch.zeros(1, 512, HEADS, 128, dtype=BF, device=DEV),
                    "is_init": False} for _ in range(layers)]
        self.wr(self.lat, self.cond, self.t, self.kv, self.ca, current_start=0)
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

    def stream_ops(self, layers):
        # operations in front of the GEMMs, from the launch sequence of csrc/dit_forward.hip: a per-tensor Linear has 3 (memset, absmax,
        # quantise), a per-row Linear 1, and none when a LayerNorm feeds it; 4 Linears outside the layers (time MLP, projection, head)
        rows = self.model._cfg.use_fp8 == 2
        out = {"quantisation_ops_from_launch_sequence": (4 + 3 * layers) if rows else 3 * (4 + 6 * layers)}
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                self.forward()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
            out.update(count=n or None, method="device events (kernels, memsets, copies) of a torch.profiler trace of one forward")
        except Exception as e:                                       # noqa: BLE001 - a box without a working tracer still measures the rest
            out.update(count=None, method=f"not traced ({type(e).__name__}: {str(e)[:80]})")
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--modes", default="tensor,row")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_fp8_rows.json"))
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    ops.ensure_gemm_workspace(DEV)
    res = {"device": torch.cuda.get_device_name(0), "modes": modes, "layers": args.layers, "rounds": args.rounds,
           "shape": {"M": M, "dim": D, "ffn_dim": FFN, "num_heads": HEADS}}

    fns = quant_layer_fns(modes)
    for f in fns.values():
        event_ms(f, 5)
    samples = {m: [] for m in fns}
    for _ in range(args.rounds):
        for m, f in fns.items():
            samples[m].append(event_ms(f, 20))
    res["quant_ms_per_layer"] = {m: summary(v) for m, v in samples.items()}

    rigs = {m: Rig(m, args.layers) for m in modes}
    for r in rigs.values():
        r.block_ms()
    samples = {m: [] for m in rigs}
    for _ in range(args.rounds):
        for m, r in rigs.items():
            samples[m].append(r.block_ms())
    res["block_ms"] = {m: summary(v) for m, v in samples.items()}
    res["stream_ops"] = {m: r.stream_ops(args.layers) for m, r in rigs.items()}      # (traced last: the timed rounds ran untraced)
    if "tensor" in rigs and "row" in rigs:
        t, r = res["block_ms"]["tensor"]["median"], res["block_ms"]["row"]["median"]
        res["row_vs_tensor_block_pct"] = 100.0 * (r - t) / t
        a, b = rigs["tensor"].forward().float(), rigs["row"].forward().float()
        res["row_vs_tensor_output_rel_l2"] = float((a - b).norm() / a.norm())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "shape"}, default=str)[:3000])


if __name__ == "__main__":
    main()
