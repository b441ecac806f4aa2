"""TAEHV against the Wan VAE decoder on one GPU, in one process (832 x 480: latent 60 x 104, one 3-latent block):

  * decode time per steady-state block (a continuing stream: 12 frames per call) of TAEHVDecoder and VAEDecoderWrapper;
  * the 1.3B-shaped GenerationSession block (Wan2.1-T2V-1.3B architecture, random weights, 4 denoising steps, the reference's
    first-frame re-encode on the Wan encoder) with use_taehv off and on;
  * the per-stream arena of each decoder.

    python scripts/taehv_bench.py [--iters 20] [--blocks 4] [--out profiles/r07_taehv_decode.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_decoder(dec, z, iters):
    """ms per steady-state call (the stream is started once, then continued) from device events over `iters` calls."""
    _, state = dec(z, *([None] * 55))
    for _ in range(3):
        _, state = dec(z, *state)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        px, state = dec(z, *state)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, px


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4, help="timed session blocks per mode (after 2 warm-up blocks)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_taehv_decode.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "taehv_bench needs a GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    from realtime_video_amd.taehv import TAEHVDecoder, arena_bytes
    from realtime_video_amd.vae_decoder import VAEDecoderWrapper

    h, w = 60, 104
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn(1, 3, 16, h, w, generator=g, device=dev).half()
    taehv = TAEHVDecoder(dev).init_random_weights(1)
    wan = VAEDecoderWrapper(dev).init_random_weights(seed=1)
    res = {"latent": [h, w], "pixels": [8 * h, 8 * w], "latent_frames_per_block": 3, "frames_per_block": 12}
    # alternate the two decoders (shared box: a drift hits both)
    t_taehv, t_wan = [], []
    for _ in range(2):
        t_taehv.append(time_decoder(taehv, z, args.iters)[0])
        t_wan.append(time_decoder(wan, z, args.iters)[0])
    res["taehv_decode_ms"] = min(t_taehv)
    res["wan_decode_ms"] = min(t_wan)
    res["taehv_decode_ms_runs"], res["wan_decode_ms_runs"] = t_taehv, t_wan
    res["speedup"] = res["wan_decode_ms"] / res["taehv_decode_ms"]
    res["taehv_arena_bytes"] = arena_bytes(h, w, 3)
    res["wan_arena_bytes"] = int(wan._new_arena(h, w).numel())
    flop = 0.0   # multiply-adds x 2 of the TAEHV decoder per steady-state block (T = 3), from the layer shapes
    T = 3
    flop += 2 * T * h * w * 9 * 32 * 256                                              # conv_in (Cin padded to 32)
    for s, C in enumerate((256, 128, 64)):
        F = T if s < 2 else 2 * T
        flop += 3 * 2 * F * (h << s) * (w << s) * 9 * C * C * (2 + 1 + 1)             # MemBlocks: conv.0 over 2C, conv.2, conv.4
    flop += 2 * T * (2 * h) * (2 * w) * 9 * 256 * 128 + 2 * T * (4 * h) * (4 * w) * 9 * 128 * 128   # folded TGrow + conv
    flop += 2 * 2 * T * (8 * h) * (8 * w) * 9 * 64 * 128 + 2 * 4 * T * (8 * h) * (8 * w) * 9 * 64 * 32   # fold 3, head (32 filters run)
    res["taehv_tflop_per_block"] = flop / 1e12
    res["taehv_tflops_achieved"] = flop / (res["taehv_decode_ms"] * 1e-3) / 1e12
    print(json.dumps(res), flush=True)

    # ---- 1.3B-shaped session block, use_taehv off / on
    from realtime_video_amd.causal_model import CausalWanModel
    from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
    from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
    from realtime_video_amd.vae_encoder import VAEEncoderWrapper
    from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
    model = CausalWanModel(dim=1536, ffn_dim=8960, num_heads=12, num_layers=30, text_dim=4096, freq_dim=256,
                           device=dev).init_random_weights(seed=0)
    wr = WanDiffusionWrapper(model, timestep_shift=5.0)
    enc = VAEEncoderWrapper(device=dev).init_random_weights(seed=2)
    prompt = torch.zeros(1, 512, 4096, dtype=torch.bfloat16, device=dev)
    prompt[:, :64] = torch.randn(1, 64, 4096, generator=g, device=dev).to(torch.bfloat16)

    def session_ms(use_taehv):
        pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 750, 500, 250]), dev,
                                       generator=wr)
        models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(prompt), vae_decoder=wan,
                        vae_encoder=enc, taehv_decoder=taehv)
        params = GenerateParams(prompt="synthetic", seed=42, num_blocks=2 + args.blocks, num_denoising_steps=4)
        sess = GenerationSession(params, models, device=dev, use_taehv=use_taehv)
        for _ in range(2):
            sess.generate_block()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.blocks):
            sess.generate_block()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.blocks

    runs_off, runs_on = [], []
    for _ in range(2):
        runs_off.append(session_ms(False))
        runs_on.append(session_ms(True))
    res["session_block_ms_wan"] = min(runs_off)
    res["session_block_ms_taehv"] = min(runs_on)
    res["session_block_ms_wan_runs"], res["session_block_ms_taehv_runs"] = runs_off, runs_on
    res["session_note"] = ("Wan2.1-T2V-1.3B architecture, random weights, 4 denoising steps, keep_first_frame=False (first-frame "
                           "re-encode on the Wan encoder), eager; wall clock over the timed blocks ending in a device synchronise")
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
