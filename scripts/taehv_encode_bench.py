"""The TAEHV encoder against the Wan VAE encoder on one GPU, in one process (832 x 480):

  * ms per steady-state 12-frame streamed encode (a continuing stream, 3 latents per call) of TAEHVEncoder and VAEEncoderWrapper;
  * ms per fresh one-frame encode (the session's first-frame re-encode site), both encoders;
  * the per-stream arena of each encoder;
  * the webcam-mode GenerationSession block at the 1.3B architecture (random weights, 4 denoising steps, use_taehv=True) with
    and without a taehv_encoder.

    python scripts/taehv_encode_bench.py [--iters 20] [--blocks 4] [--out profiles/r08_taehv_encode.json]
    python scripts/taehv_encode_bench.py --encode-only 10      # only steady-state TAEHV encodes: the workload to put under
                                                               # `rocprofv3 --kernel-trace --stats -- python ...`
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 480, 832


def time_stream(enc, x12, x9, iters):
    """ms per steady-state 12-frame call (the stream is started once with 9 frames, then continued) from device events."""
    _, cache = enc(x9, [None] * 55, stream=False)
    for _ in range(3):
        _, cache = enc(x12, cache, stream=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        mu, cache = enc(x12, cache, stream=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_fresh(enc, x1, iters):
    """ms per fresh one-frame encode; the cache list is dropped after every call, as the session's re-encode does."""
    for _ in range(3):
        enc(x1, [None] * 55, stream=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        enc(x1, [None] * 55, stream=False)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4, help="timed session blocks per mode (after 2 warm-up blocks)")
    ap.add_argument("--encode-only", type=int, default=0, help="run this many steady-state TAEHV encodes and exit")
    ap.add_argument("--no-session", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_taehv_encode.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "taehv_encode_bench needs a GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    from realtime_video_amd import _lib
    from realtime_video_amd.taehv import TAEHVDecoder, TAEHVEncoder, enc_arena_bytes
    from realtime_video_amd.vae_encoder import VAEEncoderWrapper

    g = torch.Generator(device=dev).manual_seed(0)
    x12 = (torch.rand(1, 3, 12, H, W, generator=g, device=dev) * 2 - 1).half()
    x9, x1 = x12[:, :, :9].contiguous(), x12[:, :, :1].contiguous()
    taehv = TAEHVEncoder(dev).init_random_weights(1)
    if args.encode_only:
        print("steady-state ms", time_stream(taehv, x12, x9, args.encode_only))
        return
    wan = VAEEncoderWrapper(device=dev).init_random_weights(seed=2)
    res = {"pixels": [H, W], "frames_per_block": 12, "latent_frames_per_block": 3}
    # alternate the two encoders (shared box: a drift hits both)
    t_taehv, t_wan, f_taehv, f_wan = [], [], [], []
    for _ in range(2):
        t_taehv.append(time_stream(taehv, x12, x9, args.iters))
        t_wan.append(time_stream(wan, x12, x9, args.iters))
        f_taehv.append(time_fresh(taehv, x1, args.iters))
        f_wan.append(time_fresh(wan, x1, args.iters))
    res["taehv_encode12_ms"], res["wan_encode12_ms"] = min(t_taehv), min(t_wan)
    res["taehv_encode12_ms_runs"], res["wan_encode12_ms_runs"] = t_taehv, t_wan
    res["encode12_speedup"] = res["wan_encode12_ms"] / res["taehv_encode12_ms"]
    res["taehv_fresh1_ms"], res["wan_fresh1_ms"] = min(f_taehv), min(f_wan)
    res["taehv_fresh1_ms_runs"], res["wan_fresh1_ms_runs"] = f_taehv, f_wan
    res["fresh1_note"] = "the TAEHV fresh stream presents the frame four times (one full 4-frame group); the Wan encoder runs one frame"
    res["taehv_arena_bytes"] = enc_arena_bytes(H, W, TAEHVEncoder.GROUP)
    res["wan_arena_bytes"] = int(_lib.load().rtv_vae_enc_arena_bytes(H, W))
    flop = 2.0 * 12 * H * W * 27 * 64                                             # first conv
    flop += 2.0 * 6 * (H // 2) * (W // 2) * 18 * 64 * 64                          # TPool(64, 2) + stride-2 conv, folded
    flop += 2.0 * 3 * (H // 4) * (W // 4) * 18 * 64 * 64 + 2.0 * 3 * (H // 8) * (W // 8) * 9 * 64 * 64
    for s, F in enumerate((6, 3, 3)):
        flop += 3 * 2.0 * F * (H >> (s + 1)) * (W >> (s + 1)) * 9 * 64 * 64 * (2 + 1 + 1)    # MemBlocks: conv.0 over 2C, conv.2, conv.4
    flop += 2.0 * 3 * (H // 8) * (W // 8) * 9 * 64 * 16
    res["taehv_tflop_per_block"] = flop / 1e12
    res["taehv_tflops_achieved"] = flop / (res["taehv_encode12_ms"] * 1e-3) / 1e12
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)

    if not args.no_session:
        # ---- 1.3B-shaped webcam session block, use_taehv=True, pixel input on the Wan encoder / on the TAEHV encoder
        from realtime_video_amd.causal_model import CausalWanModel
        from realtime_video_amd.pipeline import CausalInferencePipeline, make_args
        from realtime_video_amd.session import GenerateParams, GenerationSession, Models, StaticTextEncoder
        from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
        model = CausalWanModel(dim=1536, ffn_dim=8960, num_heads=12, num_layers=30, text_dim=4096, freq_dim=256,
                               device=dev).init_random_weights(seed=0)
        wr = WanDiffusionWrapper(model, timestep_shift=5.0)
        dec = TAEHVDecoder(dev).init_random_weights(1)
        prompt = torch.zeros(1, 512, 4096, dtype=torch.bfloat16, device=dev)
        prompt[:, :64] = torch.randn(1, 64, 4096, generator=g, device=dev).to(torch.bfloat16)
        frames = list(x12[0].transpose(0, 1))

        def session_ms(with_taehv_encoder):
            pipe = CausalInferencePipeline(make_args(num_frame_per_block=3, denoising_step_list=[1000, 750, 500, 250]), dev,
                                           generator=wr)
            models = Models(transformer=wr, pipeline=pipe, text_encoder=StaticTextEncoder(prompt), vae_encoder=wan,
                            taehv_decoder=dec, taehv_encoder=taehv if with_taehv_encoder else None)
            params = GenerateParams(prompt="synthetic", seed=42, num_blocks=2 + args.blocks, num_denoising_steps=4,
                                    webcam_mode=True, keep_first_frame=True, strength=0.8)
            sess = GenerationSession(params, models, device=dev, use_taehv=True)

            def block(i):
                for f in frames[:9 if i == 0 else 12]:
                    sess.push_frame(f)
                sess.generate_block()
            for i in range(2):
                block(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.blocks):
                block(2 + i)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.blocks

        runs_wan, runs_taehv = [], []
        for _ in range(2):
            runs_wan.append(session_ms(False))
            runs_taehv.append(session_ms(True))
        res["webcam_block_ms_wan_encoder"], res["webcam_block_ms_taehv_encoder"] = min(runs_wan), min(runs_taehv)
        res["webcam_block_ms_wan_encoder_runs"], res["webcam_block_ms_taehv_encoder_runs"] = runs_wan, runs_taehv
        res["webcam_block_ratio"] = res["webcam_block_ms_taehv_encoder"] / res["webcam_block_ms_wan_encoder"]
        res["session_note"] = ("Wan2.1-T2V-1.3B architecture, random weights, 4 denoising steps, webcam_mode, use_taehv=True (TAEHV "
                               "decode in both), eager; wall clock over the timed blocks ending in a device synchronise")
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
