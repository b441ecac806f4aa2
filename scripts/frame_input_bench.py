"""The input side of the webcam / video-to-video loop on one GPU, in one process: a block of 12 camera frames from host memory
to the tensor handed to the VAE encoder (float16 [3, 12, 480, 832] in [-1, 1]), for 1280 x 720 and 640 x 480 cameras (bicubic
resize) and for 832 x 480 (decode only).

  * torch path  = what the reference does and this package did before the native path: per frame a pinned float16 [3, Hin, Win]
                  tensor (the CPU's to_tensor / half is NOT timed) uploaded and mapped with sub_(0.5).mul_(2.0)
                  (release_server.py:479-481), then the front of encode_video_latent (stack, F.interpolate(float32, bicubic) at
                  another size, transpose, float16, the encoder's contiguous());
  * native path = frames.FrameUploader.push per uint8 [Hin, Win, 3] frame (1 byte per sample over PCIe) and one gather
                  (rtv_frames_from_rgb8).

Per size and path: `block_ms`, device events on the compute stream around upload + front (the native gather waits for the upload
stream's copies), `front_ms`, the same with the frames already on the device (the passes that sit in front of every block's
encode on the compute stream), and `wall_ms`, the host clock around the block ending in a device synchronise.  The two paths
alternate; the minimum of the rounds is reported next to all rounds.

    python scripts/frame_input_bench.py [--iters 20] [--rounds 3] [--out profiles/r09_frame_input.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, T = 480, 832, 12


def torch_front(frames):
    """encode_video_latent up to the encoder's input (vae_encoder.py: resize, transpose, cast; the wrapper's contiguous())."""
    if tuple(frames.shape[2:]) != (H, W):
        frames = torch.nn.functional.interpolate(frames.float(), size=(H, W), mode="bicubic")
    return frames.transpose(0, 1).to(torch.float16).contiguous()


def timed(fn, iters, warmup=3):
    """(ms per call from device events on the current stream, ms per call from the host clock ending in a synchronise)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, 1e3 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_frame_input.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "frame_input_bench needs a GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    from realtime_video_amd import ops
    from realtime_video_amd.frames import FrameUploader

    res = {"frames_per_block": T, "output": [3, T, H, W], "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "note": "ms per 12-frame block; min over alternating rounds; the torch path's CPU-side to_tensor / half is not timed"}
    g = torch.Generator().manual_seed(0)
    for name, (hin, win) in (("1280x720", (720, 1280)), ("640x480", (480, 640)), ("832x480", (480, 832))):
        u8 = torch.randint(0, 256, (T, hin, win, 3), generator=g, dtype=torch.uint8).pin_memory()
        f16 = (u8.permute(0, 3, 1, 2).float() / 255).half().pin_memory()          # TF.to_tensor(image).to(float16).pin_memory()
        up = FrameUploader(dev, slots=2 * T)
        u8_dev = u8.to(dev)
        f16_dev = [f.to(dev).sub_(0.5).mul_(2.0) for f in f16]

        def torch_block():
            return torch_front(torch.stack([f.to(dev, non_blocking=True).sub_(0.5).mul_(2.0) for f in f16]))

        def native_block():
            return up.gather([up.push(f) for f in u8], (H, W))

        def torch_resident():
            return torch_front(torch.stack(f16_dev))

        def native_resident():
            return ops.frames_from_rgb8(u8_dev, (H, W))

        a, b = torch_block(), native_block()
        differ = (a != b).float().mean().item()                                    # same inputs: what the two paths disagree on
        max_abs = (a.float() - b.float()).abs().max().item()
        runs = {k: [] for k in ("torch_block", "native_block", "torch_front", "native_front")}
        for _ in range(args.rounds):
            runs["torch_block"].append(timed(torch_block, args.iters))
            runs["native_block"].append(timed(native_block, args.iters))
            runs["torch_front"].append(timed(torch_resident, args.iters))
            runs["native_front"].append(timed(native_resident, args.iters))
        r = {"input": [hin, win], "elements_differing": differ, "max_abs_difference": max_abs,
             "upload_bytes_torch": T * hin * win * 3 * 2, "upload_bytes_native": T * hin * win * 3}
        for path in ("torch", "native"):
            r[f"{path}_block_ms"] = min(x[0] for x in runs[f"{path}_block"])
            r[f"{path}_wall_ms"] = min(x[1] for x in runs[f"{path}_block"])
            r[f"{path}_front_ms"] = min(x[0] for x in runs[f"{path}_front"])
            r[f"{path}_block_ms_runs"] = [x[0] for x in runs[f"{path}_block"]]
            r[f"{path}_wall_ms_runs"] = [x[1] for x in runs[f"{path}_block"]]
            r[f"{path}_front_ms_runs"] = [x[0] for x in runs[f"{path}_front"]]
        # the native launch moves 3 B per source pixel in and 6 B per output pixel out
        r["native_front_bytes"] = T * (hin * win * 3 + H * W * 6)
        r["native_front_gbps"] = r["native_front_bytes"] / (r["native_front_ms"] * 1e-3) / 1e9
        res[name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
