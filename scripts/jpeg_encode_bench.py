#!/usr/bin/env python
"""Frame delivery of one 12-frame 480 x 832 block, two ways, on decoder-like pixels:

  (a) the path without the JPEG kernels: frames.FrameDownloader (rgb8 on the device, 3 bytes per pixel over PCIe) and
      PIL.Image.fromarray(frame).save(format='JPEG', quality=90) per frame on a 16-thread pool (release_server.py:970-1007 runs
      the same encode on 24 threads);
  (b) frames.JpegFrameDownloader: rtv_jpeg_encode on the device, only the files cross.

Per block (medians over --blocks blocks after --warmup): GPU time of the three kernels of rtv_jpeg_encode (device events around the
call), device-to-host bytes, wall time from the call to the last frame's bytes, and CPU seconds of the process (all threads).
Needs a GPU; writes one JSON document (default profiles/r10_jpeg_encode.json).

    python scripts/jpeg_encode_bench.py [--blocks 20] [--warmup 3] [--out FILE]"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realtime_video_amd import ops  # noqa: E402
from realtime_video_amd.frames import FrameDownloader, JpegFrameDownloader  # noqa: E402

T, H, W, QUALITY, THREADS = 12, 480, 832, 90, 16


def decoder_like_pixels(seed):
    """float32 [1, T, 3, H, W] in about [-1, 1]: smooth structure at several scales that drifts over the frames, plus fine noise."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(T, 3, H, W)
    for size, gain in ((4, 0.5), (15, 0.3), (60, 0.15)):
        low = torch.randn(1, 3, size, size * 2, generator=g).repeat(T, 1, 1, 1) + 0.2 * torch.randn(T, 3, size, size * 2, generator=g)
        x += gain * torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    return (x + 0.03 * torch.randn(x.shape, generator=g)).clamp(-1.1, 1.1)[None].contiguous()


def pil_encode(frame):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(frame).save(b, format="JPEG", quality=QUALITY)
    return b.getvalue()


def measure(run, blocks, warmup):
    wall, cpu, extra = [], [], []
    for i in range(warmup + blocks):
        torch.cuda.synchronize()
        c0, t0 = time.process_time(), time.perf_counter()
        out = run()
        t1, c1 = time.perf_counter(), time.process_time()
        if i >= warmup:
            wall.append((t1 - t0) * 1e3)
            cpu.append(c1 - c0)
            extra.append(out)
    return statistics.median(wall), statistics.median(cpu), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r10_jpeg_encode.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("jpeg_encode_bench needs a GPU: nothing here can be measured without one")
    dev = "cuda"
    pixels = decoder_like_pixels(0).to(dev)

    # (a) rgb8 download + PIL on a thread pool
    down, pool = FrameDownloader(dev), ThreadPoolExecutor(THREADS)

    def run_a():
        frames = down.fetch(down(pixels)).numpy()
        return sum(len(f) for f in pool.map(pil_encode, frames))
    a_wall, a_cpu, a_bytes = measure(run_a, args.blocks, args.warmup)

    # (b) encode on the device
    jdown = JpegFrameDownloader(dev, quality=QUALITY)

    def run_b():
        before = jdown.topups
        files = jdown.fetch(jdown(pixels))
        return sum(len(f) for f in files), jdown._copied[(jdown._n - 1) % jdown.slots], jdown.topups - before
    b_wall, b_cpu, b_extra = measure(run_b, args.blocks, args.warmup)

    # the three kernels alone, device events around rtv_jpeg_encode
    src = pixels[0].contiguous()
    out = torch.empty(ops.jpeg_out_bound(T, H, W), dtype=torch.uint8, device=dev)
    offs = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    arena = torch.empty(ops.jpeg_arena_bytes(T, H, W), dtype=torch.uint8, device=dev)
    gpu_ms = []
    for i in range(args.warmup + args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.jpeg_encode(src, QUALITY, out=out, offsets=offs, arena=arena)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            gpu_ms.append(e0.elapsed_time(e1))

    result = {
        "workload": f"{T} frames {H}x{W}, quality {QUALITY}, decoder-like pixels (seed 0)", "blocks": args.blocks, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "a_rgb8_download_plus_pil_pool": {"threads": THREADS, "wall_ms_per_block": round(a_wall, 3), "cpu_s_per_block": round(a_cpu, 4),
                                          "d2h_bytes_per_block": T * H * W * 3, "jpeg_bytes_per_block": a_bytes[-1]},
        "b_jpeg_frame_downloader": {"wall_ms_per_block": round(b_wall, 3), "cpu_s_per_block": round(b_cpu, 4),
                                    "d2h_bytes_per_block": b_extra[-1][1] + 8 * (T + 1), "jpeg_bytes_per_block": b_extra[-1][0],
                                    "topups_in_timed_blocks": sum(e[2] for e in b_extra),
                                    "gpu_ms_three_kernels": round(statistics.median(gpu_ms), 4),
                                    "gpu_ms_three_kernels_min_max": [round(min(gpu_ms), 4), round(max(gpu_ms), 4)]},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
