"""The camera side of the webcam / video-to-video loop on one GPU, in one process: a block of 12 JPEG files from host memory to
rgb8 frames in the upload ring, in two flavours:

  * browser  = 640 x 480, PIL quality 80, 4:2:0, no restart markers: what `canvas.toBlob('image/jpeg')` sends;
  * own      = 832 x 480 files of the native encoder (rtv_jpeg_encode, one restart interval per MCU row).

Per flavour, medians of `--blocks` blocks:
  * jpeg path = frames.FrameUploader.push_jpeg per file (host parse, file bytes over PCIe, rtv_jpeg_decode on the upload stream):
                `kernel_ms_per_frame` (device events around the decode calls alone, files already on the device),
                `rounds` (synchronisation rounds of the entropy kernel, per frame), `push_to_event_ms` (host clock from the first
                push_jpeg to the last slot's event), `host_cpu_ms_per_frame` (process CPU time of the pushes), `pcie_bytes`;
  * pil path  = what this replaces: PIL decode of every file on ONE thread, then FrameUploader.push of the pixels; the same
                figures (no kernel).
The pixels of the two paths are compared (they are equal, tests/test_jpeg_decode_gpu.py).

    python scripts/jpeg_decode_bench.py [--blocks 20] [--out profiles/r11_jpeg_decode.json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T = 12


def camera_frames(H, W, seed):
    """Smooth moving content with mild sensor noise: frames a camera might deliver (fixed seed)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for t in range(T):
        a = np.stack([127 + 100 * np.sin((xx + 7 * t) / 23.0 + yy / 41.0), 127 + 90 * np.cos(xx / 17.0 - (yy + 5 * t) / 29.0),
                      127 + 80 * np.sin((xx + yy + 11 * t) / 37.0)], -1) + rng.normal(0, 4, (H, W, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_jpeg_decode.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_decode_bench needs a GPU"
    dev = "cuda:0"
    torch.cuda.set_device(0)
    from PIL import Image
    from realtime_video_amd import ops
    from realtime_video_amd.frames import FrameUploader

    def pil_decode(f):
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))

    res = {"frames_per_block": T, "blocks": args.blocks, "device": torch.cuda.get_device_name(0),
           "note": "medians over blocks; the pil path decodes on one thread"}
    flavours = {}
    imgs = camera_frames(480, 640, 0)
    files = []
    for im in imgs:
        b = io.BytesIO()
        Image.fromarray(im).save(b, format="JPEG", quality=80, subsampling=2)
        files.append(b.getvalue())
    flavours["browser_640x480_q80_420"] = files
    rgb = torch.from_numpy(np.stack(camera_frames(480, 832, 1))).to(dev)
    buf, offs = ops.jpeg_encode(rgb, 90)
    buf, offs = buf.cpu().numpy().tobytes(), offs.tolist()
    flavours["own_832x480_q90"] = [buf[offs[t]:offs[t + 1]] for t in range(T)]

    for name, files in flavours.items():
        infos = [ops.jpeg_parse(f) for f in files]
        H, W = infos[0].H, infos[0].W
        # kernel time and rounds: the decode call alone, files resident
        frames = [torch.frombuffer(bytearray(i.packed() + f), dtype=torch.uint8).to(dev) for i, f in zip(infos, files)]
        outs = [torch.empty((H, W, 3), dtype=torch.uint8, device=dev) for _ in files]
        status = torch.zeros(T, dtype=torch.int32, device=dev)
        rounds = torch.zeros(T, dtype=torch.int32, device=dev)
        arena = torch.empty(ops.jpeg_decode_arena_bytes(infos), dtype=torch.uint8, device=dev)
        kernel_ms = []
        for it in range(args.blocks + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.jpeg_decode_frames(infos, frames, outs, status, arena, rounds=rounds)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                kernel_ms.append(e0.elapsed_time(e1) / T)
        assert status.tolist() == [0] * T
        equal = all(np.array_equal(o.cpu().numpy(), pil_decode(f)) for o, f in zip(outs, files))

        def block(push_all):
            up.stream.synchronize()
            c0, t0 = time.process_time(), time.perf_counter()
            tickets = push_all()
            c1 = time.process_time()
            up._done[tickets[-1] % up.slots].synchronize()
            return 1e3 * (time.perf_counter() - t0), 1e3 * (c1 - c0) / T

        r = {"size": [H, W], "file_bytes_per_block": sum(len(f) for f in files), "pixels_equal_pil": equal,
             "kernel_ms_per_frame": statistics.median(kernel_ms), "rounds_per_frame": rounds.tolist()}
        for path, push_all in (("jpeg", lambda: [up.push_jpeg(f) for f in files]), ("pil", lambda: [up.push(pil_decode(f)) for f in files])):
            up = FrameUploader(dev, slots=2 * T)
            runs = [block(push_all) for _ in range(args.blocks + 3)][3:]
            r[f"{path}_push_to_event_ms"] = statistics.median(x[0] for x in runs)
            r[f"{path}_host_cpu_ms_per_frame"] = statistics.median(x[1] for x in runs)
        r["jpeg_pcie_bytes"] = sum(len(f) + ops.JPEG_DESC_BYTES for f in files)
        r["pil_pcie_bytes"] = T * H * W * 3
        res[name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
