"""Mint the TAEHV encoder golden from the upstream reference module (demo_utils/taehv.py).

Run where the reference checkout exists (like scripts/make_taehv_golden.py):   python scripts/make_taehv_encoder_golden.py REFERENCE_ROOT
Writes tests/golden/taehv_encoder.pt (seed, frame seed, weights checksum, the float32 latents of three cases) and
tests/golden/taehv_encoder_manifest.json (the reference module's encoder key names and shapes).
The reference TAEHV is built without a checkpoint, loaded with TAEHVEncoder.random_state_dict(SEED) (weights are regenerated
by the tests, only their checksum is stored) and run with encode_video(parallel=True) in float32 on CPU; the sequential form
(parallel=False) must agree.  Frames are regenerated from FRAME_SEED by the tests (torch.rand in [0, 1]; the wrapper takes
2 * x - 1).  Cases whose name ends in "_fresh" follow TAEHVEncoder's fresh-stream contract: frame 0 is presented to the
reference four times.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realtime_video_amd.taehv import TAEHVEncoder  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 7
FRAME_SEED = 13
# name -> (H, W, frames handed to the wrapper, fresh-stream contract)
CASES = {"64x96_12": (64, 96, 12, False), "56x88_9_fresh": (56, 88, 9, True), "56x88_21_fresh": (56, 88, 21, True)}


def frames01(H, W, T, seed=FRAME_SEED):
    """[T, 3, H, W] in [0, 1]; a prefix of a longer clip of the same size is the same frames."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    return torch.rand(24, 3, H, W, generator=g)[:T]


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TAEHV_REFERENCE_ROOT")
    if not ref_root:
        sys.exit("usage: make_taehv_encoder_golden.py REFERENCE_ROOT (or set TAEHV_REFERENCE_ROOT)")
    sys.path.insert(0, ref_root)
    from demo_utils.taehv import TAEHV

    torch.manual_seed(0)
    model = TAEHV(checkpoint_path=None).float().eval()
    enc_sd = {k: v for k, v in model.state_dict().items() if k.startswith("encoder.")}
    spec = TAEHVEncoder.state_dict_spec()
    assert [(k, tuple(v.shape)) for k, v in enc_sd.items()] == spec, "state_dict_spec differs from the reference module"
    sd = TAEHVEncoder.random_state_dict(SEED)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("decoder.") for k in missing)

    out = {"seed": SEED, "frame_seed": FRAME_SEED, "checksum": TAEHVEncoder.checksum(sd), "cases": {k: list(v) for k, v in CASES.items()},
           "latents": {}}
    with torch.no_grad():
        for name, (H, W, T, fresh) in CASES.items():
            x = frames01(H, W, T)
            if fresh:
                x = torch.cat([x[:1].expand(3, -1, -1, -1), x])
            x = x[None]
            y = model.encode_video(x, parallel=True, show_progress_bar=False)
            y_seq = model.encode_video(x, parallel=False, show_progress_bar=False)
            assert y.shape == (1, x.shape[1] // 4, 16, H // 8, W // 8), y.shape
            rel = float((y - y_seq).norm() / y.norm())
            assert rel < 1e-5, f"parallel / sequential encode disagree: rel-L2 {rel}"
            std = float(y.std())
            print(f"{name}: {tuple(y.shape)} mean {float(y.mean()):.4f} std {std:.4f} max-abs {float(y.abs().max()):.4f} "
                  f"parallel/sequential rel-L2 {rel:.2e}")
            assert std > 1e-2, "output is dead"
            out["latents"][name] = y[0].float().contiguous()     # [T', 16, h, w]
    torch.save(out, os.path.join(OUT, "taehv_encoder.pt"))
    with open(os.path.join(OUT, "taehv_encoder_manifest.json"), "w") as f:
        json.dump({"encoder": [[k, list(v.shape)] for k, v in enc_sd.items()]}, f, indent=1)
    print("wrote taehv_encoder.pt, taehv_encoder_manifest.json under", OUT)


if __name__ == "__main__":
    main()
