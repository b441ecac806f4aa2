"""Mint the TAEHV decoder golden from the upstream reference module (demo_utils/taehv.py).

Run where the reference checkout exists (like oracle/make_golden.py):   python scripts/make_taehv_golden.py [REFERENCE_ROOT]
Writes tests/golden/taehv_decoder.pt (seed, weights checksum, the 8x12 output), tests/golden/taehv_decoder_7x11.pt (the
ragged-grid output; two files so that each stays under the 1 MiB limit of a committed file) and tests/golden/taehv_manifest.json.
The reference TAEHV is built without a checkpoint, loaded with TAEHVDecoder.random_state_dict(SEED) (weights are regenerated
by the tests, only their checksum is stored) and run with decode_video(parallel=True) in float32 on CPU; the sequential form (parallel=False) must agree.  Latents are
regenerated from LATENT_SEED by the tests; the stored outputs are the reference's frames 3 .. 4T-1 (the 3 warm-up frames
trimmed), fp16.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from realtime_video_amd.taehv import TAEHVDecoder  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED = 7
LATENT_SEED = 11
T = 6
SIZES = ((7, 11), (8, 12))   # a ragged grid (no dimension a multiple of 4) and an even one


def latents(h, w, seed=LATENT_SEED):
    g = torch.Generator().manual_seed(seed + 1000 * h + w)
    return torch.randn(1, T, 16, h, w, generator=g)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TAEHV_REFERENCE_ROOT", "/root/reference")
    sys.path.insert(0, ref_root)
    from demo_utils.taehv import TAEHV

    torch.manual_seed(0)
    model = TAEHV(checkpoint_path=None).float().eval()
    dec_sd = {k: v for k, v in model.state_dict().items() if k.startswith("decoder.")}
    spec = TAEHVDecoder.state_dict_spec()
    assert [(k, tuple(v.shape)) for k, v in dec_sd.items()] == spec, "state_dict_spec differs from the reference module"
    sd = TAEHVDecoder.random_state_dict(SEED)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("encoder.") for k in missing)

    out = {"seed": SEED, "latent_seed": LATENT_SEED, "T": T, "checksum": TAEHVDecoder.checksum(sd), "outputs": {}}
    with torch.no_grad():
        for h, w in SIZES:
            z = latents(h, w)
            y = model.decode_video(z, parallel=True)
            y_seq = model.decode_video(z, parallel=False)
            assert y.shape == (1, 4 * T, 3, 8 * h, 8 * w), y.shape
            rel = float((y - y_seq).norm() / y.norm())
            assert rel < 1e-5, f"parallel / sequential decode disagree: rel-L2 {rel}"
            y3 = y[:, 3:]
            std = float(y3.std())
            print(f"{h}x{w}: range [{float(y3.min()):.4f}, {float(y3.max()):.4f}] mean {float(y3.mean()):.4f} std {std:.4f} "
                  f"parallel/sequential rel-L2 {rel:.2e}")
            assert std > 1e-2, "output is dead"
            assert 0.0 < float(y3.min()) and float(y3.max()) < 1.0, "output leaves (0, 1): saturates TAEHV's range"
            out["outputs"][f"{h}x{w}"] = y3.to(torch.float16).contiguous()
    ragged = {k: v for k, v in out.items() if k != "outputs"}
    ragged["outputs"] = {"7x11": out["outputs"].pop("7x11")}
    torch.save(out, os.path.join(OUT, "taehv_decoder.pt"))
    torch.save(ragged, os.path.join(OUT, "taehv_decoder_7x11.pt"))
    manifest = {"decoder": [[k, list(v.shape)] for k, v in dec_sd.items()],
                "encoder_keys": sorted(k for k in model.state_dict() if k.startswith("encoder."))}
    with open(os.path.join(OUT, "taehv_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote taehv_decoder.pt, taehv_decoder_7x11.pt, taehv_manifest.json under", OUT)


if __name__ == "__main__":
    main()
