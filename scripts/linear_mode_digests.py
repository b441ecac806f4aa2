"""Digests of everything a DiT Linear precision mode prepares and computes, for comparing two revisions of the weight-preparation
and dispatch code bit for bit: run it on each revision and diff the two files (only the "commit" line may differ).  It uses the
public calls (enable_fp8 / enable_mxfp4 / enable_mxfp6 / set_linear_precision / linear_precision, load_lora / set_lora_scale) and
the attributes the tests read (_tensors, _fp8_scales, _fp8_row_scales, _mx_scales, _cfg), nothing else.

On the tiny model of tests/mx_cases.py, for bf16 (fold_cross_v off), the six pure modes and the MIXED policy of
tests/test_precision_policy_gpu.py:

  outputs       SHA-256 of each of the three forwards of mx_cases.three_forwards (denoise, recompute, denoise)
  weights       SHA-256 over every Linear's weight bytes and the scale bytes of its mode, in the order of rtv_dit_weights.fp8_scales
  dispatch      ops.dispatch_counts() of one first forward
  workspace     rtv_dit_workspace_bytes at dim 1536, ffn 8960, 12 heads, 2 layers, F, gh, gw = 3, 30, 52
  lora_weights  `weights` again after: the rank-4 adapter of tests/test_lora_gpu.py's _lora_sd loaded at strength 0.7 before the
                mode is enabled, set_lora_scale(0.25) afterwards

    python scripts/linear_mode_digests.py --commit $(git rev-parse --short HEAD) --out profiles/r22_linear_modes_head.json"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mx_cases                                                      # noqa: E402
from realtime_video_amd import _lib, ops, precision_policy            # noqa: E402

MIXED = {"default": "fp8_row", "ffn0": "mxfp4", "ffn2": "mxfp4", "head": "bf16", "L0.qkv": "mxfp6"}      # tests/test_precision_policy_gpu.py


def _bf16(m):
    m.fold_cross_v = False


SETUPS = {"bf16": _bf16, "fp8": lambda m: m.enable_fp8(), "fp8_row": lambda m: m.enable_fp8("row"), "mxfp4": lambda m: m.enable_mxfp4(),
          "mxfp6": lambda m: m.enable_mxfp6(), "mxfp4_rot": lambda m: m.enable_mxfp4(rotate=True),
          "mxfp6_rot": lambda m: m.enable_mxfp6(rotate=True), "mixed": lambda m: m.set_linear_precision(MIXED)}
T = torch.ones([1, 3], dtype=torch.int64) * 700
T0 = torch.zeros([1, 3], dtype=torch.int64)


def sha(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c)
    return h.hexdigest()


def tensor_bytes(t):
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()


def weights_digest(model):
    """Every Linear in table order: its weight as held, then the scales its mode keeps (per tensor, per row, or per block)."""
    torch.cuda.synchronize()
    chunks = []
    for i, (name, mode) in enumerate(model.linear_precision().items()):
        key = name + "_w"
        chunks.append(tensor_bytes(model._tensors[key]))
        if mode == "fp8":
            chunks.append(struct.pack("<f", model._fp8_scales[i]))
        elif mode == "fp8_row":
            chunks.append(tensor_bytes(model._fp8_row_scales[key]))
        elif mode != "bf16":
            chunks.append(tensor_bytes(model._mx_scales[key]))
    return sha(*chunks)


def one_setup(setup, weights, lat, ctx, lora_sd):
    model, wr = mx_cases.build(weights)
    setup(model)
    res = {"use_fp8": int(model._cfg.use_fp8), "weights": weights_digest(model)}
    kv, ca = mx_cases.caches()
    ops.dispatch_counts(reset=True)
    wr(lat[0].to(mx_cases.DEV), {"prompt_embeds": [ctx.to(mx_cases.DEV)]}, T.to(mx_cases.DEV), kv, ca, current_start=0)
    torch.cuda.synchronize()
    res["dispatch"] = ops.dispatch_counts()
    res["outputs"] = [sha(tensor_bytes(o)) for o in mx_cases.three_forwards(model, wr, lat, ctx, T, T0)]
    cfg = _lib.STRUCTS["rtv_dit_config"](dim=1536, ffn_dim=8960, num_heads=12, num_layers=2, freq_dim=256, text_dim=4096, text_len=512,
                                         in_dim=16, out_dim=16, eps=1e-6, use_fp8=int(model._cfg.use_fp8), max_attn_kv_splits=0)
    res["workspace"] = int(_lib.load().rtv_dit_workspace_bytes(ctypes.byref(cfg), 3, 30, 52))
    model, _ = mx_cases.build(weights)
    model.load_lora(lora_sd, scale=0.7, name="style")
    setup(model)
    model.set_lora_scale("style", 0.25)
    res["lora_weights"] = weights_digest(model)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default="unknown", help="recorded in the output; the one field that differs between two revisions")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the digests are of GPU results: this needs the GPU"
    from oracle import wan_oracle as wo
    from test_lora_gpu import _lora_sd
    weights = wo.make_weights(mx_cases.CFG, seed=0, text_dim=mx_cases.TEXT_DIM)
    lat, ctx = mx_cases.inputs()
    lora_sd = _lora_sd(weights, rank=4)
    res = {"commit": args.commit, "model": dict(mx_cases.CFG, text_dim=mx_cases.TEXT_DIM), "linears": precision_policy.linear_names(2),
           "setups": {name: one_setup(setup, weights, lat, ctx, lora_sd) for name, setup in SETUPS.items()}}
    text = json.dumps(res, indent=1, sort_keys=True) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
