"""LoRA adapters for the native DiT.  The model has no nn.Module tree - every Linear is a raw bf16 buffer behind the ctypes
weight table, self-attention q / k / v fused into one [3d, d] matrix - so an adapter is MERGED into the weights in place
(rtv_lora_merge, include/rtv_hip_lora.h): weight pointers do not move and captured hipGraphs stay valid.

This module holds the host side: `parse_lora_state_dict` maps a LoRA state dict (the key styles Wan 2.1 LoRAs are published with)
onto the model's matrices, `merge` is the kernel call.  CausalWanModel.load_lora / set_lora_scale / unload_lora
(causal_model.py) keep the base copies and re-merge.  There is no CPU fallback: a model on the CPU parses and refuses to merge."""
import collections
import ctypes
import math
import re

import torch

from . import _lib

MAX_ADAPTERS, MAX_RANK = _lib.LORA_MAX_ADAPTERS, _lib.LORA_MAX_RANK
_Adapter = _lib.LORA_STRUCTS["rtv_lora_adapter"]

_PREFIXES = ("model.diffusion_model.", "diffusion_model.", "model.")
_TARGET = re.compile(r"blocks\.(\d+)\.(?:(self_attn|cross_attn)\.([qkvo])|ffn\.([02]))")
_SUFFIXES = {".lora_A.weight": "A", ".lora_down.weight": "A", ".lora_B.weight": "B", ".lora_up.weight": "B", ".alpha": "alpha"}

# One Linear an adapter changes: `tensor` is the model's matrix (a key of CausalWanModel._tensors), rows [row0, row0 + rows) of
# it are this Linear's weight [rows, cols]; A [rank, cols] ("down") and B [rows, rank] ("up") are the adapter's tensors as given,
# `factor` is alpha / rank (1.0 without alpha): the merge adds scale * factor * B @ A.
Target = collections.namedtuple("Target", ["tensor", "row0", "rows", "cols", "rank", "factor", "A", "B"])


def _strip(key):
    for p in _PREFIXES:
        if key.startswith(p):
            return key[len(p):]
    return key


def parse_lora_state_dict(sd, model_shapes, strict=True):
    """LoRA state dict -> ({target name: Target}, unexpected keys).  `model_shapes` is CausalWanModel.state_dict_shapes().
    Accepted keys: an optional prefix (`diffusion_model.`, `model.diffusion_model.`, `model.`), a target
    (`blocks.N.{self_attn,cross_attn}.{q,k,v,o}`, `blocks.N.ffn.0`, `blocks.N.ffn.2`) and a suffix (`.lora_A.weight` /
    `.lora_B.weight`, `.lora_down.weight` / `.lora_up.weight`, or the optional scalar `.alpha`).  A half-pair, a shape that does
    not fit the model (A [r, in], B [out, r]) or a rank above MAX_RANK raises a ValueError that names the key.  Any other key
    (`.diff`, `.diff_b`, norms, embeddings, the head, flattened `lora_unet_...` names) raises under strict=True and is
    returned as unexpected under strict=False."""
    found, unexpected = {}, []
    for key in sd:
        name = _strip(key)
        part = next((s for s in _SUFFIXES if name.endswith(s)), None)
        target = name[:-len(part)] if part else None
        if part is None or not _TARGET.fullmatch(target) or target + ".weight" not in model_shapes:
            unexpected.append(key)
            continue
        slot = found.setdefault(target, {})
        if _SUFFIXES[part] in slot:
            raise ValueError(f"LoRA key {key!r} repeats {slot[_SUFFIXES[part]][0]!r}")
        slot[_SUFFIXES[part]] = (key, sd[key])
    if unexpected and strict:
        raise ValueError("unexpected key(s) in LoRA state dict (only lora_A / lora_B, lora_down / lora_up and alpha of the attention "
                         "and ffn Linears are merged): " + ", ".join(repr(k) for k in sorted(unexpected)[:12])
                         + (f" ... ({len(unexpected)} in total)" if len(unexpected) > 12 else ""))
    targets = {}
    for target, slot in sorted(found.items()):
        for have, lack in (("A", "B"), ("B", "A"), ("alpha", "A")):
            if have in slot and lack not in slot:
                raise ValueError(f"LoRA key {slot[have][0]!r} has no lora_{lack} / lora_{'up' if lack == 'B' else 'down'} partner")
        (ka, A), (kb, B) = slot["A"], slot["B"]
        out_f, in_f = model_shapes[target + ".weight"]
        if A.ndim != 2 or A.shape[1] != in_f:
            raise ValueError(f"LoRA key {ka!r}: shape {tuple(A.shape)} does not fit, {target} wants A [rank, {in_f}]")
        rank = int(A.shape[0])
        if rank < 1 or rank > MAX_RANK:
            raise ValueError(f"LoRA key {ka!r}: rank {rank} outside 1 .. {MAX_RANK}")
        if tuple(B.shape) != (out_f, rank):
            raise ValueError(f"LoRA key {kb!r}: shape {tuple(B.shape)} does not fit, {target} wants B [{out_f}, {rank}]")
        factor = 1.0
        if "alpha" in slot:
            kal, alpha = slot["alpha"]
            if torch.is_tensor(alpha) and alpha.numel() != 1:
                raise ValueError(f"LoRA key {kal!r}: alpha must be a scalar, not shape {tuple(alpha.shape)}")
            factor = float(alpha) / rank
            if not math.isfinite(factor):
                raise ValueError(f"LoRA key {kal!r}: alpha is not finite")
        m = _TARGET.fullmatch(target)
        layer, attn, proj, ffn = int(m.group(1)), m.group(2), m.group(3), m.group(4)
        row0 = 0
        if ffn is not None:
            field = f"ffn{ffn}_w"
        elif attn == "cross_attn":
            field = f"c{proj}_w"
        elif proj == "o":
            field = "o_w"
        else:                       # self-attention q / k / v: row blocks of the fused [3d, d] matrix
            field, row0 = "qkv_w", "qkv".index(proj) * out_f
        targets[target] = Target(f"L{layer}.{field}", row0, out_f, in_f, rank, factor, A, B)
    return targets, sorted(unexpected)


def merge(base, out, adapters, stream=None):
    """out = bf16(base + sum scale * B @ A) over one matrix or row range (rtv_lora_merge): `base` / `out` are bf16 [N, K] views
    with unit column stride (the same view for an in-place merge), `adapters` a list of (A [r, K], B [N, r], scale) with dense
    bf16 device tensors.  One launch on the current stream."""
    if not (base.is_cuda and out.is_cuda):
        raise RuntimeError("the LoRA merge is a HIP kernel: it needs GPU tensors (no CPU fallback)")
    for t in (base, out):
        if t.dtype != torch.bfloat16 or t.ndim != 2 or t.stride(1) != 1:
            raise ValueError("lora merge: base / out must be bf16 [N, K] with unit column stride")
    if base.shape != out.shape:
        raise ValueError("lora merge: base and out differ in shape")
    N, K = base.shape
    table = (_Adapter * max(1, len(adapters)))()
    for i, (A, B, scale) in enumerate(adapters):
        for t, shape in ((A, (A.shape[0], K)), (B, (N, A.shape[0]))):
            if t.dtype != torch.bfloat16 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError("lora merge: A [r, K] / B [N, r] must be dense bf16 device tensors")
        table[i] = _Adapter(A.data_ptr(), B.data_ptr(), int(A.shape[0]), float(scale))
    if stream is None:
        stream = torch.cuda.current_stream(base.device).cuda_stream
    with torch.cuda.device(base.device):
        _lib.call("rtv_lora_merge", base.data_ptr(), base.stride(0), out.data_ptr(), out.stride(0), N, K,
                  table if adapters else None, len(adapters), ctypes.c_void_p(stream))
    return out
