"""LoRA adapters for the native DiT.  The model has no nn.Module tree - every Linear is a raw bf16 buffer behind the ctypes
weight table, self-attention q / k / v fused into one [3d, d] matrix - so an adapter is MERGED into the weights in place
(rtv_lora_merge, include/rtv_hip_lora.h): weight pointers do not move and captured hipGraphs stay valid.

This module holds the host side: `parse_lora_state_dict` maps a LoRA state dict (the key styles Wan 2.1 LoRAs are published with)
onto the model's matrices, `merge` is the kernel call.  extended=True (opt-in) adds the kohya and diffusers key styles, every Linear
of the model, `.diff` / `.diff_b` deltas and DoRA magnitude vectors; `merge_ex` / `merge_dora` are the kernel calls of those forms
(include/rtv_hip_lora_ext.h).  CausalWanModel.load_lora / set_lora_scale / unload_lora
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
# extended=True adds, all None by default: `diff` (a dense delta of the weight rows, [rows, cols]; on a norm the target is the
# weight vector itself, rows == 1 and diff [cols]), `diff_b` (a delta of elements [bias0, bias0 + bias_n) of the vector `bias`) and
# `dora` (the DoRA magnitude vector [rows]; the merge is then the row-normalised one, not additive).  rank == 0 and A / B None: a
# target without a low-rank pair.
Target = collections.namedtuple("Target", ["tensor", "row0", "rows", "cols", "rank", "factor", "A", "B", "diff", "diff_b", "bias",
                                           "bias0", "bias_n", "dora"], defaults=(None, None, None, 0, 0, None))


def _strip(key):
    for p in _PREFIXES:
        if key.startswith(p):
            return key[len(p):]
    return key


def parse_lora_state_dict(sd, model_shapes, strict=True, extended=False):
    """LoRA state dict -> ({target name: Target}, unexpected keys).  `model_shapes` is CausalWanModel.state_dict_shapes().
    Accepted keys: an optional prefix (`diffusion_model.`, `model.diffusion_model.`, `model.`), a target
    (`blocks.N.{self_attn,cross_attn}.{q,k,v,o}`, `blocks.N.ffn.0`, `blocks.N.ffn.2`) and a suffix (`.lora_A.weight` /
    `.lora_B.weight`, `.lora_down.weight` / `.lora_up.weight`, or the optional scalar `.alpha`).  A half-pair, a shape that does
    not fit the model (A [r, in], B [out, r]) or a rank above MAX_RANK raises a ValueError that names the key.  Any other key
    (`.diff`, `.diff_b`, norms, embeddings, the head, flattened `lora_unet_...` names) raises under strict=True and is
    returned as unexpected under strict=False.

    extended=True lifts most of that list (everything above stays as it is with extended=False): see _parse_extended."""
    if extended:
        return _parse_extended(sd, model_shapes, strict)
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


# ------------------------------------------------------------------ extended=True: more key styles, more targets, more terms
_EXT_PREFIXES = ("model.diffusion_model.", "diffusion_model.", "transformer.", "model.")
_EXT_SUFFIXES = {**_SUFFIXES, ".diff": "diff", ".diff_b": "diff_b", ".dora_scale": "dora", ".lora_magnitude_vector": "dora",
                 ".lora_magnitude_vector.weight": "dora"}
# The renames of the diffusers Wan conversion, (diffusers, canonical), on whole dotted components: inside `blocks.N.` and at the
# top level.  Restated from the trainers' conventions; no published adapter file was at hand.
_DIFFUSERS_BLOCK = (("attn1", "self_attn"), ("attn2", "cross_attn"), ("to_q", "q"), ("to_k", "k"), ("to_v", "v"), ("to_out.0", "o"),
                    ("ffn.net.0.proj", "ffn.0"), ("ffn.net.2", "ffn.2"), ("norm2", "norm3"))
_DIFFUSERS_TOP = (("condition_embedder.text_embedder.linear_1", "text_embedding.0"),
                  ("condition_embedder.text_embedder.linear_2", "text_embedding.2"),
                  ("condition_embedder.time_embedder.linear_1", "time_embedding.0"),
                  ("condition_embedder.time_embedder.linear_2", "time_embedding.2"),
                  ("condition_embedder.time_proj", "time_projection.1"), ("proj_out", "head.head"))
_TOP_TENSORS = {"text_embedding.0": "text0", "text_embedding.2": "text2", "time_embedding.0": "time0", "time_embedding.2": "time2",
                "time_projection.1": "tproj", "head.head": "head"}
_NORM_TENSORS = {"self_attn.norm_q": "norm_q_w", "self_attn.norm_k": "norm_k_w", "cross_attn.norm_q": "cnorm_q_w",
                 "cross_attn.norm_k": "cnorm_k_w", "norm3": "norm3_w"}
_BLOCK = re.compile(r"blocks\.(\d+)\.(.+)")


def diffusers_name(target):
    """The diffusers spelling of a canonical target (`blocks.0.self_attn.q` -> `blocks.0.attn1.to_q`)."""
    m = _BLOCK.fullmatch(target)
    head, rest, table = (f"blocks.{m.group(1)}.", m.group(2), _DIFFUSERS_BLOCK) if m else ("", target, _DIFFUSERS_TOP)
    rest = "." + rest + "."
    for theirs, ours in table:
        rest = rest.replace("." + ours + ".", "." + theirs + ".")
    return head + rest[1:-1]


def extended_targets(model_shapes):
    """{canonical target: ("linear" | "norm", weight tensor key, row0, rows, cols, bias tensor key or None, bias0, bias_n)} of
    everything an extended adapter may touch: every Linear of `model_shapes`, the q / k RMSNorm weights and norm3."""
    out = {}
    for key, shape in model_shapes.items():
        if not key.endswith(".weight"):
            continue
        target = key[:-len(".weight")]
        m = _BLOCK.fullmatch(target)
        if m is None:
            if target in _TOP_TENSORS and len(shape) == 2:
                t = _TOP_TENSORS[target]
                out[target] = ("linear", t + "_w", 0, shape[0], shape[1], t + "_b", 0, shape[0])
            continue
        layer, rest = m.group(1), m.group(2)
        if rest in _NORM_TENSORS:
            bias = f"L{layer}.norm3_b" if rest == "norm3" else None
            out[target] = ("norm", f"L{layer}.{_NORM_TENSORS[rest]}", 0, 1, shape[0], bias, 0, shape[0] if bias else 0)
            continue
        lm = _TARGET.fullmatch(target)
        if lm is None or len(shape) != 2:
            continue
        attn, proj, ffn = lm.group(2), lm.group(3), lm.group(4)
        row0 = 0
        if ffn is not None:
            field = f"ffn{ffn}"
        elif attn == "cross_attn":
            field = f"c{proj}"
        elif proj == "o":
            field = "o"
        else:
            field, row0 = "qkv", "qkv".index(proj) * shape[0]
        out[target] = ("linear", f"L{layer}.{field}_w", row0, shape[0], shape[1], f"L{layer}.{field}_b", row0, shape[0])
    return out


def flattened_names(model_shapes):
    """{flattened kohya name without `lora_unet_`: canonical target}: every target in its canonical and its diffusers spelling with
    each `.` replaced by `_`.  A flattened key is resolved by exact lookup here, never by splitting on underscores."""
    out = {}
    for target in extended_targets(model_shapes):
        for spelling in (target, diffusers_name(target)):
            out[spelling.replace(".", "_")] = target
    return out


def _parse_extended(sd, model_shapes, strict):
    """parse_lora_state_dict(extended=True).  Every key is normalised to (canonical target, part), then treated as before.
    Prefixes: those of the default plus `transformer.`.  Names: canonical (`blocks.0.self_attn.q`), diffusers (`blocks.0.attn1.to_q`,
    `condition_embedder...`, `proj_out`: _DIFFUSERS_BLOCK / _DIFFUSERS_TOP) or flattened kohya (`lora_unet_blocks_0_self_attn_q`,
    of either spelling).  Targets: every Linear of the model for low-rank pairs (+ `.alpha`), `.diff` (the weight's shape), `.diff_b`
    (the bias' shape) and a DoRA vector (`.dora_scale`, `.lora_magnitude_vector[.weight]`; [out] or [out, 1]; needs the pair and
    excludes a `.diff`); `.diff` on the q / k norms and norm3, `.diff_b` on norm3.  Two keys for one slot, a DoRA vector without
    its pair, a wrong shape and a non-finite alpha raise a ValueError naming the key, beside everything the default raises.
    Anything else (`patch_embedding`, `modulation`, unknown names) is unexpected."""
    kinds = extended_targets(model_shapes)
    by_diffusers = {diffusers_name(t): t for t in kinds}
    flat = flattened_names(model_shapes)
    found, unexpected = {}, []
    for key in sd:
        name = next((key[len(p):] for p in _EXT_PREFIXES if key.startswith(p)), key)
        target = part = None
        if name.startswith("lora_unet_"):
            stem, dot, suffix = name[len("lora_unet_"):].partition(".")
            if dot + suffix in _EXT_SUFFIXES:
                target, part = flat.get(stem), _EXT_SUFFIXES[dot + suffix]
        else:
            suffix = next((s for s in _EXT_SUFFIXES if name.endswith(s)), None)
            if suffix:
                stem, part = name[:-len(suffix)], _EXT_SUFFIXES[suffix]
                target = stem if stem in kinds else by_diffusers.get(stem)
        if target is None or (kinds[target][0] == "norm" and part not in ("diff", "diff_b")) \
                or (part == "diff_b" and kinds[target][5] is None):
            unexpected.append(key)
            continue
        slot = found.setdefault(target, {})
        if part in slot:
            raise ValueError(f"LoRA key {key!r} repeats {slot[part][0]!r}: both name the {part} of {target}")
        slot[part] = (key, sd[key])
    if unexpected and strict:
        raise ValueError("unexpected key(s) in LoRA state dict: " + ", ".join(repr(k) for k in sorted(unexpected)[:12])
                         + (f" ... ({len(unexpected)} in total)" if len(unexpected) > 12 else ""))
    targets = {}
    for target, slot in sorted(found.items()):
        _, tensor, row0, rows, cols, bias, bias0, bias_n = kinds[target]
        for have, lack in (("A", "B"), ("B", "A"), ("alpha", "A")):
            if have in slot and lack not in slot:
                raise ValueError(f"LoRA key {slot[have][0]!r} has no lora_{lack} / lora_{'up' if lack == 'B' else 'down'} partner")
        A = B = diff = diff_b = dora = None
        rank, factor = 0, 1.0
        if "A" in slot:
            (ka, A), (kb, B) = slot["A"], slot["B"]
            if A.ndim != 2 or A.shape[1] != cols:
                raise ValueError(f"LoRA key {ka!r}: shape {tuple(A.shape)} does not fit, {target} wants A [rank, {cols}]")
            rank = int(A.shape[0])
            if rank < 1 or rank > MAX_RANK:
                raise ValueError(f"LoRA key {ka!r}: rank {rank} outside 1 .. {MAX_RANK}")
            if tuple(B.shape) != (rows, rank):
                raise ValueError(f"LoRA key {kb!r}: shape {tuple(B.shape)} does not fit, {target} wants B [{rows}, {rank}]")
        if "alpha" in slot:
            kal, alpha = slot["alpha"]
            if torch.is_tensor(alpha) and alpha.numel() != 1:
                raise ValueError(f"LoRA key {kal!r}: alpha must be a scalar, not shape {tuple(alpha.shape)}")
            factor = float(alpha) / rank
            if not math.isfinite(factor):
                raise ValueError(f"LoRA key {kal!r}: alpha is not finite")
        if "diff" in slot:
            kd, diff = slot["diff"]
            want = (cols,) if kinds[target][0] == "norm" else (rows, cols)
            if tuple(diff.shape) != want:
                raise ValueError(f"LoRA key {kd!r}: shape {tuple(diff.shape)} does not fit, {target} wants a diff {list(want)}")
        if "diff_b" in slot:
            kd, diff_b = slot["diff_b"]
            if tuple(diff_b.shape) != (bias_n,):
                raise ValueError(f"LoRA key {kd!r}: shape {tuple(diff_b.shape)} does not fit, {target} wants a diff_b [{bias_n}]")
        if "dora" in slot:
            kd, dora = slot["dora"]
            if A is None:
                raise ValueError(f"LoRA key {kd!r}: a DoRA magnitude vector without its lora_A / lora_B (lora_down / lora_up) pair")
            if diff is not None:
                raise ValueError(f"LoRA key {kd!r}: a DoRA magnitude vector beside {slot['diff'][0]!r}: the DoRA merge is not "
                                 "additive and takes no dense delta")
            if tuple(dora.shape) == (1, cols):      # (checked first: with in == out this is still the per-input form)
                raise ValueError(f"LoRA key {kd!r}: shape [1, {cols}] is a per-input-column magnitude (the LyCORIS decomposition "
                                 f"over the output axis); only the per-output-row form [{rows}] / [{rows}, 1] is merged")
            if tuple(dora.shape) not in ((rows,), (rows, 1)):
                raise ValueError(f"LoRA key {kd!r}: shape {tuple(dora.shape)} does not fit, {target} wants a magnitude vector "
                                 f"[{rows}] or [{rows}, 1]")
            dora = dora.reshape(rows)
        has_b = diff_b is not None
        targets[target] = Target(tensor, row0, rows, cols, rank, factor, A, B, diff, diff_b, bias if has_b else None,
                                 bias0 if has_b else 0, bias_n if has_b else 0, dora)
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


_Term = _lib.LORA_EXT_STRUCTS["rtv_lora_term"]


def _check_views(what, base, out):
    if not (base.is_cuda and out.is_cuda):
        raise RuntimeError("the LoRA merge is a HIP kernel: it needs GPU tensors (no CPU fallback)")
    for t in (base, out):
        if t.dtype != torch.bfloat16 or t.ndim != 2 or t.stride(1) != 1:
            raise ValueError(f"{what}: base / out must be bf16 [N, K] with unit column stride")
    if base.shape != out.shape:
        raise ValueError(f"{what}: base and out differ in shape")


def _dense(what, t, shape):
    if t.dtype != torch.bfloat16 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: A [r, K] / B [N, r] / mag [N] must be dense bf16 device tensors")


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]      # (the stride of a single row is never used)


def merge_ex(base, out, terms, stream=None):
    """out = bf16(base + sum (scale * B @ A + diff_scale * diff)) over one matrix, row range or - as [1, K] - vector
    (rtv_lora_merge_ex).  `terms` is a list of (A, B, scale, diff, diff_scale): A [r, K] / B [N, r] dense bf16 device tensors or
    both None, diff a bf16 [N, K] view with unit column stride or None.  One launch on the current stream."""
    _check_views("lora merge_ex", base, out)
    N, K = base.shape
    table = (_Term * max(1, len(terms)))()
    for i, (A, B, scale, diff, diff_scale) in enumerate(terms):
        if (A is None) != (B is None):
            raise ValueError("lora merge_ex: half a low-rank pair")
        if A is not None:
            _dense("lora merge_ex", A, (A.shape[0], K))
            _dense("lora merge_ex", B, (N, A.shape[0]))
        if diff is not None and (diff.dtype != torch.bfloat16 or not diff.is_cuda or tuple(diff.shape) != (N, K) or diff.stride(1) != 1):
            raise ValueError("lora merge_ex: diff must be a bf16 [N, K] device tensor with unit column stride")
        table[i] = _Term(A.data_ptr() if A is not None else None, B.data_ptr() if B is not None else None,
                         int(A.shape[0]) if A is not None else 0, float(scale), diff.data_ptr() if diff is not None else None,
                         _ld(diff) if diff is not None else 0, float(diff_scale))
    if stream is None:
        stream = torch.cuda.current_stream(base.device).cuda_stream
    with torch.cuda.device(base.device):
        _lib.call("rtv_lora_merge_ex", base.data_ptr(), _ld(base), out.data_ptr(), _ld(out), N, K, table if terms else None,
                  len(terms), ctypes.c_void_p(stream))
    return out


def dora_workspace_bytes(N, K):
    return int(_lib.load().rtv_lora_dora_workspace_bytes(int(N), int(K)))


def merge_dora(base, out, A, B, factor, mag, strength, workspace, stream=None):
    """out = bf16(base + strength * (g * V - base)), V = base + factor * B @ A, g[n] = mag[n] / ||V[n]|| (rtv_lora_merge_dora) over
    one matrix or row range.  `mag` bf16 [N]; `workspace` a device tensor of at least dora_workspace_bytes(N, K) bytes.  Two
    launches on the current stream."""
    _check_views("lora merge_dora", base, out)
    N, K = base.shape
    _dense("lora merge_dora", A, (A.shape[0], K))
    _dense("lora merge_dora", B, (N, A.shape[0]))
    _dense("lora merge_dora", mag, (N,))
    if not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("lora merge_dora: the workspace must be a dense device tensor")
    if stream is None:
        stream = torch.cuda.current_stream(base.device).cuda_stream
    with torch.cuda.device(base.device):
        _lib.call("rtv_lora_merge_dora", base.data_ptr(), _ld(base), out.data_ptr(), _ld(out), N, K, A.data_ptr(), B.data_ptr(),
                  int(A.shape[0]), float(factor), mag.data_ptr(), float(strength), workspace.data_ptr(),
                  workspace.numel() * workspace.element_size(), ctypes.c_void_p(stream))
    return out
