"""Thin tensor-level wrappers over the C-ABI kernels (device pointers + sizes + current HIP stream).

PyTorch is plumbing here: it owns device memory and the stream; all arithmetic happens in
librtv_hip.so.  Every wrapper refuses non-GPU tensors (no CPU fallback).
"""
import collections
import ctypes
import math

import torch

from . import _lib

ACT_NONE, ACT_GELU_TANH, ACT_SILU = 0, 1, 2
DT_BF16, DT_F16 = 0, 1
PROF_CLASSES = {"gemm": 0, "attn": 1, "layernorm": 2, "rope": 3, "conv": 4, "misc": 5}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t):
    if t.dtype == torch.bfloat16:
        return DT_BF16
    if t.dtype == torch.float16:
        return DT_F16
    raise TypeError(f"expected bfloat16 or float16 tensor, got {t.dtype}")


def _gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("realtime_video_amd kernels need GPU tensors (no CPU fallback)")


# --------------------------------------------------------------------------------------- profiling
def prof_enable(on=True, classes=None):
    """Bracket kernel launches with hipEvents: all classes, or only `classes` (names from PROF_CLASSES)."""
    mask = 0
    if on:
        mask = 0x3F if classes is None else sum(1 << PROF_CLASSES[c] for c in classes)
    _lib.call("rtv_prof_enable", int(mask))


def prof_reset():
    _lib.call("rtv_prof_reset")


def prof_set_stride(cls, stride):
    """Bracket only every `stride`-th launch of a class (an event pair costs the stream a few microseconds; prof_read then
    carries the sampled launches and `seen_*` all of them)."""
    _lib.call("rtv_prof_set_stride", PROF_CLASSES[cls] if isinstance(cls, str) else int(cls), int(stride))


def prof_bracket_overhead(n=256):
    """ms an EMPTY event bracket reads on the current stream (rtv_prof_bracket_overhead): what every bracketed launch's time
    carries on top of its kernel.  Synchronises."""
    ms = ctypes.c_double(0)
    _lib.call("rtv_prof_bracket_overhead", int(n), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.byref(ms))
    return ms.value


def dispatch_counts(reset=False):
    """{kernel variant name: launches since load / the last reset} for the variants that ran (rtv_dispatch_counts): which GEMM /
    attention / conv kernels the dispatch rules actually chose."""
    lib = _lib.load()
    n = lib.rtv_dispatch_counts(None, 0)
    buf = (ctypes.c_int64 * n)()
    lib.rtv_dispatch_counts(buf, n)
    out = {lib.rtv_dispatch_name(i).decode(): int(buf[i]) for i in range(n) if buf[i]}
    if reset:
        lib.rtv_dispatch_reset()
    return out


def prof_read(cls):
    """-> ms / launches / work of the BRACKETED launches, seen_launches / seen_work of all launches of the class, and `ms_class` =
    the bracketed time scaled to the whole class by work."""
    c = PROF_CLASSES[cls] if isinstance(cls, str) else int(cls)
    ms, n, work = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
    _lib.call("rtv_prof_read", c, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(work))
    sn, swork = ctypes.c_int64(0), ctypes.c_double(0)
    _lib.call("rtv_prof_read_seen", c, ctypes.byref(sn), ctypes.byref(swork))
    scale = swork.value / work.value if work.value > 0 else 1.0
    return {"ms": ms.value, "launches": n.value, "work": work.value, "seen_launches": sn.value, "seen_work": swork.value,
            "ms_class": ms.value * scale}


# --------------------------------------------------------------------------------------- attention
def attn_set_waves(waves=0):
    """Workgroup shape / kernel of attn_fwd (rtv_attn_set_waves, include/rtv_hip_lab.h): 0 = by grid size and window; 4 / 8 = 128 /
    256 query rows; 81 / 82 = 256 rows on the lockstep / four-phase schedule; 840 + v = the one-wave-per-SIMD kernel, variant v."""
    _lib.call("rtv_attn_set_waves", int(waves))


def attn_fwd(q, k, v, out=None, scale=None, causal_block=0, q_offset=0):
    """softmax(scale q k^T) v.  q:[B,Lq,H,128], k/v:[B,Lkv,H,128] (strided views allowed as long as
    the last two dims are dense), returns [B,Lq,H,128] contiguous."""
    _gpu(q, k, v)
    B, Lq, H, D = q.shape
    Lkv = k.shape[1]
    if k.shape != v.shape or k.shape[0] != B or k.shape[2] != H or k.shape[3] != D:
        raise ValueError(f"attention shape mismatch q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)}")
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("q, k, v must share a dtype")
    for t in (q, k, v):
        if t.stride(3) != 1 or t.stride(2) != D:
            raise ValueError("attention operands need dense [H, D] inner dims (BLHD layout)")
    if out is None:
        out = torch.empty((B, Lq, H, D), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    _lib.call("rtv_attn_fwd", _ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Lq, Lkv, H, D,
              q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
              out.stride(0), out.stride(1), float(scale), int(causal_block), int(q_offset), _dt(q), _stream())
    return out


def attn_fwd_dup(q, k, v, dup_key, dup_count, out=None, scale=None):
    """Dense attention in which key `dup_key` of the window stands for `dup_count` identical keys (rtv_attn_fwd_dup)."""
    _gpu(q, k, v)
    B, Lq, H, D = q.shape
    Lkv = k.shape[1]
    if k.shape != v.shape or k.shape[0] != B or k.shape[2] != H or k.shape[3] != D:
        raise ValueError(f"attention shape mismatch q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)}")
    for t in (q, k, v):
        if t.stride(3) != 1 or t.stride(2) != D:
            raise ValueError("attention operands need dense [H, D] inner dims (BLHD layout)")
    if out is None:
        out = torch.empty((B, Lq, H, D), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    _lib.call("rtv_attn_fwd_dup", _ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Lq, Lkv, H, D,
              q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
              out.stride(0), out.stride(1), float(scale), int(dup_key), int(dup_count), _dt(q), _stream())
    return out


def cross_fold_dims(num_heads, text_rows):
    """-> (applies, kh, k_fold): the column layout of the folded cross-attention (rtv_cross_fold_dims)."""
    kh, kf = ctypes.c_int(0), ctypes.c_int(0)
    ok = _lib.load().rtv_cross_fold_dims(int(num_heads), int(text_rows), ctypes.byref(kh), ctypes.byref(kf))
    return bool(ok), kh.value, kf.value


def attn_probs_dup(q, k, dup_key, dup_count, kh, p_cols, out=None, scale=None):
    """Softmax probabilities of a short key window with a counted key (rtv_attn_probs_dup).  q [Lq, H, 128], k [Lkv, H, 128]
    -> [Lq, p_cols] bf16 with head h's keys in columns [h * kh, h * kh + Lkv) and zeros in every other column."""
    _gpu(q, k)
    Lq, H, D = q.shape
    Lkv = k.shape[0]
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16:
        raise TypeError("attn_probs_dup is bf16 only")
    for t in (q, k):
        if t.stride(2) != 1 or t.stride(1) != D:
            raise ValueError("attention operands need dense [H, D] inner dims")
    if out is None:
        out = torch.empty((Lq, p_cols), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    _lib.call("rtv_attn_probs_dup", _ptr(q), _ptr(k), _ptr(out), Lq, Lkv, H, D, q.stride(0), k.stride(0), out.stride(0),
              int(kh), int(p_cols), float(scale), int(dup_key), int(dup_count), _stream())
    return out


def cross_fold_weight(co_w, v, rows, kh, k_fold, out=None):
    """vo[n, h * kh + t] = sum_d' co_w[n, h * 128 + d'] * v[t, h * 128 + d'] for t < rows, zeros elsewhere (rtv_cross_fold_weight).
    co_w [d, d], v [>= rows, d] bf16 -> [d, k_fold] bf16."""
    _gpu(co_w, v)
    d = co_w.shape[0]
    if out is None:
        out = torch.empty((d, k_fold), dtype=torch.bfloat16, device=co_w.device)
    _lib.call("rtv_cross_fold_weight", _ptr(co_w), co_w.stride(0), _ptr(v), v.stride(0), _ptr(out), out.stride(0), d // 128,
              int(rows), int(kh), int(k_fold), _stream())
    return out


def attn_fwd_win(q, k_cache, v_cache, seg0, seg1=(0, 0), out=None, scale=None):
    """Attention over a key window made of two row ranges of a cache (rtv_attn_fwd_win): k_cache / v_cache [B, rows, H, 128],
    seg = (first_row, n_rows).  How a ring-indexed rolling KV cache is attended without the reference's shift copy."""
    _gpu(q, k_cache, v_cache)
    B, Lq, H, D = q.shape
    (r0, n0), (r1, n1) = seg0, seg1
    rows = k_cache.shape[1]
    if min(r0, n0, r1, n1) < 0 or r0 + n0 > rows or (n1 and r1 + n1 > rows):
        raise ValueError("attn_fwd_win: segment outside the cache")
    for t in (q, k_cache, v_cache):
        if t.stride(3) != 1 or t.stride(2) != D:
            raise ValueError("attention operands need dense [H, D] inner dims (BLHD layout)")
    if out is None:
        out = torch.empty((B, Lq, H, D), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    k, v = k_cache[:, r0:], v_cache[:, r0:]
    _lib.call("rtv_attn_fwd_win", _ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Lq, n0, n1,
              (r1 - r0) if n1 else 0, H, D, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
              out.stride(0), out.stride(1), float(scale), 0, 0, _dt(q), _stream())
    return out


def attn_fwd_split(q, k_cache, v_cache, seg0, seg1=(0, 0), kv_splits=2, out=None, scale=None, workspace=None, causal_block=0,
                   q_offset=0):
    """attn_fwd_win with the key window cut into `kv_splits` ranges, one workgroup per (head, query tile, range), merged by a
    second kernel (rtv_attn_fwd_split): for launches too small to fill the chip.  workspace: fp32 tensor of at least
    kv_splits * B * H * Lq * 130 elements (allocated when None)."""
    _gpu(q, k_cache, v_cache)
    B, Lq, H, D = q.shape
    (r0, n0), (r1, n1) = seg0, seg1
    rows = k_cache.shape[1]
    if min(r0, n0, r1, n1) < 0 or r0 + n0 > rows or (n1 and r1 + n1 > rows):
        raise ValueError("attn_fwd_split: segment outside the cache")
    for t in (q, k_cache, v_cache):
        if t.stride(3) != 1 or t.stride(2) != D:
            raise ValueError("attention operands need dense [H, D] inner dims (BLHD layout)")
    if out is None:
        out = torch.empty((B, Lq, H, D), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if workspace is None:
        need = _lib.load().rtv_attn_split_workspace_bytes(B, Lq, H, int(kv_splits))
        workspace = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=q.device)
    k, v = k_cache[:, r0:], v_cache[:, r0:]
    _lib.call("rtv_attn_fwd_split", _ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Lq, n0, n1,
              (r1 - r0) if n1 else 0, H, D, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
              out.stride(0), out.stride(1), float(scale), int(causal_block), int(q_offset), int(kv_splits), _ptr(workspace),
              workspace.numel() * workspace.element_size(), _dt(q), _stream())
    return out


# --------------------------------------------------------------------------------------- fp8 attention (e4m3 shadow of a KV cache)
def attn_fp8_shadow(cache_rows, H, device):
    """Zero-filled shadow of a cache [cache_rows][H][128]: (k8 uint8 [cache_rows, H, 128], v8t uint8 [ceil(cache_rows / 64), H, 128, 64])."""
    return (torch.zeros((cache_rows, H, 128), dtype=torch.uint8, device=device),
            torch.zeros(((cache_rows + 63) // 64, H, 128, 64), dtype=torch.uint8, device=device))


def _check_shadow(k8, v8t, what):
    _gpu(k8, v8t)
    if k8.dtype != torch.uint8 or v8t.dtype != torch.uint8 or k8.dim() != 3 or v8t.dim() != 4 or not (k8.is_contiguous() and v8t.is_contiguous()):
        raise ValueError(f"{what}: k8 / v8t must be dense uint8 tensors [rows, H, 128] / [tiles, H, 128, 64]")
    rows, H, D = k8.shape
    if D != 128 or tuple(v8t.shape) != ((rows + 63) // 64, H, 128, 64):
        raise ValueError(f"{what}: v8t must be [ceil(rows / 64), H, 128, 64] for k8 [rows, H, 128]")
    return rows, H


def _check_center(center, H, what):
    if center.dtype != torch.float32 or tuple(center.shape) != (H, 128) or not center.is_contiguous() or center.data_ptr() % 16:
        raise ValueError(f"{what}: center must be a dense, 16-byte aligned float32 tensor [H, 128]")


def attn_kv_center_workspace_bytes(rows, H):
    """Bytes of workspace attn_kv_center needs for a window of `rows` rows and H heads (rtv_attn_kv_center_workspace_bytes)."""
    return int(_lib.load().rtv_attn_kv_center_workspace_bytes(int(rows), int(H)))


def attn_kv_center(k_cache, seg0, seg1=(0, 0), out=None, workspace=None):
    """fp32 column means [H, 128] of the bf16 K rows of the window seg0 + seg1 (each (first physical row, rows)) of a cache
    k_cache [rows, H, 128] (rtv_attn_kv_center; the K plane of an interleaved arena is fine): the centre a smoothed shadow subtracts
    (attn_quantize_kv(..., center=)).  Deterministic: the same rows give the same bits.  workspace: float32 tensor of at least
    rtv_attn_kv_center_workspace_bytes(rows of the window, H) bytes (allocated when None)."""
    _gpu(k_cache, out, workspace)
    if k_cache.dtype != torch.bfloat16 or k_cache.dim() != 3 or k_cache.shape[2] != 128 or k_cache.stride(2) != 1 or k_cache.stride(1) != 128:
        raise ValueError("attn_kv_center: k_cache must be bf16 [rows, H, 128] with dense [H, 128] inner dims")
    cache_rows, H = k_cache.shape[0], k_cache.shape[1]
    (r0, n0), (r1, n1) = seg0, seg1
    if min(r0, n0, r1, n1) < 0 or r0 + n0 > cache_rows or (n1 and r1 + n1 > cache_rows):
        raise ValueError("attn_kv_center: segment outside the cache")
    if out is None:
        out = torch.empty((H, 128), dtype=torch.float32, device=k_cache.device)
    _check_center(out, H, "attn_kv_center")
    need = attn_kv_center_workspace_bytes(n0 + n1, H)
    if workspace is None:
        workspace = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=k_cache.device)
    elif workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise ValueError("attn_kv_center: workspace must be a dense float32 tensor")
    _lib.call("rtv_attn_kv_center", _ptr(k_cache), k_cache.stride(0), int(r0), int(n0), int(r1), int(n1), H, _ptr(out), _ptr(workspace),
              workspace.numel() * 4, _stream())
    return out


def attn_quantize_kv(k_cache, v_cache, k8, v8t, row0=0, rows=None, k_scale=1.0, v_scale=1.0, amax=None, center=None):
    """Quantise the physical rows [row0, row0 + rows) of a bf16 KV cache (k_cache / v_cache [rows, H, 128] with one row stride; the
    two planes of an interleaved arena are fine) into its e4m3 shadow (rtv_attn_quantize_kv).  amax: optional float32 [2] tensor,
    the running maxima of |k| and |v|.  center: optional float32 [H, 128]: the K codes are those of k - center, and amax[0] follows
    |k - center| (rtv_attn_quantize_kv_centered, include/rtv_hip_attn_fp8_center.h)."""
    _gpu(k_cache, v_cache, amax, center)
    cache_rows, H = _check_shadow(k8, v8t, "attn_quantize_kv")
    for t in (k_cache, v_cache):
        if t.dtype != torch.bfloat16 or t.dim() != 3 or tuple(t.shape) != (cache_rows, H, 128) or t.stride(2) != 1 or t.stride(1) != 128:
            raise ValueError("attn_quantize_kv: caches must be bf16 [rows, H, 128] with dense [H, 128] inner dims, rows as in k8")
    if k_cache.stride(0) != v_cache.stride(0):
        raise ValueError("attn_quantize_kv: K and V need the same row stride")
    if amax is not None and (amax.dtype != torch.float32 or amax.numel() != 2 or not amax.is_contiguous()):
        raise ValueError("attn_quantize_kv: amax must be a dense float32 tensor of 2 elements")
    if rows is None:
        rows = cache_rows - row0
    if center is not None:
        _check_center(center, H, "attn_quantize_kv")
        _lib.call("rtv_attn_quantize_kv_centered", _ptr(k_cache), _ptr(v_cache), k_cache.stride(0), int(row0), int(rows), H, _ptr(k8),
                  _ptr(v8t), cache_rows, float(k_scale), float(v_scale), _ptr(amax), _ptr(center), _stream())
        return k8, v8t
    _lib.call("rtv_attn_quantize_kv", _ptr(k_cache), _ptr(v_cache), k_cache.stride(0), int(row0), int(rows), H, _ptr(k8), _ptr(v8t),
              cache_rows, float(k_scale), float(v_scale), _ptr(amax), _stream())
    return k8, v8t


def attn_fwd_fp8(q, k8, v8t, seg0, seg1=(0, 0), out=None, scale=None, k_scale=1.0, v_scale=1.0, causal_block=0, q_offset=0, kv_splits=1,
                 workspace=None):
    """fp8 attention of q [Lq, H, 128] bf16 over the key window seg0 + seg1 (each (first physical row, rows)) of a shadow
    (rtv_attn_fwd_fp8).  causal_block > 0: the block-causal prefix rule of attn_fwd, one range only.
    kv_splits > 1, or a workspace: the window's storage tiles cut into kv_splits ranges, one workgroup per (head, query tile, range),
    merged by a second kernel (rtv_attn_fwd_fp8_split, include/rtv_hip_attn_fp8_cp.h).  workspace: float32 tensor of at least
    rtv_attn_split_workspace_bytes(1, Lq, H, kv_splits) bytes (allocated when None)."""
    _gpu(q, out, workspace)
    cache_rows, H = _check_shadow(k8, v8t, "attn_fwd_fp8")
    if q.dtype != torch.bfloat16 or q.dim() != 3 or q.shape[1] != H or q.shape[2] != 128 or q.stride(2) != 1 or q.stride(1) != 128:
        raise ValueError("attn_fwd_fp8: q must be bf16 [Lq, H, 128] with dense [H, 128] inner dims, H as in k8")
    if out is None:
        out = torch.empty((q.shape[0], H, 128), dtype=q.dtype, device=q.device)
    elif out.dtype != q.dtype or out.shape != q.shape or out.stride(2) != 1 or out.stride(1) != 128:
        raise ValueError("attn_fwd_fp8: out must match q")
    if scale is None:
        scale = 1.0 / math.sqrt(128)
    (r0, n0), (r1, n1) = seg0, seg1
    if int(kv_splits) == 1 and workspace is None:
        _lib.call("rtv_attn_fwd_fp8", _ptr(q), _ptr(k8), _ptr(v8t), _ptr(out), q.shape[0], H, cache_rows, int(r0), int(n0), int(r1), int(n1),
                  q.stride(0), out.stride(0), float(scale), float(k_scale), float(v_scale), int(causal_block), int(q_offset), _stream())
        return out
    if workspace is None:
        need = _lib.load().rtv_attn_split_workspace_bytes(1, q.shape[0], H, int(kv_splits))
        workspace = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=q.device)
    elif workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise ValueError("attn_fwd_fp8: workspace must be a dense float32 tensor")
    _lib.call("rtv_attn_fwd_fp8_split", _ptr(q), _ptr(k8), _ptr(v8t), _ptr(out), q.shape[0], H, cache_rows, int(r0), int(n0), int(r1), int(n1),
              q.stride(0), out.stride(0), float(scale), float(k_scale), float(v_scale), int(causal_block), int(q_offset), int(kv_splits),
              _ptr(workspace), workspace.numel() * 4, _stream())
    return out


def qk_norm_rope_k8(qkv, k8, cache_row0, num_heads, wq, wk, rope_cs, grid, start_frame, eps=1e-6, q_out=None, row_offset=0,
                    ring=(0, 0, 0), k_scale=1.0, amax=None, want_q=True):
    """qk_norm_rope_cache with the K rows stored as e4m3 codes in k8 [cache_rows, H, 128] and no V role (rtv_qk_norm_rope_k8,
    include/rtv_hip_attn_fp8_only.h).  amax: optional float32 [2], [0] follows |k|.  want_q=False: no q role (the kv_only pass).
    A thin wrapper: the entry point itself refuses what it documents."""
    _gpu(qkv, k8, wq, wk, rope_cs, q_out, amax)
    M, d3 = qkv.shape
    d = d3 // 3
    F, gh, gw = grid
    if q_out is None and want_q:
        q_out = torch.empty((M, d), dtype=qkv.dtype, device=qkv.device)
    _lib.call("rtv_qk_norm_rope_k8", _ptr(qkv), _ptr(q_out) if want_q else None, _ptr(k8), k8.shape[0], float(k_scale), _ptr(amax),
              int(cache_row0), M, d, int(num_heads), float(eps), _ptr(wq), _ptr(wk), _ptr(rope_cs), int(F), int(gh), int(gw),
              int(start_frame), int(row_offset), int(ring[0]), int(ring[1]), int(ring[2]), _stream())
    return q_out


def qk_norm_rope_k8_centered(qkv, k8, cache_row0, num_heads, wq, wk, rope_cs, grid, start_frame, center, eps=1e-6, q_out=None,
                             row_offset=0, ring=(0, 0, 0), k_scale=1.0, amax=None, want_q=True):
    """qk_norm_rope_k8 with the K codes of k - center, center float32 [H, 128]; amax[0] follows |k - center|
    (rtv_qk_norm_rope_k8_centered, include/rtv_hip_attn_fp8_only_center.h).  A thin wrapper: the entry point itself refuses what it
    documents."""
    _gpu(qkv, k8, wq, wk, rope_cs, q_out, amax, center)
    M, d3 = qkv.shape
    d = d3 // 3
    F, gh, gw = grid
    if q_out is None and want_q:
        q_out = torch.empty((M, d), dtype=qkv.dtype, device=qkv.device)
    _lib.call("rtv_qk_norm_rope_k8_centered", _ptr(qkv), _ptr(q_out) if want_q else None, _ptr(k8), k8.shape[0], float(k_scale), _ptr(amax),
              int(cache_row0), M, d, int(num_heads), float(eps), _ptr(wq), _ptr(wk), _ptr(rope_cs), int(F), int(gh), int(gw),
              int(start_frame), int(row_offset), int(ring[0]), int(ring[1]), int(ring[2]), _ptr(center), _stream())
    return q_out


def _check_k8(k8, what):
    _gpu(k8)
    if k8.dtype != torch.uint8 or k8.dim() != 3 or k8.shape[2] != 128 or not k8.is_contiguous():
        raise ValueError(f"{what}: k8 must be a dense uint8 tensor [rows, H, 128]")
    return k8.shape[0], k8.shape[1]


def attn_k8_center(k8, seg0, seg1=(0, 0), k_scale=1.0, c_old=None, out=None, workspace=None):
    """The centre of a compact cache taken from its codes: c_old + the fp32 column means [H, 128] of code * k_scale over the window
    seg0 + seg1 (each (first physical row, rows)) of k8 [rows, H, 128] (rtv_attn_k8_center,
    include/rtv_hip_attn_fp8_only_center.h).  c_old: the centre the codes stand under (None: zeros).  Deterministic: the same input
    gives the same bits.  workspace as for attn_kv_center."""
    _gpu(c_old, out, workspace)
    cache_rows, H = _check_k8(k8, "attn_k8_center")
    (r0, n0), (r1, n1) = seg0, seg1
    if c_old is None:
        c_old = torch.zeros((H, 128), dtype=torch.float32, device=k8.device)
    if out is None:
        out = torch.empty((H, 128), dtype=torch.float32, device=k8.device)
    _check_center(c_old, H, "attn_k8_center")
    _check_center(out, H, "attn_k8_center")
    need = attn_kv_center_workspace_bytes(n0 + n1, H)
    if workspace is None:
        workspace = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=k8.device)
    elif workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise ValueError("attn_k8_center: workspace must be a dense float32 tensor")
    _lib.call("rtv_attn_k8_center", _ptr(k8), cache_rows, int(r0), int(n0), int(r1), int(n1), H, float(k_scale), _ptr(c_old), _ptr(out),
              _ptr(workspace), workspace.numel() * 4, _stream())
    return out


def attn_k8_recenter(k8, c_old, c_new, row0=0, rows=None, k_scale=1.0, amax=None):
    """Move the rows [row0, row0 + rows) of k8 [rows, H, 128] from the centre c_old to the centre c_new (float32 [H, 128]), in place:
    code' = e4m3((code * k_scale + (c_old - c_new)) / k_scale) (rtv_attn_k8_recenter, whose header states the arithmetic).  amax:
    optional float32 [2], [0] is raised to the largest |code * k_scale + (c_old - c_new)|."""
    _gpu(c_old, c_new, amax)
    cache_rows, H = _check_k8(k8, "attn_k8_recenter")
    _check_center(c_old, H, "attn_k8_recenter")
    _check_center(c_new, H, "attn_k8_recenter")
    if amax is not None and (amax.dtype != torch.float32 or amax.numel() != 2 or not amax.is_contiguous()):
        raise ValueError("attn_k8_recenter: amax must be a dense float32 tensor of 2 elements")
    if rows is None:
        rows = cache_rows - row0
    _lib.call("rtv_attn_k8_recenter", _ptr(k8), cache_rows, int(row0), int(rows), H, float(k_scale), _ptr(c_old), _ptr(c_new), _ptr(amax),
              _stream())
    return k8


def attn_quantize_v_rows(v_src, v8t, cache_rows, dst_row0, v_scale=1.0, amax=None):
    """Quantise the bf16 rows v_src [rows, H, 128] (any row stride: the V third of a projection buffer is fine) into the physical rows
    [dst_row0, dst_row0 + rows) of v8t (rtv_attn_quantize_v_rows, include/rtv_hip_attn_fp8_only.h).  amax: optional float32 [2], [1]
    follows |v|.  A thin wrapper: the entry point itself refuses what it documents."""
    _gpu(v_src, v8t, amax)
    rows, H = v_src.shape[0], v_src.shape[1]
    _lib.call("rtv_attn_quantize_v_rows", _ptr(v_src), v_src.stride(0), rows, H, _ptr(v8t), int(cache_rows), int(dst_row0), float(v_scale),
              _ptr(amax), _stream())
    return v8t


def attn_fp8_staging(M, H, world, device, fill=0):
    """The staging buffer of the code exchange (include/rtv_hip_attn_fp8_only_cp.h): uint8 [world, 2, M / world, H * 128], rank r's
    K codes then its V codes, one contiguous message per rank."""
    if world <= 0 or M % world:
        raise ValueError(f"attn_fp8_staging: {M} rows are not divisible by the context-parallel degree {world}")
    return torch.full((world, 2, M // world, H * 128), fill, dtype=torch.uint8, device=device)


def attn_fp8_stage_kv8(qkv, kv8, row_begin, num_heads, wk, rope_cs, grid, start_frame, eps=1e-6, k_scale=1.0, v_scale=1.0, amax=None):
    """The codes of the logical rows [row_begin, row_begin + rows) of a block of F * gh * gw rows (qkv [rows, 3 d] bf16, the
    projection output of those rows) into the staging buffer kv8 [world, 2, M / world, d] (rtv_attn_fp8_stage_kv8).  amax: optional
    float32 [2], raised over the rows written.  A thin wrapper: the entry point itself refuses what it documents."""
    _gpu(qkv, kv8, wk, rope_cs, amax)
    rows, d3 = qkv.shape
    F, gh, gw = grid
    _lib.call("rtv_attn_fp8_stage_kv8", _ptr(qkv), _ptr(kv8), kv8.shape[0], int(row_begin), rows, float(k_scale), float(v_scale), _ptr(amax),
              d3 // 3, int(num_heads), float(eps), _ptr(wk), _ptr(rope_cs), int(F), int(gh), int(gw), int(start_frame), _stream())
    return kv8


def attn_fp8_commit_kv8(kv8, k8, v8t, cache_row0, ring=(0, 0, 0)):
    """The M = world * kv8.shape[2] rows of a gathered staging buffer into the logical rows [cache_row0, cache_row0 + M) of k8 / v8t,
    ring = (ring_lo, ring_size, ring_shift) of the cache (rtv_attn_fp8_commit_kv8).  A thin wrapper: the entry point itself refuses
    what it documents."""
    _gpu(kv8, k8, v8t)
    world, _, S, d = kv8.shape
    _lib.call("rtv_attn_fp8_commit_kv8", _ptr(kv8), world, world * S, d // 128, _ptr(k8), _ptr(v8t), k8.shape[0], int(cache_row0),
              int(ring[0]), int(ring[1]), int(ring[2]), _stream())
    return k8, v8t


# --------------------------------------------------------------------------------------- GEMM
_gemm_ws = {}


def ensure_gemm_workspace(device, stream=None):
    """Attach a split-K workspace (fp32 partial tiles + arrival counters, 64 MiB) for GEMM launches on `stream` (default: the
    current stream) of `device`.  One workspace per (device, stream): two streams - or two devices - never share slabs or
    arrival counters (rtv_gemm_set_stream_workspace)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if stream is None:
        stream = torch.cuda.current_stream(idx).cuda_stream
    key = (idx, int(stream))
    if key in _gemm_ws:
        return
    n = _lib.load().rtv_gemm_workspace_bytes()
    with torch.cuda.device(idx):
        ws = torch.zeros(n + 256, dtype=torch.uint8, device=torch.device("cuda", idx))
        off = (-ws.data_ptr()) % 256
        try:
            _lib.call("rtv_gemm_set_stream_workspace", ctypes.c_void_p(int(stream)), ctypes.c_void_p(ws.data_ptr() + off),
                      ctypes.c_size_t(n))
        except RuntimeError as e:
            if "too many workspaces" not in str(e):
                raise
            # the library's table (64 streams over all devices) is full: GEMMs on this stream run WITHOUT split-K (same
            # results up to fp32 association, a few per cent slower on partial tile rounds) instead of failing the forward
            import warnings
            warnings.warn("rtv: split-K workspace table full; GEMMs on this stream run unsplit "
                          "(release_gemm_workspace() frees the entry of a stream that is no longer used)")
            ws = None
    _gemm_ws[key] = ws


def release_gemm_workspace(device, stream):
    """Detach and free the split-K workspace of a stream that will not launch GEMMs any more (e.g. before it is destroyed).
    Waits for the stream first: a launch still in flight may be using the slabs."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    handle = int(stream.cuda_stream if hasattr(stream, "cuda_stream") else stream)
    ws = _gemm_ws.pop((idx, handle), None)
    if ws is None:
        return
    with torch.cuda.device(idx):
        if hasattr(stream, "synchronize"):
            stream.synchronize()
        else:
            torch.cuda.synchronize(idx)
        _lib.call("rtv_gemm_set_stream_workspace", ctypes.c_void_p(handle), ctypes.c_void_p(0), ctypes.c_size_t(0))


def gemm(a, w, bias=None, act=ACT_NONE, gate=None, gate_stride=0, rows_per_frame=0, residual=None,
         out=None, tile_cfg=0, row_offset=0):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T) — nn.Linear with fused bias/activation/gate/residual."""
    _gpu(a, w, bias, gate, residual, out)
    if a.dim() != 2 or w.dim() != 2 or a.shape[1] != w.shape[1]:
        raise ValueError(f"gemm shape mismatch a{tuple(a.shape)} w{tuple(w.shape)}")
    if a.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError("gemm operands must be K-contiguous")
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    if tile_cfg in (0, 5, 7, 50):
        ensure_gemm_workspace(a.device)
    _lib.call("rtv_gemm", _ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(out), out.stride(0), M, N, K,
              _ptr(bias), int(act), _ptr(gate), int(gate_stride), int(rows_per_frame), int(row_offset),
              _ptr(residual), residual.stride(0) if residual is not None else 0,
              _dt(a), int(tile_cfg), _stream())
    return out


# --------------------------------------------------------------------------------------- fp8 path
def quantize_fp8(x, out=None):
    """Dynamic per-tensor e4m3 quantisation of a bf16 matrix (torchao PerTensor semantics): returns (q, scale) with
    q = e4m3(clamp(x / scale, +-448)) as a torch.float8_e4m3fn tensor and scale = max|x| / 448 as a 1-element fp32 tensor."""
    _gpu(x)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise TypeError("quantize_fp8 expects a K-contiguous bf16 matrix")
    M, d = x.shape
    if out is None:
        out = torch.empty((M, d), dtype=torch.float8_e4m3fn, device=x.device)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    scratch = torch.empty(1, dtype=torch.int32, device=x.device)
    _lib.call("rtv_quantize_fp8", _ptr(x), ctypes.c_int64(x.stride(0)), M, d, _ptr(out), ctypes.c_int64(out.stride(0)),
              _ptr(scale), _ptr(scratch), _stream())
    return out, scale


def gemm_fp8(a_q, a_scale, w_q, w_scale, bias=None, act=ACT_NONE, gate=None, gate_stride=0, rows_per_frame=0,
             residual=None, out=None, row_offset=0):
    """out[M,N] bf16 = epi((a_q @ w_q^T) * a_scale * w_scale): e4m3 operands, fp32 accumulation, rtv_gemm's epilogue."""
    _gpu(a_q, w_q, a_scale, bias, gate, residual, out)
    if a_q.dtype != torch.float8_e4m3fn or w_q.dtype != torch.float8_e4m3fn:
        raise TypeError("gemm_fp8 expects float8_e4m3fn operands")
    M, K = a_q.shape
    N = w_q.shape[0]
    if w_q.shape[1] != K or a_q.stride(1) != 1 or w_q.stride(1) != 1:
        raise ValueError("gemm_fp8 shape / stride mismatch")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a_q.device)
    ensure_gemm_workspace(a_q.device)
    _lib.call("rtv_gemm_fp8", _ptr(a_q), a_q.stride(0), _ptr(w_q), w_q.stride(0), _ptr(a_scale), ctypes.c_float(float(w_scale)),
              _ptr(out), out.stride(0), M, N, K, _ptr(bias), int(act), _ptr(gate), int(gate_stride), int(rows_per_frame),
              int(row_offset), _ptr(residual), residual.stride(0) if residual is not None else 0, _stream())
    return out


# --------------------------------------------------------------------------------------- fp8 path, per-row scales
def quantize_fp8_rows(x, out=None):
    """Dynamic per-row e4m3 quantisation of a bf16 matrix (torchao PerRow semantics, include/rtv_hip_fp8_rows.h): returns
    (q, scales) with q[m] = e4m3(clamp(x[m] / scales[m], +-448)) and scales[m] = max(max|x[m]|, 1e-12) / 448, an fp32 [M] tensor."""
    _gpu(x, out)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise TypeError("quantize_fp8_rows expects a K-contiguous bf16 matrix")
    M, d = x.shape
    if out is None:
        out = torch.empty((M, d), dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty(M, dtype=torch.float32, device=x.device)
    _lib.call("rtv_quantize_fp8_rows", _ptr(x), ctypes.c_int64(x.stride(0)), M, d, _ptr(out), ctypes.c_int64(out.stride(0)),
              _ptr(scales), _stream())
    return out, scales


def layernorm_modulate_fp8_rows(x, eps=1e-6, shift=None, scale=None, frame_stride=0, rows_per_frame=0, weight=None, bias=None,
                                row_offset=0):
    """layernorm_modulate followed by quantize_fp8_rows on its bf16 result, in one kernel and bit for bit: returns (q, scales)."""
    _gpu(x, shift, scale, weight, bias)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or not x.is_contiguous():
        raise TypeError("layernorm_modulate_fp8_rows expects a contiguous bf16 matrix")
    M, d = x.shape
    out = torch.empty((M, d), dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty(M, dtype=torch.float32, device=x.device)
    _lib.call("rtv_layernorm_modulate_fp8_rows", _ptr(x), _ptr(out), ctypes.c_int64(out.stride(0)), _ptr(scales), M, d, float(eps),
              _ptr(shift), _ptr(scale), int(frame_stride), int(rows_per_frame), int(row_offset), _ptr(weight), _ptr(bias), _stream())
    return out, scales


def gemm_fp8_rows(a_q, a_scales, w_q, w_scales, bias=None, act=ACT_NONE, gate=None, gate_stride=0, rows_per_frame=0,
                  residual=None, out=None, row_offset=0):
    """out[M,N] bf16 = epi((a_q @ w_q^T)[m, n] * a_scales[m] * w_scales[n]): gemm_fp8 with one fp32 scale per row of each operand."""
    _gpu(a_q, w_q, a_scales, w_scales, bias, gate, residual, out)
    if a_q.dtype != torch.float8_e4m3fn or w_q.dtype != torch.float8_e4m3fn:
        raise TypeError("gemm_fp8_rows expects float8_e4m3fn operands")
    M, K = a_q.shape
    N = w_q.shape[0]
    if w_q.shape[1] != K or a_q.stride(1) != 1 or w_q.stride(1) != 1:
        raise ValueError("gemm_fp8_rows shape / stride mismatch")
    for s, n in ((a_scales, M), (w_scales, N)):
        if s.dtype != torch.float32 or s.dim() != 1 or s.shape[0] != n or not s.is_contiguous():
            raise ValueError("gemm_fp8_rows expects contiguous fp32 scale vectors of M and N elements")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a_q.device)
    ensure_gemm_workspace(a_q.device)
    _lib.call("rtv_gemm_fp8_rows", _ptr(a_q), a_q.stride(0), _ptr(w_q), w_q.stride(0), _ptr(a_scales), _ptr(w_scales),
              _ptr(out), out.stride(0), M, N, K, _ptr(bias), int(act), _ptr(gate), int(gate_stride), int(rows_per_frame),
              int(row_offset), _ptr(residual), residual.stride(0) if residual is not None else 0, _stream())
    return out


def gemm_w8(a, w_q, w_scales, out=None, transpose_out=False, workspace=None):
    """Weight-only fp8 GEMM at prompt length (include/rtv_hip_t5_w8.h): out bf16 = bf16((a @ value(w_q)^T)[m, n] * w_scales[n])
    for bf16 rows a [M, K] and e4m3 codes w_q [N, K]; out is [M, N], or [N, M] with transpose_out.  The K-split slabs live in
    `workspace` (a uint8 tensor; allocated per call when None)."""
    _gpu(a, w_q, w_scales, out, workspace)
    if a.dtype != torch.bfloat16 or w_q.dtype != torch.float8_e4m3fn or w_scales.dtype != torch.float32:
        raise TypeError("gemm_w8 expects bf16 rows, float8_e4m3fn codes and fp32 scales")
    M, K = a.shape
    N = w_q.shape[0]
    if w_q.shape[1] != K or a.stride(1) != 1 or w_q.stride(1) != 1 or w_scales.shape != (N,) or not w_scales.is_contiguous():
        raise ValueError("gemm_w8 shape / stride mismatch")
    if out is None:
        out = torch.empty((N, M) if transpose_out else (M, N), dtype=torch.bfloat16, device=a.device)
    need = _lib.load().rtv_gemm_w8_workspace_bytes(M, N, K)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=a.device)
    _lib.call("rtv_gemm_w8", _ptr(a), a.stride(0), _ptr(w_q), w_q.stride(0), _ptr(w_scales), _ptr(out), out.stride(0),
              int(bool(transpose_out)), M, N, K, _ptr(workspace), ctypes.c_size_t(workspace.numel() if workspace is not None else 0),
              _stream())
    return out


# ------------------------------------------------------- block-scaled paths (include/rtv_hip_mxfp4.h, include/rtv_hip_mxfp6.h)
class _MxFormat(collections.namedtuple("_MxFormat", "name group_elems group_bytes scale_align k_multiple min_codes")):
    """A block-scaled format: `group_elems` codes fill `group_bytes` bytes, a row's scales are padded to `scale_align` bytes, the
    GEMM takes K % k_multiple == 0; `min_codes` is the spelling of a row's code bytes in messages."""
    block = 32

    def code_bytes(self, k):
        return k // self.group_elems * self.group_bytes

    def scale_bytes(self, k):
        return ((k // self.block) + self.scale_align - 1) & ~(self.scale_align - 1)


_MXFP4 = _MxFormat("mxfp4", 2, 1, 8, 256, "d / 2")
_MXFP6 = _MxFormat("mxfp6", 4, 3, 4, 128, "3 d / 4")
MXFP4_BLOCK = _MXFP4.block
MXFP6_BLOCK = _MXFP6.block


def mxfp4_scale_bytes(k):
    """Bytes a row of k elements owns in a scales array (RTV_MXFP4_SCALE_BYTES)."""
    return _MXFP4.scale_bytes(k)


def mxfp6_scale_bytes(k):
    """Bytes a row of k elements owns in a scales array (RTV_MXFP6_SCALE_BYTES)."""
    return _MXFP6.scale_bytes(k)


def mxfp6_code_bytes(k):
    """Bytes a row of k elements owns in a codes array (RTV_MXFP6_CODE_BYTES)."""
    return _MXFP6.code_bytes(k)


def _mx_out(fmt, M, d, device, codes, scales):
    if codes is None:
        codes = torch.empty((M, fmt.code_bytes(d)), dtype=torch.uint8, device=device)
    if scales is None:
        # (zero-filled: a row whose last K-tile is short owns bytes the kernel never writes)
        scales = torch.zeros((M, fmt.scale_bytes(d)), dtype=torch.uint8, device=device)
    for t in (codes, scales):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] != M or t.stride(1) != 1:
            raise TypeError(f"{fmt.name}: codes and scales are uint8 matrices of M rows with contiguous rows")
    if codes.shape[1] != fmt.code_bytes(d) or scales.shape[1] != fmt.scale_bytes(d):
        raise ValueError(f"{fmt.name}: codes must be [M, {fmt.min_codes}] and scales [M, RTV_{fmt.name.upper()}_SCALE_BYTES(d)]")
    return codes, scales


MX_ROT_ACT_SHIFT, MX_ROT_WEIGHT_SHIFT = _lib.MX_ROT_ACT_SHIFT, _lib.MX_ROT_WEIGHT_SHIFT   # include/rtv_hip_mx_rotate.h


def _quantize_mx(fmt, x, codes, scales, rotate_shift=None):
    _gpu(x, codes, scales)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise TypeError(f"quantize_{fmt.name} expects a K-contiguous bf16 matrix")
    M, d = x.shape
    if d % fmt.block:
        raise ValueError(f"quantize_{fmt.name}: d must be a multiple of 32")
    if rotate_shift is not None and not 0 <= int(rotate_shift) <= _lib.MX_ROT_MAX_SHIFT:
        raise ValueError(f"quantize_{fmt.name}: rotate_shift must be in 0 .. {_lib.MX_ROT_MAX_SHIFT}")
    codes, scales = _mx_out(fmt, M, d, x.device, codes, scales)
    rot = () if rotate_shift is None else (int(rotate_shift),)
    _lib.call("rtv_quantize_" + fmt.name + ("_rot" if rot else ""), _ptr(x), ctypes.c_int64(x.stride(0)), M, d, _ptr(codes),
              ctypes.c_int64(codes.stride(0)), _ptr(scales), ctypes.c_int64(scales.stride(0)), *rot, _stream())
    return codes, scales


def _layernorm_modulate_mx(fmt, x, eps, shift, scale, frame_stride, rows_per_frame, weight, bias, row_offset, rotate=False):
    _gpu(x, shift, scale, weight, bias)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or not x.is_contiguous():
        raise TypeError(f"layernorm_modulate_{fmt.name} expects a contiguous bf16 matrix")
    M, d = x.shape
    if d % fmt.block:
        raise ValueError(f"layernorm_modulate_{fmt.name}: d must be a multiple of 32")
    codes, scales = _mx_out(fmt, M, d, x.device, None, None)
    _lib.call("rtv_layernorm_modulate_" + fmt.name + ("_rot" if rotate else ""), _ptr(x), _ptr(codes), ctypes.c_int64(codes.stride(0)), _ptr(scales),
              ctypes.c_int64(scales.stride(0)), M, d, float(eps), _ptr(shift), _ptr(scale), int(frame_stride), int(rows_per_frame),
              int(row_offset), _ptr(weight), _ptr(bias), _stream())
    return codes, scales


def _gate_in_bounds(gate, gate_stride, rows_per_frame, row_offset, M, N):
    """The epilogue reads gate[((row_offset + m) // rows_per_frame) * gate_stride + n] for every row m < M and has no way to know
    where the caller's table ends.  A table that ends in front of the last frame the rows address (a row offset that moves the last
    rows past the last frame) would be read past its allocation: it is handed over in a copy that continues with zeros, so those
    rows get a gate of 0.  A table that covers its rows - every call of the model - is passed as it is."""
    if gate is None or int(rows_per_frame) <= 0:
        return gate
    need = ((int(row_offset) + M - 1) // int(rows_per_frame)) * int(gate_stride) + N
    have = gate.untyped_storage().nbytes() // gate.element_size() - gate.storage_offset()
    if have >= need:
        return gate
    padded = torch.zeros(need, dtype=gate.dtype, device=gate.device)
    padded[:have] = torch.as_strided(gate, (have,), (1,))
    return padded


def _gemm_mx(fmt, a_codes, a_scales, w_codes, w_scales, bias, act, gate, gate_stride, rows_per_frame, residual, out, row_offset):
    who = "gemm_" + fmt.name
    _gpu(a_codes, w_codes, a_scales, w_scales, bias, gate, residual, out)
    for t in (a_codes, w_codes, a_scales, w_scales):
        if t.dtype != torch.uint8 or t.dim() != 2:
            raise TypeError(f"{who} expects uint8 code and scale matrices")
    if a_codes.shape[1] % fmt.group_bytes:
        raise ValueError(f"{who}: a row of codes is {fmt.min_codes.replace('d', 'K')} bytes")
    M, K = a_codes.shape[0], a_codes.shape[1] // fmt.group_bytes * fmt.group_elems
    N = w_codes.shape[0]
    if w_codes.shape[1] != a_codes.shape[1] or a_codes.stride(1) != 1 or w_codes.stride(1) != 1:
        raise ValueError(f"{who} shape / stride mismatch")
    if K % fmt.k_multiple:
        raise ValueError(f"{who}: K must be a multiple of {fmt.k_multiple}")
    for s_, n in ((a_scales, M), (w_scales, N)):
        if tuple(s_.shape) != (n, K // fmt.block) or not s_.is_contiguous():
            raise ValueError(f"{who} expects contiguous scale matrices [rows, K / 32]")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a_codes.device)
    ensure_gemm_workspace(a_codes.device)
    gate = _gate_in_bounds(gate, gate_stride, rows_per_frame, row_offset, M, N)
    _lib.call("rtv_" + who, _ptr(a_codes), a_codes.stride(0), _ptr(w_codes), w_codes.stride(0), _ptr(a_scales), _ptr(w_scales),
              _ptr(out), out.stride(0), M, N, K, _ptr(bias), int(act), _ptr(gate), int(gate_stride), int(rows_per_frame),
              int(row_offset), _ptr(residual), residual.stride(0) if residual is not None else 0, _stream())
    return out


def quantize_mxfp4(x, codes=None, scales=None, rotate_shift=None):
    """MXFP4 quantisation of a bf16 matrix [M, d], d % 32 == 0: returns (codes, scales), uint8 [M, d / 2] (two e2m1 codes per
    byte, element 2j in the low nibble) and uint8 [M, RTV_MXFP4_SCALE_BYTES(d)] (e8m0 block scales in the header's order).
    rotate_shift (None: no rotation): each block of 32 goes through the Hadamard butterflies of include/rtv_hip_mx_rotate.h and is
    scaled by 2^-rotate_shift first (MX_ROT_ACT_SHIFT for activations, MX_ROT_WEIGHT_SHIFT for weights)."""
    return _quantize_mx(_MXFP4, x, codes, scales, rotate_shift)


def quantize_mxfp6(x, codes=None, scales=None, rotate_shift=None):
    """MXFP6 quantisation of a bf16 matrix [M, d], d % 32 == 0: returns (codes, scales), uint8 [M, 3 d / 4] (e2m3 codes, a block of
    32 in 24 bytes, element j at bits [6 j, 6 j + 6)) and uint8 [M, RTV_MXFP6_SCALE_BYTES(d)] (e8m0 block scales in the header's
    order).  rotate_shift: as for quantize_mxfp4."""
    return _quantize_mx(_MXFP6, x, codes, scales, rotate_shift)


def layernorm_modulate_mxfp4(x, eps=1e-6, shift=None, scale=None, frame_stride=0, rows_per_frame=0, weight=None, bias=None,
                             row_offset=0):
    """layernorm_modulate followed by quantize_mxfp4 on its bf16 result, in one kernel and bit for bit: returns (codes, scales)."""
    return _layernorm_modulate_mx(_MXFP4, x, eps, shift, scale, frame_stride, rows_per_frame, weight, bias, row_offset)


def layernorm_modulate_mxfp6(x, eps=1e-6, shift=None, scale=None, frame_stride=0, rows_per_frame=0, weight=None, bias=None,
                             row_offset=0):
    """layernorm_modulate followed by quantize_mxfp6 on its bf16 result, in one kernel and bit for bit: returns (codes, scales)."""
    return _layernorm_modulate_mx(_MXFP6, x, eps, shift, scale, frame_stride, rows_per_frame, weight, bias, row_offset)


def layernorm_modulate_mxfp4_rot(x, eps=1e-6, shift=None, scale=None, frame_stride=0, rows_per_frame=0, weight=None, bias=None,
                                 row_offset=0):
    """layernorm_modulate followed by quantize_mxfp4(rotate_shift=MX_ROT_ACT_SHIFT) on its bf16 result, in one kernel and bit for
    bit: returns (codes, scales)."""
    return _layernorm_modulate_mx(_MXFP4, x, eps, shift, scale, frame_stride, rows_per_frame, weight, bias, row_offset, rotate=True)


def layernorm_modulate_mxfp6_rot(x, eps=1e-6, shift=None, scale=None, frame_stride=0, rows_per_frame=0, weight=None, bias=None,
                                 row_offset=0):
    """layernorm_modulate followed by quantize_mxfp6(rotate_shift=MX_ROT_ACT_SHIFT) on its bf16 result, in one kernel and bit for
    bit: returns (codes, scales)."""
    return _layernorm_modulate_mx(_MXFP6, x, eps, shift, scale, frame_stride, rows_per_frame, weight, bias, row_offset, rotate=True)


def gemm_mxfp4(a_codes, a_scales, w_codes, w_scales, bias=None, act=ACT_NONE, gate=None, gate_stride=0, rows_per_frame=0,
               residual=None, out=None, row_offset=0):
    """out[M,N] bf16 = epi(sum over 32-blocks of 2^(ea + ew) * (a . w^T)): uint8 code matrices [M, K / 2] and [N, K / 2], uint8
    block scales [M, K / 32] and [N, K / 32] with dense rows, fp32 accumulation, rtv_gemm's epilogue.  K % 256 == 0."""
    return _gemm_mx(_MXFP4, a_codes, a_scales, w_codes, w_scales, bias, act, gate, gate_stride, rows_per_frame, residual, out, row_offset)


def gemm_mxfp6(a_codes, a_scales, w_codes, w_scales, bias=None, act=ACT_NONE, gate=None, gate_stride=0, rows_per_frame=0,
               residual=None, out=None, row_offset=0):
    """out[M,N] bf16 = epi(sum over 32-blocks of 2^(ea + ew) * (a . w^T)): uint8 code matrices [M, 3 K / 4] and [N, 3 K / 4], uint8
    block scales [M, K / 32] and [N, K / 32] with dense rows, fp32 accumulation, rtv_gemm's epilogue.  K % 128 == 0."""
    return _gemm_mx(_MXFP6, a_codes, a_scales, w_codes, w_scales, bias, act, gate, gate_stride, rows_per_frame, residual, out, row_offset)


# --------------------------------------------------------------------------------------- norms
def layernorm_modulate(x, eps=1e-6, shift=None, scale=None, frame_stride=0, rows_per_frame=0,
                       weight=None, bias=None, out=None, row_offset=0):
    """LN(x) [* (1+scale[f]) + shift[f]]  or affine LN.  x:[M,d] bf16."""
    _gpu(x, shift, scale, weight, bias)
    M, d = x.shape
    if out is None:
        out = torch.empty_like(x)
    _lib.call("rtv_layernorm_modulate", _ptr(x), _ptr(out), M, d, float(eps), _ptr(shift), _ptr(scale),
              int(frame_stride), int(rows_per_frame), int(row_offset), _ptr(weight), _ptr(bias), _stream())
    return out


def rmsnorm(x, weight, eps=1e-6, out=None):
    _gpu(x, weight)
    M, d = x.shape
    if out is None:
        out = torch.empty((M, d), dtype=x.dtype, device=x.device)
    _lib.call("rtv_rmsnorm", _ptr(x), x.stride(0), _ptr(out), out.stride(0), M, d, float(eps), _ptr(weight),
              _stream())
    return out


def qk_norm_rope_cache(qkv, k_cache, v_cache, cache_row0, num_heads, wq, wk, rope_cs, grid, start_frame,
                       eps=1e-6, q_out=None, row_offset=0, ring=(0, 0, 0)):
    """qkv:[M,3d]; k_cache/v_cache:[kv_size,H,hd] views (row stride = stride(0)); grid=(F,gh,gw).
    ring = (ring_lo, ring_size, ring_shift): logical row r >= ring_lo is stored at ring_lo + (r - ring_lo + ring_shift) % ring_size."""
    _gpu(qkv, k_cache, v_cache, wq, wk, rope_cs)
    M, d3 = qkv.shape
    d = d3 // 3
    F, gh, gw = grid
    if q_out is None:
        q_out = torch.empty((M, d), dtype=qkv.dtype, device=qkv.device)
    if cache_row0 + row_offset + M > k_cache.shape[0]:
        raise ValueError("KV-cache write out of range")
    _lib.call("rtv_qk_norm_rope_cache_ring", _ptr(qkv), _ptr(q_out), _ptr(k_cache), _ptr(v_cache),
              k_cache.stride(0), int(cache_row0), M, d, int(num_heads), float(eps), _ptr(wq), _ptr(wk),
              _ptr(rope_cs), int(F), int(gh), int(gw), int(start_frame), int(row_offset),
              int(ring[0]), int(ring[1]), int(ring[2]), _stream())
    return q_out


def modulation_table(modulation, e0, out=None):
    """modulation:[L,J,d], e0:[F,J0,d] -> [L,F,J,d] = bf16(modulation + e0)."""
    _gpu(modulation, e0)
    L, J, d = modulation.shape
    F, J0, _ = e0.shape
    if out is None:
        out = torch.empty((L, F, J, d), dtype=modulation.dtype, device=modulation.device)
    _lib.call("rtv_modulation_table", _ptr(modulation), _ptr(e0), _ptr(out), L, F, J, J0, d, _stream())
    return out


def sinusoidal_embedding(t, dim):
    _gpu(t)
    t = t.to(torch.float32).contiguous()
    out = torch.empty((t.numel(), dim), dtype=torch.bfloat16, device=t.device)
    _lib.call("rtv_sinusoidal_embedding", _ptr(t), _ptr(out), t.numel(), int(dim), _stream())
    return out


def patchify(x, gh, gw):
    """x:[C,F,2gh,2gw] -> [F*gh*gw, C*4]"""
    _gpu(x)
    C, F = x.shape[0], x.shape[1]
    x = x.contiguous()
    out = torch.empty((F * gh * gw, C * 4), dtype=x.dtype, device=x.device)
    _lib.call("rtv_patchify", _ptr(x), _ptr(out), C, F, gh, gw, _stream())
    return out


def unpatchify(rows, C, F, gh, gw):
    _gpu(rows)
    rows = rows.contiguous()
    out = torch.empty((C, F, 2 * gh, 2 * gw), dtype=rows.dtype, device=rows.device)
    _lib.call("rtv_unpatchify", _ptr(rows), _ptr(out), C, F, gh, gw, _stream())
    return out


_T_KIND = {torch.float32: 0, torch.float64: 1, torch.int64: 2}


def _frame_view(x, what):
    """[F, C, h, w] (any frame / channel strides, contiguous h*w plane) -> (tensor, frame stride, channel stride)."""
    if x.dtype != torch.bfloat16:
        raise NotImplementedError(f"scheduler_step: {what} must be bf16 (the reference's inference dtype), got {x.dtype}")
    F, C, h, w = x.shape
    if w > 1 and x.stride(3) != 1 or h > 1 and x.stride(2) != w:
        x = x.contiguous()
    return x, x.stride(0), x.stride(1)


def scheduler_step(timesteps, sigmas, flow=None, xt=None, t=None, x0=None, noise=None, t_next=None):
    """One launch of the flow-matching step arithmetic (include/rtv_hip.h: rtv_scheduler_step) on [F, C, h, w] latents.
    flow/xt/t -> x0 (wan_wrapper.py:181-205); x0 (computed or given)/noise/t_next -> noisy (scheduler.py:159-176).
    Returns (x0, noisy or None)."""
    src = flow if flow is not None else x0
    _gpu(src, timesteps, sigmas)
    F, C, h, w = src.shape
    if timesteps.dtype != torch.float32 or sigmas.dtype != torch.float32 or timesteps.numel() != sigmas.numel():
        raise ValueError("scheduler_step: timesteps / sigmas must be float32 tables of one length")
    tk = None
    for tt in (t, t_next):
        if tt is not None:
            _gpu(tt)
            if tt.dtype not in _T_KIND or tt.numel() != F or not tt.is_contiguous():
                raise ValueError(f"scheduler_step: timestep must be a contiguous [F] float32/float64/int64 tensor, got "
                                 f"{tt.dtype} {tuple(tt.shape)}")
            if tk is not None and tk != _T_KIND[tt.dtype]:
                raise ValueError("scheduler_step: t and t_next must share a dtype")
            tk = _T_KIND[tt.dtype]
    fs = fc = xs = xc = 0
    if flow is not None:
        _gpu(xt)
        if xt.shape != flow.shape:
            raise ValueError(f"scheduler_step: flow {tuple(flow.shape)} vs xt {tuple(xt.shape)}")
        flow, fs, fc = _frame_view(flow, "flow")
        xt, xs, xc = _frame_view(xt, "xt")
        x0 = torch.empty((F, C, h, w), dtype=torch.bfloat16, device=src.device)
    else:
        if x0.dtype != torch.bfloat16:
            raise NotImplementedError("scheduler_step: x0 must be bf16")
        x0 = x0.contiguous()
    noisy = None
    if t_next is not None:
        _gpu(noise)
        if noise.dtype != torch.bfloat16 or noise.shape != x0.shape:
            raise ValueError("scheduler_step: noise must be bf16 of the latent shape")
        noise = noise.contiguous()
        noisy = torch.empty_like(x0)
    _lib.call("rtv_scheduler_step", _ptr(flow) if flow is not None else None, fs, fc,
              _ptr(xt) if flow is not None else None, xs, xc, _ptr(t) if t is not None else None,
              _ptr(t_next) if t_next is not None else None, tk if tk is not None else 0,
              _ptr(timesteps), _ptr(sigmas), timesteps.numel(), _ptr(x0),
              _ptr(noise) if noise is not None else None, _ptr(noisy) if noisy is not None else None,
              F, C, h * w, _stream())
    return x0, noisy


def pixels_to_rgb8(pixels, out=None):
    """Decoder pixels float32 [..., 3, H, W] in [-1, 1] -> uint8 [..., H, W, 3] (rtv_pixels_to_rgb8): the reference's
    host-side normalisation + to_pil_image byte conversion (release_server.py:984, :972) done on the GPU."""
    _gpu(pixels)
    if pixels.dtype != torch.float32 or pixels.shape[-3] != 3 or not pixels.is_contiguous():
        raise ValueError("pixels_to_rgb8 expects contiguous float32 [..., 3, H, W]")
    H, W = pixels.shape[-2:]
    T = pixels.numel() // (3 * H * W)
    shape = tuple(pixels.shape[:-3]) + (H, W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=pixels.device)
    elif out.shape != shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("pixels_to_rgb8: out must be contiguous uint8 [..., H, W, 3]")
    _lib.call("rtv_pixels_to_rgb8", _ptr(pixels), _ptr(out), T, H, W, _stream())
    return out


def frames_from_rgb8(rgb8, size, out=None, slots=None):
    """Camera / decoder bytes uint8 [N, Hin, Win, 3] -> the VAE encoder's input, float16 [3, T, h, w] in [-1, 1]
    (rtv_frames_from_rgb8): the reference's push_frame arithmetic (release_server.py:479-481) and, when (Hin, Win) != size,
    the bicubic resize of encode_video_latent (v2v.py:153), one launch per 16 frames.  `slots`: the T frames to take, as indices
    into N (a ring of frame slots; default all N in order)."""
    _gpu(rgb8)
    if rgb8.dtype != torch.uint8 or rgb8.dim() != 4 or rgb8.shape[-1] != 3 or not rgb8.is_contiguous():
        raise ValueError("frames_from_rgb8 expects contiguous uint8 [T, Hin, Win, 3]")
    N, Hin, Win = rgb8.shape[:3]
    h, w = int(size[0]), int(size[1])
    slots = list(range(N)) if slots is None else [int(i) for i in slots]
    if any(not 0 <= i < N for i in slots):
        raise IndexError(f"frames_from_rgb8: slot outside the {N} frames")
    T = len(slots)
    if out is None:
        out = torch.empty((3, T, h, w), dtype=torch.float16, device=rgb8.device)
    elif out.shape != (3, T, h, w) or out.dtype != torch.float16 or not out.is_contiguous() or out.device != rgb8.device:
        raise ValueError("frames_from_rgb8: out must be contiguous float16 [3, T, h, w] on the frames' device")
    for t0 in range(0, T, _lib.FRAMES_MAX):
        part = slots[t0:t0 + _lib.FRAMES_MAX]
        _lib.call("rtv_frames_from_rgb8", _ptr(rgb8), (ctypes.c_int * len(part))(*part), Hin * Win * 3, len(part), Hin, Win,
                  _ptr(out), T, t0, h, w, _stream())
    return out


# ------------------------------------------------------------------------------------ JPEG frame encoder (include/rtv_hip_jpeg.h)
def jpeg_header(quality, H, W):
    """Everything of the JPEG file in front of the entropy-coded data, SOI .. SOS (rtv_jpeg_header; host only, no GPU call)."""
    buf = ctypes.create_string_buffer(1024)
    n = _lib.load().rtv_jpeg_header(int(quality), int(H), int(W), buf, len(buf))
    if n == 0:
        _lib.check(-1, "rtv_jpeg_header")
    return buf.raw[:n]


def _jpeg_input(x, what):
    """-> (contiguous tensor, pixels_are_rgb8, T, H, W) for float32 [..., 3, H, W] or uint8 [..., H, W, 3]."""
    _gpu(x)
    if x.dtype == torch.float32 and x.dim() >= 3 and x.shape[-3] == 3 and x.is_contiguous():
        H, W = x.shape[-2:]
        return x, 0, x.numel() // (3 * H * W), H, W
    if x.dtype == torch.uint8 and x.dim() >= 3 and x.shape[-1] == 3 and x.is_contiguous():
        H, W = x.shape[-3:-1]
        return x, 1, x.numel() // (3 * H * W), H, W
    raise ValueError(f"{what} expects contiguous float32 [..., 3, H, W] in [-1, 1] or uint8 [..., H, W, 3]")


def _jpeg_arena(T, H, W, device, arena):
    need = jpeg_arena_bytes(T, H, W)
    if arena is None:
        # sizes the entry point refuses give 0: it is called all the same, for its message
        arena = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    elif arena.dtype != torch.uint8 or not arena.is_contiguous() or arena.device != device:
        raise ValueError("arena must be a contiguous uint8 tensor on the pixels' device")
    return arena


def jpeg_arena_bytes(T, H, W):
    """Bytes of device scratch one jpeg_encode / jpeg_coefficients call of T frames needs (rtv_jpeg_arena_bytes); 0 = refused."""
    return _lib.load().rtv_jpeg_arena_bytes(int(T), int(H), int(W))


def jpeg_out_bound(T, H, W):
    """Bytes an `out` buffer of T frames can never exceed (rtv_jpeg_out_bound); real frames take a few percent of it."""
    return _lib.load().rtv_jpeg_out_bound(int(T), int(H), int(W))


def jpeg_encode(pixels, quality=90, out=None, offsets=None, arena=None):
    """Decoder pixels float32 [T, 3, H, W] in [-1, 1], or rgb8 uint8 [T, H, W, 3] -> (uint8 device buffer, int64 device
    offsets [T + 1]): T complete baseline JPEG files back to back, file t = buffer[offsets[t]:offsets[t + 1]]
    (rtv_jpeg_encode; three launches on the current stream).

    With `out` (uint8, its numel is the capacity) nothing synchronises: nothing is written beyond it, the offsets hold the true
    sizes, and offsets[T] > out.numel() means the files are truncated.  Without it the call reads the total back (one
    synchronisation), encodes again if one byte per pixel did not suffice, and returns a buffer of exactly the total."""
    pixels, rgb8, T, H, W = _jpeg_input(pixels, "jpeg_encode")
    dev = pixels.device
    arena = _jpeg_arena(T, H, W, dev, arena)
    if offsets is None:
        offsets = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    elif offsets.dtype != torch.int64 or offsets.numel() != T + 1 or not offsets.is_contiguous() or offsets.device != dev:
        raise ValueError("jpeg_encode: offsets must be contiguous int64 [T + 1] on the pixels' device")
    if out is not None and (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev):
        raise ValueError("jpeg_encode: out must be a contiguous uint8 tensor on the pixels' device")

    def run(buf):
        _lib.call("rtv_jpeg_encode", _ptr(pixels), rgb8, T, H, W, int(quality), _ptr(arena), arena.numel(), _ptr(buf), buf.numel(),
                  _ptr(offsets), _stream())
    if out is not None:
        run(out)
        return out, offsets
    out = torch.empty(T * (H * W + 1024), dtype=torch.uint8, device=dev)
    run(out)
    total = int(offsets[-1]) if T else 0
    if total > out.numel():
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        run(out)
    return out[:total], offsets


def jpeg_coefficients(pixels, quality=90, arena=None):
    """The encoder's first stage alone (rtv_jpeg_coefficients, a unit-test hook): quantised DCT coefficients int16
    [T, mcu_rows, mcus, 6, 64] - the six blocks of an MCU as Y00 Y01 Y10 Y11 Cb Cr, each in zigzag order."""
    pixels, rgb8, T, H, W = _jpeg_input(pixels, "jpeg_coefficients")
    arena = _jpeg_arena(T, H, W, pixels.device, arena)
    out = torch.empty((T, (H + 15) // 16, (W + 15) // 16, 6, 64), dtype=torch.int16, device=pixels.device)
    _lib.call("rtv_jpeg_coefficients", _ptr(pixels), rgb8, T, H, W, int(quality), _ptr(arena), arena.numel(), _ptr(out), _stream())
    return out


# ----------------------------------------------------------------------------- JPEG frame decoder (include/rtv_hip_jpeg_decode.h)
JPEG_DESC_BYTES = ctypes.sizeof(_lib.JPEGDEC_STRUCTS["rtv_jpeg_desc"])


class JpegInfo:
    """What jpeg_parse makes of a file's marker segments: H, W, components (1 or 3), sampling (luma blocks per MCU, horizontal x
    vertical), restart_interval (MCUs, 0 = none), file_bytes, and `desc`, the rtv_jpeg_desc the decode calls take; `packed()` is
    its bytes, which go in front of the file's bytes on the device."""

    def __init__(self, desc):
        self.desc = desc
        self.H, self.W, self.components = desc.height, desc.width, desc.components
        self.sampling = (desc.hsamp, desc.vsamp)
        self.restart_interval, self.file_bytes = desc.restart_interval, desc.file_bytes

    def packed(self):
        return ctypes.string_at(ctypes.byref(self.desc), JPEG_DESC_BYTES)


def _jpeg_bytes(data, what):
    if isinstance(data, (bytearray, memoryview)):
        data = bytes(data)
    if not isinstance(data, bytes):
        raise TypeError(f"{what} expects a JPEG file as bytes, bytearray or memoryview, not {type(data).__name__}")
    return data


def jpeg_parse(data):
    """A JPEG file (bytes-like) -> JpegInfo (rtv_jpeg_parse; host only, no GPU call).  ValueError with the reason for a file
    outside what the decoder accepts - progressive, CMYK, 12 bit, other sampling, a missing table, a cut header, above the caps:
    a server can hand that one frame to PIL and push its pixels instead."""
    data = _jpeg_bytes(data, "jpeg_parse")
    lib = _lib.load()
    desc = _lib.JPEGDEC_STRUCTS["rtv_jpeg_desc"]()
    if lib.rtv_jpeg_parse(data, len(data), ctypes.byref(desc)) != 0:
        raise ValueError(lib.rtv_last_error().decode("utf-8", "replace"))
    return JpegInfo(desc)


def jpeg_decode_arena_bytes(infos):
    """Bytes of device scratch one jpeg_decode call of these frames needs (rtv_jpeg_decode_arena_bytes); 0 = refused."""
    descs = (_lib.JPEGDEC_STRUCTS["rtv_jpeg_desc"] * max(len(infos), 1))(*[i.desc for i in infos])
    return _lib.load().rtv_jpeg_decode_arena_bytes(descs, len(infos))


def jpeg_decode_frames(infos, frames, outs, status, arena, rounds=None, subseq_bits=0):
    """The call itself (rtv_jpeg_decode, two launches on the current stream): infos [T] JpegInfo; frames [T] uint8 CUDA tensors,
    each a frame's descriptor plus file (16-byte aligned); outs [T] uint8 [H, W, 3] CUDA tensors; status int32 [T]; arena uint8;
    rounds int32 [T] or None.  Nothing is allocated and nothing synchronises."""
    T = len(infos)
    if not (len(frames) == len(outs) == T) or T > _lib.FRAMES_MAX:
        raise ValueError(f"jpeg_decode: as many frames as outputs, at most {_lib.FRAMES_MAX} per call")
    _gpu(status, arena, rounds, *frames, *outs)
    for info, f, o in zip(infos, frames, outs):
        if f.dtype != torch.uint8 or not f.is_contiguous() or f.numel() < JPEG_DESC_BYTES + info.file_bytes:
            raise ValueError("jpeg_decode: a frame must be a contiguous uint8 tensor of descriptor plus file")
        if o.dtype != torch.uint8 or tuple(o.shape) != (info.H, info.W, 3) or not o.is_contiguous():
            raise ValueError("jpeg_decode: an output must be contiguous uint8 [H, W, 3] of the file's size")
    if status.dtype != torch.int32 or status.numel() < T or not status.is_contiguous():
        raise ValueError("jpeg_decode: status must be contiguous int32 [T]")
    if rounds is not None and (rounds.dtype != torch.int32 or rounds.numel() < T or not rounds.is_contiguous()):
        raise ValueError("jpeg_decode: rounds must be contiguous int32 [T]")
    if arena.dtype != torch.uint8 or not arena.is_contiguous():
        raise ValueError("jpeg_decode: arena must be a contiguous uint8 tensor")
    descs = (_lib.JPEGDEC_STRUCTS["rtv_jpeg_desc"] * T)(*[i.desc for i in infos])
    fp = (ctypes.c_void_p * T)(*[f.data_ptr() for f in frames])
    op = (ctypes.c_void_p * T)(*[o.data_ptr() for o in outs])
    _lib.call("rtv_jpeg_decode", descs, fp, op, T, int(subseq_bits), _ptr(arena), arena.numel(), _ptr(status), _ptr(rounds), _stream())


def _jpeg_upload(file, device, what):
    """bytes-like -> (JpegInfo, uint8 CUDA tensor of descriptor plus file)."""
    if torch.is_tensor(file):
        _gpu(file)
        raise TypeError(f"{what} expects JPEG files as bytes-like objects")
    data = _jpeg_bytes(file, what)
    info = jpeg_parse(data)
    host = torch.frombuffer(bytearray(info.packed() + data), dtype=torch.uint8)
    return info, host.to(device)


def jpeg_decode(files, out=None, status=None, arena=None, subseq_bits=0, device="cuda"):
    """JPEG files (a list of bytes-like objects, which may differ in size and sampling) -> (list of uint8 [H, W, 3] CUDA tensors,
    int32 status tensor [T], 0 = clean, else RTV_JPEG_STATUS_* bits): PIL's `Image.open(...).convert("RGB")` pixels, decoded on
    the device (rtv_jpeg_decode).  ValueError for a file the parser refuses.  `out`: a list of output tensors to fill."""
    files = list(files)
    pairs = [_jpeg_upload(f, device, "jpeg_decode") for f in files]
    infos, frames = [p[0] for p in pairs], [p[1] for p in pairs]
    dev = frames[0].device if frames else torch.device(device)
    if out is None:
        out = [torch.empty((i.H, i.W, 3), dtype=torch.uint8, device=dev) for i in infos]
    if status is None:
        status = torch.zeros(len(files), dtype=torch.int32, device=dev)
    for t0 in range(0, len(files), _lib.FRAMES_MAX):
        part = slice(t0, t0 + _lib.FRAMES_MAX)
        need = jpeg_decode_arena_bytes(infos[part])
        a = arena if arena is not None else torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        jpeg_decode_frames(infos[part], frames[part], out[part], status[part], a, subseq_bits=subseq_bits)
    return out, status


def jpeg_decode_coefficients(file, subseq_bits=0, device="cuda"):
    """The decoder's entropy stage alone (rtv_jpeg_decode_coefficients, a unit-test hook) -> (one int16 tensor [block_rows,
    block_cols, 64] per component: the quantised coefficients in natural order over the padded block grid; status int32 [1];
    rounds int32 [1], the synchronisation rounds taken).  subseq_bits: bits of the scan per thread, 0 = the default."""
    info, frame = _jpeg_upload(file, device, "jpeg_decode_coefficients")
    need = jpeg_decode_arena_bytes([info])
    d = info.desc
    shapes = [(d.mcu_rows * (d.vsamp if c == 0 else 1), d.mcu_cols * (d.hsamp if c == 0 else 1), 64) for c in range(d.components)]
    n = sum(s[0] * s[1] * 64 for s in shapes)
    arena = torch.empty(max(need, 16), dtype=torch.uint8, device=frame.device)
    flat = torch.empty(n, dtype=torch.int16, device=frame.device)
    status = torch.zeros(1, dtype=torch.int32, device=frame.device)
    rounds = torch.zeros(1, dtype=torch.int32, device=frame.device)
    _lib.call("rtv_jpeg_decode_coefficients", ctypes.byref(d), _ptr(frame), int(subseq_bits), _ptr(arena), arena.numel(), _ptr(flat),
              _ptr(status), _ptr(rounds), _stream())
    out, at = [], 0
    for s in shapes:
        out.append(flat[at:at + s[0] * s[1] * 64].view(s))
        at += s[0] * s[1] * 64
    return out, status, rounds
