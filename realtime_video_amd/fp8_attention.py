"""The state of opt-in fp8 self-attention (CausalWanModel.enable_fp8_attention; include/rtv_hip_attn_fp8*.h), held by the model as
`model._fp8_attention`: the mode, the running maxima, the K centres, the e4m3 shadows of the cache dicts, and what a forward needs
of all that (`plan`).  The model's public methods delegate here and carry the documentation of the modes; the context-parallel
phase calls stay in CausalWanModel._forward_inference.

One place each for: the `amax` table (`_amax_table`), the centre buffers and their workspace (`alloc_centers`), the
rtv_attn_fp8_shadow struct with its pointer arrays (`_struct`), the "fp8_filled" state of a cache dict (`_fill_state`) and the
choice of the forward's entry point and graph key (`plan`, `_ENTRY`)."""
import collections
import ctypes
import math

import torch

from . import _lib, ops

c_vp = ctypes.c_void_p
_Fp8Shadow = _lib.ATTN_FP8_STRUCTS["rtv_attn_fp8_shadow"]

# What enable_fp8_attention() set: the scales, the epoch of the call (bumps at every enable / disable: a shadow filled before it is
# refilled from the bf16 cache), smooth in (False, True, "codes"), context_parallel in (False, True, "codes") (True: sharded forwards
# run in fp8 instead of raising; "codes": the compact cache under the row exchange, the exchange carrying the e4m3 codes) and only
# (bf16_cache=False: the e4m3 arrays are the whole KV cache).
Mode = collections.namedtuple("Mode", ["k_scale", "v_scale", "epoch", "smooth", "context_parallel", "only"])

# What _forward_inference takes from plan(): the shadow (None: bf16 attention; a list under the head exchange: one per local rank),
# what must stay alive with it, the unsharded forward's entry point followed by its extra arguments, the fp8 part of the graph key,
# and the commit hook of the compact cache (None: nothing to record).
Plan = collections.namedtuple("Plan", ["shadow", "keep", "forward", "key", "commit"])

# What stays alive with a shadow: the struct (or structs), the pointer arrays it refers to, and the centre table of the centred forwards.
Keep = collections.namedtuple("Keep", ["shadow", "arrays", "centers"])

# the unsharded forward per (only, smooth); the centred ones take the centre table behind the shadow
_ENTRY = {(False, False): "rtv_dit_forward_attn_fp8", (False, True): "rtv_dit_forward_attn_fp8_centered",
          (True, False): "rtv_dit_forward_attn_fp8_only", (True, "codes"): "rtv_dit_forward_attn_fp8_only_centered"}


def kv_cache_rows(cache):
    """Rows of one layer's KV cache dict, of either kind: the bf16 cache {"k", "v", ...} (with or without its e4m3 shadow) or the
    compact e4m3-only one {"k8", "v8t", "rows", ...} of enable_fp8_attention(bf16_cache=False)."""
    return cache["k"].shape[1] if "k" in cache else int(cache["rows"])


class Fp8Attention:
    def __init__(self, model):
        self.model = model
        self.mode = None            # a Mode while enable_fp8_attention() is on
        self.prev = None            # the Mode an enable call replaced: convert_kv_cache looks at it
        self.epoch = 0
        self.amax = None            # float32 [num_layers, 2], allocated once
        self.center = None          # float32 [num_layers, H, 128], zero-filled, allocated once; recenter() / set_centers() write it
        self.center_new = None      # smooth "codes": the second centre buffer a recentre computes into, allocated with the first
        self.center_ws = None       # workspace of the mean kernels, allocated with the centre
        self.kv8 = {}               # context_parallel="codes": (M, world, device) -> the staging buffer of the code exchange
        self.center_epoch = 0       # bumps at every recentre: part of a shadow's "fp8_filled" state, like the scales

    # ------------------------------------------------------------------ the mode
    def enable(self, k_scale, v_scale, smooth_k, context_parallel, bf16_cache):
        if smooth_k not in (False, True, "codes"):
            raise ValueError("enable_fp8_attention: smooth_k is False, True or \"codes\"")
        if not any(context_parallel is v for v in (False, True)) and context_parallel != "codes":
            raise ValueError("enable_fp8_attention: context_parallel is False, True or \"codes\"")
        codes = isinstance(smooth_k, str)
        cp_codes = isinstance(context_parallel, str)
        if smooth_k and context_parallel:
            raise ValueError(f"enable_fp8_attention: smooth_k={smooth_k!r} is not supported together with context_parallel={context_parallel!r}")
        if cp_codes and bf16_cache:
            raise ValueError("enable_fp8_attention: context_parallel=\"codes\" exchanges the codes of the compact cache: it needs "
                             "bf16_cache=False (with the bf16 cache kept, context_parallel=True)")
        if codes and bf16_cache:
            raise ValueError("enable_fp8_attention: smooth_k=\"codes\" takes the centres from the codes of the compact cache: it needs "
                             "bf16_cache=False (with the bf16 cache kept, smooth_k=True)")
        if not bf16_cache and smooth_k and not codes:
            raise ValueError("enable_fp8_attention: smooth_k=True needs the bf16 KV cache (bf16_cache=False keeps none to take the centres from; "
                             "smooth_k=\"codes\" takes them from the codes)")
        if not bf16_cache and not cp_codes and (context_parallel or self.model.context_parallel is not None):
            raise ValueError("enable_fp8_attention: bf16_cache=False does not support context parallelism "
                             "(but for context_parallel=\"codes\" under ContextParallel(exchange=\"rows\"))")
        k_scale, v_scale = float(k_scale), float(v_scale)
        for s in (k_scale, v_scale):
            if not (math.isfinite(s) and s > 0):
                raise ValueError("enable_fp8_attention: scales must be finite and positive")
        self.prev = self.mode
        self.epoch += 1
        self.mode = Mode(k_scale, v_scale, self.epoch, "codes" if codes else bool(smooth_k),
                         "codes" if cp_codes else bool(context_parallel), not bf16_cache)

    def disable(self):
        self.epoch += 1
        self.mode = self.prev = None

    def smooth(self):
        return self.mode is not None and self.mode.smooth

    def only(self):
        return self.mode is not None and self.mode.only

    def codes(self):
        """enable_fp8_attention(bf16_cache=False, smooth_k="codes") is on."""
        return self.only() and self.mode.smooth == "codes"

    def cp_codes(self):
        """enable_fp8_attention(bf16_cache=False, context_parallel="codes") is on."""
        return self.only() and self.mode.context_parallel == "codes"

    def staging(self, M, world, device):
        """The staging buffer of the code exchange (include/rtv_hip_attn_fp8_only_cp.h), one per (M, world, device) for all layers,
        never reallocated: captured hipGraphs embed its address."""
        key = (int(M), int(world), torch.device(device))
        if key not in self.kv8:
            self.kv8[key] = ops.attn_fp8_staging(M, self.model.num_heads, world, device)
        return self.kv8[key]

    def center_stamp(self):
        """What a compact dict records as "fp8_center" when rows are written into it: None in the plain compact mode, else the
        model and the epoch of its centres."""
        return (id(self.model), self.center_epoch) if self.codes() else None

    # ------------------------------------------------------------------ the buffers the model owns
    def amax_table(self):
        if self.amax is None:
            raise RuntimeError("fp8 attention has not run yet")
        return self.amax

    def _amax_table(self, device):
        if self.amax is None:
            self.amax = torch.zeros(self.model.num_layers, 2, dtype=torch.float32, device=device)
        return self.amax

    def alloc_centers(self, H, device, rows=0):
        """The centre buffers of both smoothing modes, zero-filled, and the mean kernel's workspace for a cache of `rows` rows: made by
        the first forward (or by set_centers() in front of it), kept from then on."""
        if self.center is None or tuple(self.center.shape[1:]) != (H, 128) or self.center.device != device:
            self.center = torch.zeros(self.model.num_layers, H, 128, dtype=torch.float32, device=device)
            self.center_new = self.center_ws = None
            if self.mode.smooth == "codes":
                self.center_epoch += 1          # (zeros again: rows coded under the centres dropped are under others now; a shadow
                                                #  sees the new buffer's address in its "fp8_filled" state)
        if self.mode.smooth == "codes" and self.center_new is None:
            self.center_new = torch.zeros_like(self.center)
        need = ops.attn_kv_center_workspace_bytes(rows, H) if rows > 0 else 0
        if rows > 0 and (self.center_ws is None or self.center_ws.numel() * 4 < need):      # (a larger cache than any before)
            self.center_ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=device)

    # ------------------------------------------------------------------ the shadows of a forward
    def _struct(self, k8s, v8ts, rows, centred=False):
        """One rtv_attn_fp8_shadow over per-layer k8 / v8t arrays -> Keep(struct, the pointer arrays it refers to, the centre table
        when `centred`)."""
        L = self.model.num_layers
        arrs = [(c_vp * L)(*[t_.data_ptr() for t_ in ts]) for ts in (k8s, v8ts, [self.amax[l] for l in range(L)])]
        pp = ctypes.POINTER(c_vp)
        sh = _Fp8Shadow(ctypes.cast(arrs[0], pp), ctypes.cast(arrs[1], pp), rows, self.mode.k_scale, self.mode.v_scale,
                        ctypes.cast(arrs[2], pp))
        return Keep(sh, arrs, (c_vp * L)(*[self.center[l].data_ptr() for l in range(L)]) if centred else None)

    def _fill_state(self, c, mode, centred, *extra):
        """What "fp8_filled" holds on a bf16 cache dict whose shadow is current: the scales and epoch of `mode`, the cache tensors the
        codes were made from, the centres when the K codes stand under them, and what else names the shadow's layout."""
        state = tuple(mode[:3]) + (c["k"].data_ptr(), c["v"].data_ptr())
        if centred:
            state += (self.center_epoch, self.center.data_ptr())
        return state + extra

    def _only_shadow(self, kv_cache):
        """shadow() for the e4m3-only cache (checked by check_kv_cache_kind): nothing to allocate but the maxima, nothing to fill."""
        rows, device = kv_cache_rows(kv_cache[0]), kv_cache[0]["k8"].device
        self._amax_table(device)
        if self.codes():
            self.alloc_centers(self.model.num_heads, device, rows)
        keep = self._struct([c["k8"] for c in kv_cache], [c["v8t"] for c in kv_cache], rows, centred=self.codes())
        return keep.shadow, keep

    def shadow(self, kv_cache, use_cp):
        """The rtv_attn_fp8_shadow of this forward over bf16 cache dicts (None: bf16 attention) and what must stay alive with it.
        Under the head exchange of a context-parallel forward: a list, one shadow per local rank."""
        mode, model = self.mode, self.model
        if mode is None:
            return None, None
        if use_cp and not mode.context_parallel:
            raise RuntimeError("fp8 attention does not support context parallelism (sharded calls and the KV split have no fp8 kernels)")
        self._amax_table(kv_cache[0]["k"].device)
        rows = kv_cache_rows(kv_cache[0])
        if use_cp and model.context_parallel.head_exchange(model.num_heads):
            return self._shadow_heads(kv_cache, rows)
        smooth = mode.smooth
        if smooth:
            k0 = kv_cache[0]["k"]
            self.alloc_centers(k0.shape[2], k0.device, rows)
        for l, c in enumerate(kv_cache):
            if c["k"].shape[0] != 1 or c["k"].shape[1] != rows:
                raise ValueError("fp8 attention: batch size 1 and the same number of rows in every layer's KV cache")
            H = c["k"].shape[2]
            if smooth and H != self.center.shape[1]:
                raise ValueError("fp8 attention: smooth_k needs the same number of heads in every layer's KV cache")
            if "k8" not in c or tuple(c["k8"].shape[:2]) != (rows, H) or c["k8"].device != c["k"].device:
                c["k8"], c["v8t"] = ops.attn_fp8_shadow(rows, H, c["k"].device)
                c["fp8_filled"] = None
            state = self._fill_state(c, mode, smooth)
            if c.get("fp8_filled") != state:
                ops.attn_quantize_kv(c["k"][0], c["v"][0], c["k8"], c["v8t"], 0, rows, mode.k_scale, mode.v_scale, amax=self.amax[l],
                                     center=self.center[l] if smooth else None)
                c["fp8_filled"] = state
        keep = self._struct([c["k8"] for c in kv_cache], [c["v8t"] for c in kv_cache], rows, centred=bool(smooth))
        return keep.shadow, keep

    def _shadow_heads(self, kv_cache, rows):
        """Head exchange: per layer and local rank one dense shadow of the num_heads / world heads the rank owns ("k8_hp" / "v8t_hp" of
        the cache dict, allocated once), filled from the rank's head slice of the bf16 cache.  -> ([shadow per local rank], keep)."""
        mode, cp = self.mode, self.model.context_parallel
        H, W = self.model.num_heads, cp.world
        hn = H // W
        ranks = list(cp.local_ranks())
        for l, c in enumerate(kv_cache):
            Hc = c["k"].shape[2]
            if c["k"].shape[0] != 1 or c["k"].shape[1] != rows or Hc not in (hn, H):
                raise ValueError(f"fp8 attention: batch size 1, the same number of rows in every layer's KV cache, and {hn} (this rank's) or {H} heads")
            hp = c.get("k8_hp")
            if hp is None or len(hp) != len(ranks) or tuple(hp[0].shape[:2]) != (rows, hn) or hp[0].device != c["k"].device:
                pairs = [ops.attn_fp8_shadow(rows, hn, c["k"].device) for _ in ranks]
                c["k8_hp"], c["v8t_hp"] = [p[0] for p in pairs], [p[1] for p in pairs]
                c["fp8_filled"] = None
            state = self._fill_state(c, mode, False, "heads", tuple(ranks), Hc)
            if c.get("fp8_filled") != state:
                for i, r in enumerate(ranks):
                    h0 = 0 if Hc == hn else r * hn
                    ops.attn_quantize_kv(c["k"][0][:, h0:h0 + hn], c["v"][0][:, h0:h0 + hn], c["k8_hp"][i], c["v8t_hp"][i], 0, rows,
                                         mode.k_scale, mode.v_scale, amax=self.amax[l])
                c["fp8_filled"] = state
        built = [self._struct([c["k8_hp"][i] for c in kv_cache], [c["v8t_hp"][i] for c in kv_cache], rows) for i in range(len(ranks))]
        shs = [b.shadow for b in built]
        return shs, Keep(shs, [b.arrays for b in built], None)

    def plan(self, kv_cache, use_cp):
        """What one forward over `kv_cache` (checked by check_kv_cache_kind) needs -> Plan.  Fills or refills the shadows of bf16 cache
        dicts on the way; allocates only what the first forward of a mode has to."""
        mode = self.mode
        if mode is not None and mode.only:
            shadow, keep = self._only_shadow(kv_cache)
            scales, stamp = (mode.k_scale, mode.v_scale), self.center_stamp()

            def commit():
                for c in kv_cache:
                    c["fp8_scales"] = scales      # what the codes in the cache were made with: they cannot be made again
                    c["fp8_center"] = stamp
        else:
            (shadow, keep), commit = self.shadow(kv_cache, use_cp), None
        if shadow is None:
            return Plan(None, None, ("rtv_dit_forward",), None, None)
        key = (mode.k_scale, mode.v_scale)
        if isinstance(shadow, list):      # head exchange: one shadow per local rank
            key += ("heads", kv_cache[0]["k8_hp"][0].data_ptr(), kv_cache[-1]["v8t_hp"][-1].data_ptr())
        else:
            key += (kv_cache[0]["k8"].data_ptr(), kv_cache[-1]["v8t"].data_ptr())
        if mode.only:      # the entry point is part of the graph key like the scales
            key = ("only", "codes") + key if mode.smooth else ("only",) + key
        if mode.smooth:
            key += (self.center.data_ptr(),)
        if use_cp:         # the context-parallel path has phases of its own
            return Plan(shadow, keep, ("rtv_dit_forward",), key, commit)
        forward = (_ENTRY[mode.only, mode.smooth], ctypes.byref(shadow)) + ((keep.centers,) if mode.smooth else ())
        return Plan(shadow, keep, forward, key, commit)

    # ------------------------------------------------------------------ what concerns the cache dicts
    def new_kv_cache(self, rows, device):
        caches = []
        for _ in range(self.model.num_layers):
            k8, v8t = ops.attn_fp8_shadow(int(rows), self.model.num_heads, device)
            caches.append({"k8": k8, "v8t": v8t, "rows": int(rows), "global_end_index": 0, "local_end_index": 0})
        return caches

    def check_kv_cache_kind(self, kv_cache, use_cp):
        """The refusals of the e4m3-only cache that concern the dicts: made by the forward before anything else looks at them."""
        model = self.model
        compact = ["k" not in c and "v" not in c for c in kv_cache]
        if not self.only():
            if any(compact):
                raise RuntimeError("this KV cache is an e4m3-only one (new_fp8_kv_cache): it needs enable_fp8_attention(bf16_cache=False)")
            return
        if use_cp or model.context_parallel is not None:
            if not self.cp_codes():
                raise RuntimeError("enable_fp8_attention(bf16_cache=False) does not support context parallelism "
                                   "(but for context_parallel=\"codes\" under ContextParallel(exchange=\"rows\"))")
            if model.context_parallel is not None and model.context_parallel.head_exchange(model.num_heads):
                raise RuntimeError("enable_fp8_attention(bf16_cache=False, context_parallel=\"codes\") runs under the row exchange only "
                                   "(the head exchange keeps 1 / world of the cache per rank already): use ContextParallel(exchange=\"rows\")")
        if not all(compact):
            raise RuntimeError("enable_fp8_attention(bf16_cache=False) needs the compact KV cache of new_fp8_kv_cache(): "
                               "this one has \"k\" / \"v\" entries")
        rows, scales = kv_cache_rows(kv_cache[0]), (self.mode.k_scale, self.mode.v_scale)
        for c in kv_cache:
            if kv_cache_rows(c) != rows or tuple(c["k8"].shape) != (rows, model.num_heads, 128) \
                    or tuple(c["v8t"].shape) != ((rows + 63) // 64, model.num_heads, 128, 64) \
                    or not (c["k8"].is_cuda and c["k8"].is_contiguous() and c["v8t"].is_contiguous()) \
                    or c["k8"].dtype != torch.uint8 or c["v8t"].dtype != torch.uint8 or c["v8t"].device != c["k8"].device:
                raise ValueError("fp8 attention: every layer's compact KV cache must be the k8 / v8t pair of new_fp8_kv_cache(rows) "
                                 "with the same number of rows")
            if int(c["local_end_index"]) > 0 and c.get("fp8_scales", scales) != scales:
                raise RuntimeError(f"fp8 attention: this e4m3-only KV cache holds rows quantised with k_scale, v_scale = {c['fp8_scales']}; "
                                   "their codes cannot be derived again for other scales: reset the cache first")
            if int(c["local_end_index"]) > 0 and c.get("fp8_center") != self.center_stamp():
                raise RuntimeError("fp8 attention: this e4m3-only KV cache holds rows coded under other K centres than the model's has now "
                                   "(fp8_attention_recenter / fp8_attention_set_centers move the rows of the caches they are given): "
                                   "reset the cache first")

    def _compact_rows(self, kv_cache, what):
        """The checks of the two calls that move the rows of compact dicts to other centres -> rows held per layer."""
        model = self.model
        if len(kv_cache) != model.num_layers:
            raise ValueError(f"{what}: one KV cache entry per layer")
        stamp, held = self.center_stamp(), []
        for c in kv_cache:
            if "k" in c or "v" in c or "k8" not in c:
                raise RuntimeError(f"{what}: enable_fp8_attention(bf16_cache=False) needs the compact KV cache of new_fp8_kv_cache()")
            if tuple(c["k8"].shape[1:]) != (model.num_heads, 128):
                raise ValueError(f"{what}: the compact cache must hold the model's {model.num_heads} heads")
            n = min(int(c["local_end_index"]), kv_cache_rows(c))
            if n > 0 and c.get("fp8_center") != stamp:
                raise RuntimeError(f"{what}: this e4m3-only KV cache holds rows coded under other K centres than the model's: reset the cache first")
            held.append(max(n, 0))
        return held

    def recenter(self, kv_cache):
        model = self.model
        if not self.smooth():
            raise RuntimeError("fp8_attention_recenter needs enable_fp8_attention(smooth_k=True) or, on the compact cache, smooth_k=\"codes\"")
        if self.only():
            return self._recenter_codes(kv_cache)
        if self.center is None:
            raise RuntimeError("fp8 attention has not run yet: the centres are allocated by the first forward")
        if len(kv_cache) != model.num_layers:
            raise ValueError("fp8_attention_recenter: one KV cache entry per layer")
        for l, c in enumerate(kv_cache):
            k = c["k"]
            if k.shape[0] != 1 or tuple(k.shape[2:]) != tuple(self.center.shape[1:]):
                raise ValueError("fp8_attention_recenter: batch size 1 and the heads the centres were allocated for")
            n = min(int(c["local_end_index"]), k.shape[1])
            if n <= 0:
                raise RuntimeError("fp8_attention_recenter: the KV cache is empty")
            if ops.attn_kv_center_workspace_bytes(n, k.shape[2]) > self.center_ws.numel() * 4:
                raise RuntimeError("fp8_attention_recenter: this cache is larger than the one the workspace was allocated for")
            ops.attn_kv_center(k[0], (0, n), out=self.center[l], workspace=self.center_ws)
        self.center_epoch += 1

    def _recenter_codes(self, kv_cache):
        """recenter on compact dicts (smooth_k="codes"): per layer that holds rows, the new centre from the codes (into the second
        buffer), the rows moved to it in place, the second buffer copied into the first.  Allocates nothing; captured hipGraphs keep
        their addresses."""
        if not self.codes():
            raise RuntimeError("fp8_attention_recenter on the compact cache needs enable_fp8_attention(bf16_cache=False, smooth_k=\"codes\") "
                               "(smooth_k=True takes the centres from a bf16 cache)")
        if self.center_new is None or self.center_ws is None:
            raise RuntimeError("fp8 attention has not run yet: the centres are allocated by the first forward")
        held = self._compact_rows(kv_cache, "fp8_attention_recenter")
        if not any(held):
            raise RuntimeError("fp8_attention_recenter: the KV cache is empty")
        for n in held:
            if ops.attn_kv_center_workspace_bytes(n, self.model.num_heads) > self.center_ws.numel() * 4:
                raise RuntimeError("fp8_attention_recenter: this cache is larger than the one the workspace was allocated for")
        k_scale, old, new = self.mode.k_scale, self.center, self.center_new
        for l, (c, n) in enumerate(zip(kv_cache, held)):
            if n > 0:
                ops.attn_k8_center(c["k8"], (0, n), k_scale=k_scale, c_old=old[l], out=new[l], workspace=self.center_ws)
                ops.attn_k8_recenter(c["k8"], old[l], new[l], 0, n, k_scale, amax=self.amax[l])
                old[l].copy_(new[l])
        self.center_epoch += 1
        for c in kv_cache:
            c["fp8_center"] = self.center_stamp()

    def set_centers(self, centers, kv_cache=None):
        model = self.model
        if not self.smooth():
            raise RuntimeError("fp8_attention_set_centers needs enable_fp8_attention(smooth_k=True) or smooth_k=\"codes\"")
        if not torch.is_tensor(centers) or centers.dtype != torch.float32 or centers.dim() != 3 or centers.shape[0] != model.num_layers \
                or centers.shape[2] != 128 or not centers.is_cuda:
            raise ValueError("fp8_attention_set_centers: centers must be a float32 GPU tensor [num_layers, H, 128]")
        codes = self.codes()
        if self.center is not None and tuple(centers.shape) != tuple(self.center.shape):
            raise ValueError("fp8_attention_set_centers: centers must have the heads the model's centres were allocated for")
        if codes and centers.shape[1] != model.num_heads:
            raise ValueError(f"fp8_attention_set_centers: the compact cache holds the model's {model.num_heads} heads")
        held = self._compact_rows(kv_cache, "fp8_attention_set_centers") if codes and kv_cache is not None else []
        if any(held) and self.amax is None:
            raise RuntimeError("fp8 attention has not run yet")
        self.alloc_centers(centers.shape[1], centers.device)
        if codes:
            k_scale, old, new = self.mode.k_scale, self.center, self.center_new
            new.copy_(centers)
            for l, n in enumerate(held):
                if n > 0:
                    ops.attn_k8_recenter(kv_cache[l]["k8"], old[l], new[l], 0, n, k_scale, amax=self.amax[l])
            old.copy_(new)
        else:
            self.center.copy_(centers)
        self.center_epoch += 1
        for c in (kv_cache or []) if codes else []:
            c["fp8_center"] = self.center_stamp()

    def convert_kv_cache(self, kv_cache):
        model, mode = self.model, self.mode
        if not self.only():
            raise RuntimeError("convert_kv_cache_to_fp8 needs enable_fp8_attention(bf16_cache=False)")
        if model.context_parallel is not None:
            raise RuntimeError("enable_fp8_attention(bf16_cache=False) does not support context parallelism")
        if len(kv_cache) != model.num_layers:
            raise ValueError("convert_kv_cache_to_fp8: one KV cache entry per layer")
        for c in kv_cache:
            if "k" not in c or "v" not in c:
                raise ValueError("convert_kv_cache_to_fp8: this KV cache is a compact one already")
            k, v = c["k"], c["v"]
            if k.shape[0] != 1 or tuple(k.shape[2:]) != (model.num_heads, 128) or k.shape != v.shape or k.shape[1] != kv_cache[0]["k"].shape[1]:
                raise ValueError(f"convert_kv_cache_to_fp8: batch size 1, the model's {model.num_heads} heads and the same number of rows in every layer")
        codes = self.codes()
        device, rows = kv_cache[0]["k"].device, kv_cache[0]["k"].shape[1]
        self._amax_table(device)
        if codes:
            self.alloc_centers(model.num_heads, device, rows)
        # a shadow is current when the mode this enable call replaced kept it: same scales, K codes under the same centres
        prev = self.prev
        current = prev is not None and (prev.k_scale, prev.v_scale) == (mode.k_scale, mode.v_scale) and prev.smooth is (True if codes else False)
        shape = (rows, model.num_heads, 128)
        for l, c in enumerate(kv_cache):
            if not current or "k8" not in c or c.get("fp8_filled") != self._fill_state(c, prev, codes) or tuple(c["k8"].shape) != shape:
                if "k8" not in c or tuple(c["k8"].shape) != shape or c["k8"].device != device:
                    c["k8"], c["v8t"] = ops.attn_fp8_shadow(rows, model.num_heads, device)
                ops.attn_quantize_kv(c["k"][0], c["v"][0], c["k8"], c["v8t"], 0, rows, mode.k_scale, mode.v_scale, amax=self.amax[l],
                                     center=self.center[l] if codes else None)
        for c in kv_cache:
            for name in ("k", "v", "fp8_filled", "k8_hp", "v8t_hp"):
                c.pop(name, None)
            c["rows"] = rows
            c["fp8_scales"] = (mode.k_scale, mode.v_scale)
            c["fp8_center"] = self.center_stamp()
        return kv_cache
