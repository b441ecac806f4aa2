"""TAEHV tiny-VAE streaming decoder and encoder: the opt-in fast codec behind `use_taehv` (the reference's `config.use_taehv`,
release_server.py:350), for the `decoder` / `encoder` of demo_utils/taehv.py:159-234 with the Wan 2.1 checkpoint taew2_1.pth.

    pixels, state = TAEHVDecoder(device)(z[1, T, 16, h, w] fp16, *state)

is the streaming contract of `VAEDecoderWrapper`: a list of `None` (the session's `[None] * 55`) starts a stream, passing
the returned list back continues it.  pixels are float32 [1, T', 3, 8h, 8w] = clamp(2 * decoder - 1, -1, 1), T' = 4T - 3
on a stream's first call (TAEHV's 3 warm-up frames, `frames_to_trim`, are not produced) and 4T afterwards - the frame
count and alignment of the Wan decoder.  The returned state is the nine MemBlock state slices (each block's input at the
previous frame of its rate) as [1, C, H, W] views into the stream's arena, updated in place by the next call.  Backed by
`rtv_taehv_decode` (include/rtv_hip.h, csrc/taehv.hip); no CPU fallback.

    latents[1, 16, T', h, w], cache = TAEHVEncoder(device)(frames[1, 3, T, H, W] in [-1, 1], feat_cache, stream=False)

is the call contract of `VAEEncoderWrapper`, so `encode_video_latent(vae=TAEHVEncoder, ...)` works unchanged; see the class.
"""
import ctypes
import hashlib
import math

import torch

from . import _lib
from .vae_decoder import CacheArenas, pack_conv_weight

c_vp = ctypes.c_void_p

MEMBLOCKS = (3, 4, 5, 9, 10, 11, 15, 16, 17)      # decoder indices of the nine MemBlocks
MEM_CHANNELS = (256, 256, 256, 128, 128, 128, 64, 64, 64)
TGROWS = ((7, 8, 256, 128, 1), (13, 14, 128, 64, 2), (19, 20, 64, 64, 2))   # (TGrow idx, conv idx, C in, C out, stride)
WARMUP_FRAMES = 3                                  # TAEHV.frames_to_trim with the default decoder_time_upscale

ENC_MEMBLOCKS = (4, 5, 6, 9, 10, 11, 14, 15, 16)  # encoder indices of the nine MemBlocks (64 channels each)
TPOOLS = ((2, 3, 2), (7, 8, 2), (12, 13, 1))      # (TPool idx, stride-2 conv idx, time stride)


_TaehvWeights = _lib.STRUCTS["rtv_taehv_weights"]
_TaehvEncWeights = _lib.STRUCTS["rtv_taehv_enc_weights"]


def arena_bytes(h, w, t_max):
    return int(_lib.load().rtv_taehv_arena_bytes(h, w, t_max))


def enc_arena_bytes(H, W, t_max):
    return int(_lib.load().rtv_taehv_enc_arena_bytes(H, W, t_max))


def fold_tgrow(tgrow_w, conv_w, stride):
    """TGrow (1x1, C -> stride * C, no bias) followed by a bias-free 3x3 conv C -> Cout, as ONE 3x3 conv C -> stride * Cout whose
    filter s * Cout + o is output channel o of frame stride * t + s (exact: the nearest upsampling in front commutes with the
    1x1 conv, and TGrow maps the conv's zero padding to zeros).  Composed in float32."""
    tg = tgrow_w.detach().float().reshape(tgrow_w.shape[0], tgrow_w.shape[1])   # [stride * C][C]
    cw = conv_w.detach().float()                                               # [Cout][C][3][3]
    C = tg.shape[1]
    parts = [torch.einsum("okyx,kc->ocyx", cw, tg[s * C:(s + 1) * C]) for s in range(stride)]
    return torch.cat(parts, 0)


def fold_tpool(tpool_w, conv_w, stride):
    """TPool (1x1, stride * C -> C over the channels of `stride` consecutive frames, no bias) followed by a bias-free 3x3 conv
    C -> Cout, as ONE conv whose time tap s reads frame stride * t + s: [Cout, C, stride, 3, 3] (stride 1: [Cout, C, 3, 3]).
    Exact: both are linear, nothing sits between them and TPool maps the conv's zero padding to zeros.  The mirror of
    fold_tgrow.  Composed in float32."""
    tp = tpool_w.detach().float().reshape(tpool_w.shape[0], tpool_w.shape[1])   # [C][stride * C]
    cw = conv_w.detach().float()                                               # [Cout][C][3][3]
    C = tp.shape[0]
    parts = [torch.einsum("okyx,kc->ocyx", cw, tp[:, s * C:(s + 1) * C]) for s in range(stride)]
    return parts[0] if stride == 1 else torch.stack(parts, 2)


class _TAEHVCodec:
    """What the two halves share: the state-dict loader with the MemBlock repack, the synthetic weights, and a stream's arena
    with its nine state views.  A subclass gives
        NAME, HALF / OTHER_HALF   its name in error texts; the state-dict prefix it loads / ignores
        WEIGHTS, MEM              the C struct of its weights; (module index, channels) of its nine MemBlocks
        GAINS, BIAS_MEANS         random_state_dict's exceptions by tensor name
        SLOT_FN                   the library's state-slot function of its arena
        state_dict_spec(), _pack_layers(), _arena_bytes(), forward()"""
    z_dim = 16
    BIAS_MEANS = {}

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._t = {}
        self._w = None
        self._arenas = CacheArenas()

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def half(self):
        return self

    # ------------------------------------------------------------------ weights
    def _checkpoint_view(self, sd):
        return sd

    def load_state_dict(self, sd, strict=True):
        """Reference key names (`decoder.{i}...` / `encoder.{i}...`); the keys of the other half (a real taew2_1.pth carries
        both) are ignored."""
        who = f"{type(self).__name__}.load_state_dict"
        spec = dict(self.state_dict_spec())
        sd = self._checkpoint_view({k: v for k, v in sd.items() if not k.startswith(self.OTHER_HALF)})
        missing = [k for k in spec if k not in sd]
        unexpected = [k for k in sd if k not in spec]
        if strict and (missing or unexpected):
            raise KeyError(f"{who}: missing {missing}, unexpected {unexpected}")
        if missing:
            raise KeyError(f"{who}: missing {missing}")
        for k, shape in spec.items():
            if tuple(sd[k].shape) != shape:
                raise ValueError(f"{who}: {k} has shape {tuple(sd[k].shape)}, expected {shape}")
        dev, f16 = self.device, torch.float16
        t = {}
        W = self.WEIGHTS()

        def put(name, x):
            t[name] = x.to(dev).contiguous()
            return t[name].data_ptr()

        def conv(dst, wname, w, b, cin_pad=None, cout_pad=None):
            dst.w = put(wname + ".w", pack_conv_weight(w, cin_pad, cout_pad))
            b = b.detach().to(f16).reshape(-1)
            if cout_pad and cout_pad > b.numel():
                b = torch.cat([b, b.new_zeros(cout_pad - b.numel())])
            dst.b = put(wname + ".b", b)

        for k, (idx, C) in enumerate(self.MEM):
            pre = f"{self.HALF}{idx}.conv"
            w0 = sd[pre + ".0.weight"]
            # cat([x_t, x_{t-1}]) input channels -> time taps [x_{t-1} | x_t] of a 2-slice conv
            conv(W.mem[k][0], pre + ".0", torch.stack([w0[:, C:], w0[:, :C]], dim=2), sd[pre + ".0.bias"])
            conv(W.mem[k][1], pre + ".2", sd[pre + ".2.weight"], sd[pre + ".2.bias"])
            conv(W.mem[k][2], pre + ".4", sd[pre + ".4.weight"], sd[pre + ".4.bias"])
        self._pack_layers(sd, W, put, conv)
        self._t, self._w = t, W
        return [], []

    @classmethod
    def random_state_dict(cls, seed=0):
        """Deterministic synthetic weights (CPU generator, float32) that keep the signal alive through the layers: He-scaled
        convs in front of a ReLU, each MemBlock's last conv scaled down (its branch adds to the identity), unit gain for
        TGrow / TPool (no ReLU behind them), small biases; cls.GAINS / cls.BIAS_MEANS hold the class's exceptions."""
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for name, shape in cls.state_dict_spec():
            if name.endswith(".bias"):
                sd[name] = 0.02 * torch.randn(shape, generator=g)
                if name in cls.BIAS_MEANS:
                    sd[name] = cls.BIAS_MEANS[name] + sd[name]
                continue
            fan_in = math.prod(shape[1:])
            gain = math.sqrt(2.0)
            if name.endswith(".conv.4.weight"):
                gain = 0.3
            elif ".conv.weight" in name:
                gain = 1.0
            elif name in cls.GAINS:
                gain = cls.GAINS[name]
            sd[name] = torch.randn(shape, generator=g) * (gain / math.sqrt(fan_in))
        return sd

    @classmethod
    def checksum(cls, sd):
        """sha256 over the float32 bytes of the class's tensors in state_dict_spec order."""
        h = hashlib.sha256()
        for name, _ in cls.state_dict_spec():
            h.update(sd[name].detach().float().contiguous().cpu().numpy().tobytes())
        return h.hexdigest()

    def init_random_weights(self, seed=0):
        self.load_state_dict(self.random_state_dict(seed))
        return self

    # ------------------------------------------------------------------ arena / state views
    def _new_arena(self, size, t_max):
        n = self._arena_bytes(*size, t_max)
        if n == 0:
            raise ValueError(f"{self.NAME}: unsupported size {size[0]}x{size[1]} / {t_max} frames per call")
        arena = torch.empty(n + 256, dtype=torch.uint8, device=self.device)   # the state is zeroed by a stream's first call
        return arena, (-arena.data_ptr()) % 256

    def _state_views(self, arena, base, size):
        views = []
        off, C, H, W = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        for i in range(9):
            _lib.call(self.SLOT_FN, *size, i, ctypes.byref(off), ctypes.byref(C), ctypes.byref(H), ctypes.byref(W))
            start = base + off.value
            v = arena[start:start + C.value * H.value * W.value * 2].view(torch.float16).view(H.value, W.value, C.value)
            views.append(v.permute(2, 0, 1).unsqueeze(0))     # [1, C, H, W] (channels-last in memory)
        self._arenas.register(views, arena, base, size)
        return views

    def _acquire(self, views, size, t_max, need):
        """(arena, base, views) of a stream of frame size `size` for a call that needs `need` bytes.  views None: a new stream,
        on the arena of a dropped stream of this size if there is one that is large enough, else on a new one for calls of
        up to t_max frames.  Otherwise the stream whose state views these are; a call longer than its arena was sized for
        moves the state to a larger one."""
        if views is None:
            ent = self._arenas.recycle(size)
            if ent is None or ent[0].numel() - ent[1] < need:
                ent = self._new_arena(size, t_max)
            arena, base = ent
            return arena, base, self._state_views(arena, base, size)
        arena, base = self._arenas.lookup(views, size, lambda: self._new_arena(size, t_max)[0],
                                          lambda a, b: self._state_views(a, b, size))
        if arena.numel() - base < need:
            self._arenas.forget(views)
            arena, base = self._new_arena(size, t_max)
            old, views = views, self._state_views(arena, base, size)
            for dst, src in zip(views, old):
                dst.copy_(src)
        return arena, base, views

    def _check_input(self, z):
        if self._w is None:
            raise RuntimeError(f"{self.NAME}: weights not loaded")
        if not z.is_cuda:
            raise RuntimeError(f"realtime_video_amd.{type(self).__name__} needs GPU tensors (no CPU fallback)")

    def __call__(self, *a, **k):
        return self.forward(*a, **k)


class TAEHVDecoder(_TAEHVCodec):
    NAME, HALF, OTHER_HALF = "TAEHV decoder", "decoder.", "encoder."
    WEIGHTS, MEM, SLOT_FN = _TaehvWeights, tuple(zip(MEMBLOCKS, MEM_CHANNELS)), "rtv_taehv_state_slot"
    # the conv behind a TGrow: no ReLU in between / after (decoder.20 has one); a head that maps to about 0.5 +- 0.1 (std), inside
    # TAEHV's [0, 1]
    GAINS = {"decoder.8.weight": 1.0, "decoder.14.weight": 1.0, "decoder.22.weight": 0.13}
    BIAS_MEANS = {"decoder.22.bias": 0.5}
    _arena_bytes = staticmethod(arena_bytes)

    def __init__(self, device="cuda", decoder_time_upscale=(True, True), decoder_space_upscale=(True, True, True)):
        if tuple(decoder_time_upscale) != (True, True) or tuple(decoder_space_upscale) != (True, True, True):
            raise NotImplementedError("TAEHVDecoder: only the default decoder_time_upscale / decoder_space_upscale")
        super().__init__(device)

    @staticmethod
    def state_dict_spec():
        """(name, shape) of every tensor of the reference module's `decoder` state_dict, in module order."""
        spec = [("decoder.1.weight", (256, 16, 3, 3)), ("decoder.1.bias", (256,))]
        for idx, C in zip(MEMBLOCKS, MEM_CHANNELS):
            for j, cin in ((0, 2 * C), (2, C), (4, C)):
                spec += [(f"decoder.{idx}.conv.{j}.weight", (C, cin, 3, 3)), (f"decoder.{idx}.conv.{j}.bias", (C,))]
            if idx in (5, 11, 17):
                tg, cv, cin, cout, stride = TGROWS[(idx - 5) // 6]
                spec += [(f"decoder.{tg}.conv.weight", (cin * stride, cin, 1, 1)), (f"decoder.{cv}.weight", (cout, cin, 3, 3))]
        spec += [("decoder.22.weight", (3, 64, 3, 3)), ("decoder.22.bias", (3,))]
        return spec

    @staticmethod
    def patch_tgrow_layers(sd):
        """taehv.py:195-208: a TGrow weight wider than the module's keeps its LAST stride * C output channels.  Returns a new dict."""
        sd = dict(sd)
        for tg, _cv, cin, _cout, stride in TGROWS:
            key = f"decoder.{tg}.conv.weight"
            if key in sd and sd[key].shape[0] > cin * stride:
                sd[key] = sd[key][-cin * stride:]
        return sd

    _checkpoint_view = patch_tgrow_layers

    @staticmethod
    def _pack_layers(sd, W, put, conv):
        conv(W.conv_in, "decoder.1", sd["decoder.1.weight"], sd["decoder.1.bias"], cin_pad=32)
        for s, (tg, cv, _cin, _cout, stride) in enumerate(TGROWS):
            W.up[s] = put(f"up{s}", pack_conv_weight(fold_tgrow(sd[f"decoder.{tg}.conv.weight"], sd[f"decoder.{cv}.weight"], stride)))
        conv(W.head, "decoder.22", sd["decoder.22.weight"], sd["decoder.22.bias"], cout_pad=8)

    def forward(self, z, *state):
        self._check_input(z)
        B, T, C, h, w = z.shape
        if B != 1 or C != 16:
            raise NotImplementedError("TAEHV decoder: batch 1, 16 latent channels")
        zz = z[0].to(torch.float16).contiguous()
        first = len(state) == 0 or state[0] is None
        need = arena_bytes(h, w, T)
        if need == 0:
            raise ValueError(f"TAEHV decoder: unsupported latent size {h}x{w} / T {T}")
        arena, base, views = self._acquire(None if first else list(state[:9]), (h, w), max(T, 3), need)
        n_out = 4 * T - WARMUP_FRAMES if first else 4 * T
        pixels = torch.empty((n_out, 3, 8 * h, 8 * w), dtype=torch.float32, device=z.device)
        _lib.call("rtv_taehv_decode", ctypes.byref(self._w), c_vp(zz.data_ptr()), T, h, w, int(first),
                  c_vp(arena.data_ptr() + base), ctypes.c_size_t(arena.numel() - base), c_vp(pixels.data_ptr()),
                  c_vp(torch.cuda.current_stream().cuda_stream))
        return pixels.unsqueeze(0), views


class TAEHVEncoder(_TAEHVCodec):
    """The `encoder` of demo_utils/taehv.py:172-178 behind the call contract of `VAEEncoderWrapper`: preview grade, not the
    Wan encoder.  No latent mean / std scaling (taew2_1 works in the DiT's latent space, as TAEHVDecoder assumes).

    Time contract (this project's convention - the reference never calls its encoder; the inverse of the decoder's dropped
    warm-up frames): a fresh cache (None / [None] * 55) takes T = 1 + 4k frames, presents frame 0 four times (the static clip
    whose decode is frame 0 once the decoder has dropped its 3 warm-up frames), then k groups of 4 -> 1 + k latents, the
    Wan encoder's count; a carried cache with stream=True takes T = 4k -> k latents.  Anything else raises ValueError.

    The returned cache is the nine MemBlock state slices ([1, 64, h, w] views into the stream's arena, updated in place by the
    next call).  Backed by `rtv_taehv_encode`; no CPU fallback."""
    GROUP = 12     # frames per rtv_taehv_encode call (sizes the arena: longer clips run in groups, bit-identical)
    NAME, HALF, OTHER_HALF = "TAEHV encoder", "encoder.", "decoder."
    WEIGHTS, MEM, SLOT_FN = _TaehvEncWeights, tuple((idx, 64) for idx in ENC_MEMBLOCKS), "rtv_taehv_enc_state_slot"
    # the conv behind a TPool and the head: no ReLU in between / after
    GAINS = {"encoder.3.weight": 1.0, "encoder.8.weight": 1.0, "encoder.13.weight": 1.0, "encoder.17.weight": 1.0}
    _arena_bytes = staticmethod(enc_arena_bytes)

    @staticmethod
    def state_dict_spec():
        """(name, shape) of every tensor of the reference module's `encoder` state_dict, in module order."""
        spec = [("encoder.0.weight", (64, 3, 3, 3)), ("encoder.0.bias", (64,))]
        for k, idx in enumerate(ENC_MEMBLOCKS):
            if k % 3 == 0:
                tp, cv, stride = TPOOLS[k // 3]
                spec += [(f"encoder.{tp}.conv.weight", (64, 64 * stride, 1, 1)), (f"encoder.{cv}.weight", (64, 64, 3, 3))]
            for j, cin in ((0, 128), (2, 64), (4, 64)):
                spec += [(f"encoder.{idx}.conv.{j}.weight", (64, cin, 3, 3)), (f"encoder.{idx}.conv.{j}.bias", (64,))]
        spec += [("encoder.17.weight", (16, 64, 3, 3)), ("encoder.17.bias", (16,))]
        return spec

    @staticmethod
    def _pack_layers(sd, W, put, conv):
        # first conv: K order c * 9 + dy * 3 + dx (the weight's own flattening), 27 taps padded to the MFMA's 32
        w0 = sd["encoder.0.weight"].detach().to(torch.float16).reshape(64, 27)
        W.conv_in.w = put("encoder.0.w", torch.cat([w0, w0.new_zeros(64, 5)], 1))
        W.conv_in.b = put("encoder.0.b", sd["encoder.0.bias"].detach().to(torch.float16).reshape(-1))
        for s, (tp, cv, stride) in enumerate(TPOOLS):
            W.down[s] = put(f"down{s}", pack_conv_weight(fold_tpool(sd[f"encoder.{tp}.conv.weight"], sd[f"encoder.{cv}.weight"], stride)))
        conv(W.head, "encoder.17", sd["encoder.17.weight"], sd["encoder.17.bias"])

    def forward(self, z, feat_cache=None, stream=False):
        self._check_input(z)
        B, Cc, T, H, W = z.shape
        if B != 1 or Cc != 3:
            raise NotImplementedError("TAEHV encoder: batch 1, RGB frames")
        fresh = feat_cache is None or len(feat_cache) == 0 or feat_cache[0] is None
        rule = ("TAEHV encoder time contract: a fresh cache takes T = 1 + 4k frames (frame 0 is presented four times), "
                "a carried cache with stream=True takes T = 4k")
        if fresh:
            if T < 1 or (T - 1) % 4:
                raise ValueError(f"{rule}; got a fresh cache with T = {T}")
        elif not stream or T < 4 or T % 4:
            raise ValueError(f"{rule}; got a carried cache with T = {T}, stream={bool(stream)}")
        need = 0 if H % 8 or W % 8 else enc_arena_bytes(H, W, self.GROUP)
        if need == 0:
            raise ValueError(f"TAEHV encoder: frame size {H}x{W} not supported (H and W must be multiples of 8)")
        frames = z[0].to(torch.float16)
        views = None
        if fresh:
            frames = torch.cat([frames[:, :1].expand(-1, 3, -1, -1), frames], 1)
        else:
            views = feat_cache if isinstance(feat_cache, list) else list(feat_cache)
            if len(views) != 9:
                raise ValueError(f"TAEHV encoder: a carried cache is the nine state slices a previous call returned, got {len(views)} slots")
        arena, base, views = self._acquire(views, (H, W), self.GROUP, need)
        frames = frames.contiguous()
        Tt = frames.shape[1]
        n_out = Tt // 4
        mu = torch.empty((16, n_out, H // 8, W // 8), dtype=torch.float16, device=z.device)
        st = c_vp(torch.cuda.current_stream().cuda_stream)
        for t0 in range(0, Tt, self.GROUP):
            tn = min(self.GROUP, Tt - t0)
            _lib.call("rtv_taehv_encode", ctypes.byref(self._w), c_vp(frames.data_ptr()), Tt, t0, tn, H, W, int(fresh and t0 == 0),
                      c_vp(arena.data_ptr() + base), ctypes.c_size_t(arena.numel() - base), c_vp(mu.data_ptr()), n_out, t0 // 4, st)
        return mu.unsqueeze(0).to(z.dtype), views
