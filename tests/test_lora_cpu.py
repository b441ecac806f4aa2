"""LoRA adapters, the part that needs no GPU: the binding of include/rtv_hip_lora.h, the refusals of rtv_lora_merge (all made
before any launch), the state-dict parser, and the oracle's criterion held against a torch fp32 emulation of the kernel."""
import ctypes
import math

import pytest
import torch

import lora_oracle as lo
from realtime_video_amd import _lib

KERNEL_SHAPES = [(160, 136, 4, 1.0), (256, 256, 16, 0.7), (384, 200, 48, -0.5), (128, 512, 256, 0.25)]   # N, K, rank, scale


# ------------------------------------------------------------------ binding
def test_lora_header_parses_into_tables_of_its_own():
    vp, i = ctypes.c_void_p, ctypes.c_int
    ad = _lib.LORA_STRUCTS["rtv_lora_adapter"]
    assert _lib.LORA_PROTOTYPES == {"rtv_lora_merge": (i, [vp, i, vp, i, i, i, ctypes.POINTER(ad), i, vp])}
    assert list(_lib.LORA_STRUCTS) == ["rtv_lora_adapter"]
    assert [(n, t) for n, t in ad._fields_] == [("A", vp), ("B", vp), ("rank", i), ("scale", ctypes.c_float)]
    for other in (_lib.PROTOTYPES, _lib.IO_PROTOTYPES, _lib.JPEG_PROTOTYPES, _lib.JPEGDEC_PROTOTYPES):
        assert not set(other) & set(_lib.LORA_PROTOTYPES)
    for other in (_lib.STRUCTS, _lib.IO_STRUCTS, _lib.JPEG_STRUCTS, _lib.JPEGDEC_STRUCTS):
        assert not set(other) & set(_lib.LORA_STRUCTS)
    assert (_lib.LORA_MAX_ADAPTERS, _lib.LORA_MAX_RANK) == (4, 256)


def test_library_exports_lora_merge_with_the_parsed_prototype():
    lib = _lib.load()
    fn = lib.rtv_lora_merge
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.LORA_PROTOTYPES["rtv_lora_merge"][1]


# ------------------------------------------------------------------ refusals (no launch happens: the pointers are never followed)
P = 0x10000          # a 16-byte aligned non-null "device address"


def _call(base=P, ldb=64, W=P, ldw=64, N=16, K=64, adapters=((P, P, 8, 1.0),), count=None, table=True):
    Ad = _lib.LORA_STRUCTS["rtv_lora_adapter"]
    arr = (Ad * max(1, len(adapters)))(*[Ad(*a) for a in adapters])
    status = _lib.load().rtv_lora_merge(base, ldb, W, ldw, N, K, arr if table else None, len(adapters) if count is None else count, None)
    return status, _lib.load().rtv_last_error().decode()


@pytest.mark.parametrize("kwargs, word", [
    (dict(base=None), "null"), (dict(W=None), "null"), (dict(table=False), "null"),
    (dict(adapters=((None, P, 8, 1.0),)), "null"), (dict(adapters=((P, None, 8, 1.0),)), "null"),
    (dict(N=0), "positive"), (dict(N=-3), "positive"), (dict(K=0), "positive"),
    (dict(base=P + 8), "misaligned"), (dict(W=P + 2), "misaligned"), (dict(adapters=((P + 8, P, 8, 1.0),)), "misaligned"),
    (dict(adapters=((P, P + 1, 8, 1.0),)), "misaligned"),
    (dict(K=60, ldb=64, ldw=64), "misaligned"), (dict(ldb=68), "misaligned"), (dict(ldw=100), "misaligned"),
    (dict(ldb=56), "stride"), (dict(ldw=8), "stride"),
    (dict(count=-1), "count"), (dict(count=5), "count"),
    (dict(adapters=((P, P, 0, 1.0),)), "rank"), (dict(adapters=((P, P, 257, 1.0),)), "rank"), (dict(adapters=((P, P, -1, 1.0),)), "rank"),
    (dict(adapters=((P, P, 8, math.inf),)), "finite"), (dict(adapters=((P, P, 8, math.nan),)), "finite"),
    (dict(adapters=((P, P, 8, 1.0), (P, P, 8, -math.inf))), "finite"),
])
def test_merge_refuses_before_any_launch(kwargs, word):
    status, msg = _call(**kwargs)
    assert status != 0 and msg.startswith("lora_merge") and word in msg, (status, msg)


# ------------------------------------------------------------------ the criterion, on the kernel's arithmetic in torch
@pytest.mark.parametrize("N, K, rank, scale", KERNEL_SHAPES)
def test_fp32_emulation_meets_the_kernel_criterion(N, K, rank, scale):
    base, [(A, B)] = lo.make_inputs(N, K, [rank], seed=N + rank)
    ref, mag = lo.merge_oracle(base, [(A, B, scale)])
    lo.assert_meets(lo.fp32_emulation(base, [(A, B, scale)]), ref, mag, f"fp32 emulation {N}x{K} r{rank}")   # the kernel's own criterion
    # and the criterion is not vacuous: a scale folded into a bf16 operand, or a missing adapter, fails it
    folded = (base.float() + (B.float() * scale).to(torch.bfloat16).float() @ A.float()).to(torch.bfloat16)
    if scale not in (1.0, 0.25, -0.5):      # (powers of two fold exactly)
        assert lo.criterion(folded, ref, mag)[1] < 0.999
    assert lo.criterion(base, ref, mag)[0] < 0.5


# ------------------------------------------------------------------ parser
def _model():
    from realtime_video_amd.causal_model import CausalWanModel
    return CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, device="cpu")


def _pair(out_f, in_f, r, style="AB", prefix="", target="blocks.0.self_attn.q", alpha=None):
    a, b = (".lora_A.weight", ".lora_B.weight") if style == "AB" else (".lora_down.weight", ".lora_up.weight")
    sd = {prefix + target + a: torch.zeros(r, in_f), prefix + target + b: torch.zeros(out_f, r)}
    if alpha is not None:
        sd[prefix + target + ".alpha"] = torch.tensor(float(alpha))
    return sd


@pytest.mark.parametrize("prefix", ["", "diffusion_model.", "model.diffusion_model.", "model."])
@pytest.mark.parametrize("style", ["AB", "updown"])
def test_parser_accepts_prefixes_and_suffix_styles(prefix, style):
    from realtime_video_amd.lora import parse_lora_state_dict
    sd = _pair(256, 256, 8, style, prefix)
    targets, unexpected = parse_lora_state_dict(sd, _model().state_dict_shapes())
    assert unexpected == [] and list(targets) == ["blocks.0.self_attn.q"]
    t = targets["blocks.0.self_attn.q"]
    assert (t.tensor, t.row0, t.rows, t.cols, t.rank, t.factor) == ("L0.qkv_w", 0, 256, 256, 8, 1.0)
    assert t.A.shape == (8, 256) and t.B.shape == (256, 8)


def test_parser_maps_every_target_and_applies_alpha():
    from realtime_video_amd.lora import parse_lora_state_dict
    sd = {}
    want = {"self_attn.q": ("qkv_w", 0, 256, 256), "self_attn.k": ("qkv_w", 256, 256, 256), "self_attn.v": ("qkv_w", 512, 256, 256),
            "self_attn.o": ("o_w", 0, 256, 256), "cross_attn.q": ("cq_w", 0, 256, 256), "cross_attn.k": ("ck_w", 0, 256, 256),
            "cross_attn.v": ("cv_w", 0, 256, 256), "cross_attn.o": ("co_w", 0, 256, 256), "ffn.0": ("ffn0_w", 0, 512, 256),
            "ffn.2": ("ffn2_w", 0, 256, 512)}
    for layer in (0, 1):
        for name, (_, _, out_f, in_f) in want.items():
            sd.update(_pair(out_f, in_f, 4, target=f"blocks.{layer}.{name}", alpha=2.0 if name == "ffn.0" else None))
    targets, unexpected = parse_lora_state_dict(sd, _model().state_dict_shapes())
    assert unexpected == [] and len(targets) == 20
    for layer in (0, 1):
        for name, (field, row0, out_f, in_f) in want.items():
            t = targets[f"blocks.{layer}.{name}"]
            assert (t.tensor, t.row0, t.rows, t.cols, t.rank) == (f"L{layer}.{field}", row0, out_f, in_f, 4)
            assert t.factor == (0.5 if name == "ffn.0" else 1.0)          # alpha / rank


@pytest.mark.parametrize("sd, word", [
    ({"blocks.0.self_attn.q.lora_A.weight": torch.zeros(4, 256)}, "blocks.0.self_attn.q.lora_A.weight"),
    ({"blocks.0.self_attn.q.lora_up.weight": torch.zeros(256, 4)}, "blocks.0.self_attn.q.lora_up.weight"),
    ({"blocks.0.ffn.0.alpha": torch.tensor(4.0)}, "blocks.0.ffn.0.alpha"),
    ({"blocks.0.ffn.0.lora_A.weight": torch.zeros(4, 512), "blocks.0.ffn.0.lora_B.weight": torch.zeros(512, 4)}, "ffn.0.lora_A.weight"),
    ({"blocks.0.ffn.2.lora_A.weight": torch.zeros(4, 512), "blocks.0.ffn.2.lora_B.weight": torch.zeros(512, 4)}, "ffn.2.lora_B.weight"),
    ({"blocks.0.ffn.2.lora_A.weight": torch.zeros(4, 512), "blocks.0.ffn.2.lora_B.weight": torch.zeros(256, 8)}, "ffn.2.lora_B.weight"),
    ({"blocks.1.cross_attn.o.lora_A.weight": torch.zeros(257, 256), "blocks.1.cross_attn.o.lora_B.weight": torch.zeros(256, 257)},
     "cross_attn.o.lora_A.weight"),
    ({**_pair(256, 256, 4), "blocks.0.self_attn.q.alpha": torch.ones(2)}, "blocks.0.self_attn.q.alpha"),
])
def test_parser_errors_name_the_key(sd, word):
    from realtime_video_amd.lora import parse_lora_state_dict
    with pytest.raises(ValueError, match=word.replace(".", r"\.")):
        parse_lora_state_dict(sd, _model().state_dict_shapes())


@pytest.mark.parametrize("key", [
    "blocks.0.self_attn.q.diff", "blocks.0.self_attn.q.diff_b", "blocks.0.self_attn.norm_q.lora_A.weight", "blocks.0.norm3.diff",
    "text_embedding.0.lora_A.weight", "head.head.lora_B.weight", "lora_unet_blocks_0_self_attn_q.lora_down.weight",
    "blocks.2.self_attn.q.lora_A.weight", "blocks.0.ffn.1.lora_A.weight", "blocks.0.self_attn.q.weight",
])
def test_parser_strict_against_non_strict(key):
    from realtime_video_amd.lora import parse_lora_state_dict
    sd = {**_pair(256, 256, 4), key: torch.zeros(4, 256)}
    shapes = _model().state_dict_shapes()
    with pytest.raises(ValueError, match="unexpected"):
        parse_lora_state_dict(sd, shapes)
    targets, unexpected = parse_lora_state_dict(sd, shapes, strict=False)
    assert list(targets) == ["blocks.0.self_attn.q"] and unexpected == [key]


def test_cpu_model_validates_but_refuses_to_merge():
    m = _model()
    with pytest.raises(ValueError, match="unexpected"):
        m.load_lora({"blocks.0.self_attn.q.diff": torch.zeros(256, 256)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.load_lora(_pair(256, 256, 4))
    assert m.lora_adapters() == {} and m.lora_version == 0
    with pytest.raises(KeyError):
        m.set_lora_scale("style", 0.5)
