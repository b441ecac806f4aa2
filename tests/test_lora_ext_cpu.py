"""The extended LoRA merges, the part that needs no GPU: the binding of include/rtv_hip_lora_ext.h, the refusals of
rtv_lora_merge_ex / rtv_lora_merge_dora (all made before any launch), the oracles' criterion held against torch fp32 emulations of
the kernels, the extended state-dict parser, and the CPU model."""
import ctypes
import math

import pytest
import torch

import lora_ext_oracle as xo
import lora_oracle as lo
from realtime_video_amd import _lib

BF = torch.bfloat16


# ------------------------------------------------------------------ binding
def test_ext_header_parses_into_tables_of_its_own():
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert list(_lib.LORA_EXT_STRUCTS) == ["rtv_lora_term"]
    term = _lib.LORA_EXT_STRUCTS["rtv_lora_term"]
    assert [(n, t) for n, t in term._fields_] == [("A", vp), ("B", vp), ("rank", i), ("scale", f), ("diff", vp), ("ldd", i),
                                                  ("diff_scale", f)]
    assert _lib.LORA_EXT_PROTOTYPES == {
        "rtv_lora_merge_ex": (i, [vp, i, vp, i, i, i, ctypes.POINTER(term), i, vp]),
        "rtv_lora_dora_workspace_bytes": (sz, [i, i]),
        "rtv_lora_merge_dora": (i, [vp, i, vp, i, i, i, vp, vp, i, f, vp, f, vp, sz, vp])}
    others = [n for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "LORA_EXT_PROTOTYPES"]
    assert "LORA_PROTOTYPES" in others and "PROTOTYPES" in others
    for n in others:
        assert not set(getattr(_lib, n)) & set(_lib.LORA_EXT_PROTOTYPES), n
    for n in [n for n in dir(_lib) if n.endswith("STRUCTS") and n != "LORA_EXT_STRUCTS"]:
        assert not set(getattr(_lib, n)) & set(_lib.LORA_EXT_STRUCTS), n
    # the first header is as it was
    assert list(_lib.LORA_STRUCTS) == ["rtv_lora_adapter"] and list(_lib.LORA_PROTOTYPES) == ["rtv_lora_merge"]


def test_library_exports_the_three_symbols_with_the_parsed_prototypes():
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.LORA_EXT_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_dora_workspace_bytes():
    ws = _lib.load().rtv_lora_dora_workspace_bytes
    assert ws(64, 128) == 256 and ws(64, 129) == 512 and ws(1, 8) == 16 and ws(5120, 13824) == 5120 * 108 * 4
    assert ws(0, 128) == 0 and ws(64, 0) == 0 and ws(-1, -1) == 0


# ------------------------------------------------------------------ refusals (no launch happens: the pointers are never followed)
P = 0x10000          # a 16-byte aligned non-null "device address"
LOW = (P, P, 8, 1.0, None, 0, 0.0)          # a term with a low-rank pair only


def _ex(base=P, ldb=64, W=P, ldw=64, N=16, K=64, terms=(LOW,), count=None, table=True):
    Term = _lib.LORA_EXT_STRUCTS["rtv_lora_term"]
    arr = (Term * max(1, len(terms)))(*[Term(*t) for t in terms])
    lib = _lib.load()
    status = lib.rtv_lora_merge_ex(base, ldb, W, ldw, N, K, arr if table else None, len(terms) if count is None else count, None)
    return status, lib.rtv_last_error().decode()


@pytest.mark.parametrize("kwargs, word", [
    # those of rtv_lora_merge
    (dict(base=None), "null"), (dict(W=None), "null"), (dict(table=False), "null"),
    (dict(terms=((None, P, 8, 1.0, None, 0, 0.0),)), "null"), (dict(terms=((P, None, 8, 1.0, None, 0, 0.0),)), "null"),
    (dict(N=0), "positive"), (dict(N=-3), "positive"), (dict(K=0), "positive"),
    (dict(base=P + 8), "misaligned"), (dict(W=P + 2), "misaligned"), (dict(terms=((P + 8, P, 8, 1.0, None, 0, 0.0),)), "misaligned"),
    (dict(terms=((P, P + 1, 8, 1.0, None, 0, 0.0),)), "misaligned"),
    (dict(K=60, ldb=64, ldw=64), "misaligned"), (dict(ldb=68), "misaligned"), (dict(ldw=100), "misaligned"),
    (dict(ldb=56), "stride"), (dict(ldw=8), "stride"),
    (dict(count=-1), "count"), (dict(count=5), "count"),
    (dict(terms=((P, P, 257, 1.0, None, 0, 0.0),)), "rank"), (dict(terms=((P, P, -1, 1.0, None, 0, 0.0),)), "rank"),
    (dict(terms=((P, P, 0, 1.0, None, 0, 0.0),)), "rank"),          # pointers with rank 0: half a pair, not a diff-only term
    (dict(terms=((P, P, 8, math.inf, None, 0, 0.0),)), "finite"), (dict(terms=((P, P, 8, math.nan, None, 0, 0.0),)), "finite"),
    (dict(terms=(LOW, (P, P, 8, -math.inf, None, 0, 0.0))), "finite"),
    # the new ones
    (dict(terms=((None, None, 0, 1.0, None, 64, 1.0),)), "neither"), (dict(terms=(LOW, (None, None, 0, 0.0, None, 0, 0.0))), "neither"),
    (dict(terms=((None, None, 0, 0.0, P + 8, 64, 1.0),)), "misaligned"), (dict(terms=((None, None, 0, 0.0, P, 68, 1.0),)), "misaligned"),
    (dict(terms=((None, None, 0, 0.0, P, 56, 1.0),)), "stride"), (dict(terms=((P, P, 8, 1.0, P, 8, 1.0),)), "stride"),
    (dict(terms=((None, None, 0, 0.0, P, 64, math.inf),)), "finite"), (dict(terms=((P, P, 8, 1.0, P, 64, math.nan),)), "finite"),
])
def test_merge_ex_refuses_before_any_launch(kwargs, word):
    status, msg = _ex(**kwargs)
    assert status != 0 and msg.startswith("lora_merge_ex") and word in msg, (status, msg)


def _dora(base=P, ldb=64, W=P, ldw=64, N=16, K=64, A=P, B=P, rank=8, factor=1.0, mag=P, strength=1.0, ws=P, ws_bytes=64):
    lib = _lib.load()
    status = lib.rtv_lora_merge_dora(base, ldb, W, ldw, N, K, A, B, rank, factor, mag, strength, ws, ws_bytes, None)
    return status, lib.rtv_last_error().decode()


@pytest.mark.parametrize("kwargs, word", [
    (dict(base=None), "null"), (dict(W=None), "null"), (dict(A=None), "null"), (dict(B=None), "null"),
    (dict(N=0), "positive"), (dict(K=-8), "positive"),
    (dict(base=P + 8), "misaligned"), (dict(W=P + 2), "misaligned"), (dict(A=P + 8), "misaligned"), (dict(B=P + 1), "misaligned"),
    (dict(K=60), "misaligned"), (dict(ldb=68), "misaligned"), (dict(ldw=100), "misaligned"),
    (dict(ldb=56), "stride"), (dict(ldw=8), "stride"),
    (dict(rank=0), "rank"), (dict(rank=257), "rank"),
    (dict(mag=None), "null"), (dict(mag=P + 1), "misaligned"),
    (dict(ws=None), "null"), (dict(ws=P + 4), "misaligned"), (dict(ws_bytes=63), "small"), (dict(K=136, ldb=136, ldw=136, ws_bytes=64), "small"),
    (dict(factor=math.inf), "factor"), (dict(factor=math.nan), "finite"), (dict(strength=-math.inf), "strength"),
    (dict(strength=math.nan), "finite"),
])
def test_merge_dora_refuses_before_any_launch(kwargs, word):
    status, msg = _dora(**kwargs)
    assert status != 0 and msg.startswith("lora_merge_dora") and word in msg, (status, msg)


# ------------------------------------------------------------------ the criterion, on the kernels' arithmetic in torch
@pytest.fixture(scope="module")
def inputs():
    return {(N, K, rank): xo.make_inputs(N, K, [rank], seed=N + rank) for N, K, rank, _ in xo.SHAPES}


@pytest.mark.parametrize("N, K, rank, strength", xo.SHAPES)
def test_dora_emulation_with_tile_partials_meets_the_criterion(inputs, N, K, rank, strength):
    base, [(A, B)], mag, _ = inputs[(N, K, rank)]
    factor = 8.0 / rank
    ref, bound_mag = xo.dora_oracle(base, A, B, factor, mag, strength)
    W = xo.dora_emulation(base, A, B, factor, mag, strength)
    lo.assert_meets(W, ref, bound_mag, f"dora emulation {N}x{K} r{rank}")
    # not vacuous: the norm over the wrong axis (rows scaled by 2^(n % 5)), a missing blend, or the base itself fail it
    V = base.float() + factor * (B.float() @ A.float())
    wrong_axis = (base.float() + strength * (mag.float()[:, None] / V.norm(dim=0, keepdim=True).clamp(min=1e-20) * V - base.float())).to(BF)
    assert lo.criterion(wrong_axis, ref, bound_mag)[0] < 0.5
    if strength != 1.0:
        assert lo.criterion(xo.dora_emulation(base, A, B, factor, mag, 1.0), ref, bound_mag)[0] < 0.5
    assert lo.criterion(base, ref, bound_mag)[0] < 0.5


@pytest.mark.parametrize("N, K, rank, scale", xo.SHAPES)
def test_dense_emulation_meets_the_criterion(inputs, N, K, rank, scale):
    base, [(A, B)], _, diff = inputs[(N, K, rank)]
    terms = [(A, B, scale, diff, -1.3 * scale)]
    ref, mag = xo.merge_ex_oracle(base, terms)
    lo.assert_meets(xo.ex_emulation(base, terms), ref, mag, f"dense emulation {N}x{K} r{rank}")
    assert lo.criterion(xo.ex_emulation(base, [(A, B, scale, None, 0.0)]), ref, mag)[0] < 0.5          # the diff forgotten
    assert lo.criterion(xo.ex_emulation(base, [(None, None, 0.0, diff, -1.3 * scale)]), ref, mag)[0] < 0.5   # the pair forgotten


def test_oracle_special_rows():
    base, [(A, B)], mag, _ = xo.make_inputs(8, 16, [4], seed=1)
    base[3] = 0
    B[3] = 0
    ref, _ = xo.dora_oracle(base, A, B, 1.0, mag, 1.0)
    assert torch.equal(ref[3], base[3].double())                                   # a zero row stays
    assert torch.equal(xo.dora_oracle(base, A, B, 1.0, mag, 0.0)[0], base.double())   # strength 0 is the base
    assert torch.equal(xo.dora_emulation(base, A, B, 1.0, mag, 0.0).view(torch.int16), base.view(torch.int16))


# ------------------------------------------------------------------ parser
def _model():
    from realtime_video_amd.causal_model import CausalWanModel
    return CausalWanModel(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, device="cpu")


@pytest.fixture(scope="module")
def shapes():
    return _model().state_dict_shapes()


@pytest.fixture(scope="module")
def adapter(shapes):
    return xo.full_adapter(shapes)


def _parse(sd, shapes, **kw):
    from realtime_video_amd.lora import parse_lora_state_dict
    return parse_lora_state_dict(sd, shapes, extended=True, **kw)


def _same_targets(a, b):
    assert a.keys() == b.keys()
    for t in a:
        x, y = a[t], b[t]
        assert type(x)._fields == type(y)._fields
        for f in type(x)._fields:
            u, v = getattr(x, f), getattr(y, f)
            assert (torch.equal(u, v) if torch.is_tensor(u) else u == v), (t, f)


def test_full_adapter_maps_onto_every_target(shapes, adapter):
    targets, unexpected = _parse(xo.spell(adapter, "canonical"), shapes)
    linears, norms = xo.all_targets()
    assert unexpected == [] and sorted(targets) == sorted(linears + norms) and len(targets) == 36
    t = targets["blocks.1.self_attn.v"]
    assert (t.tensor, t.row0, t.rows, t.cols, t.rank, t.factor) == ("L1.qkv_w", 512, 256, 256, 4, 1.0)
    assert (t.bias, t.bias0, t.bias_n) == ("L1.qkv_b", 512, 256) and t.diff is None and t.dora is None and t.diff_b.shape == (256,)
    t = targets["blocks.0.ffn.2"]
    assert (t.tensor, t.rows, t.cols, t.factor, t.bias) == ("L0.ffn2_w", 256, 512, 0.5, "L0.ffn2_b") and t.diff.shape == (256, 512)
    t = targets["blocks.0.self_attn.k"]
    assert t.dora.shape == (256,) and torch.equal(t.dora, adapter["blocks.0.self_attn.k.dora"])
    t = targets["blocks.1.cross_attn.norm_k"]
    assert (t.tensor, t.row0, t.rows, t.cols, t.rank, t.A, t.B, t.bias) == ("L1.cnorm_k_w", 0, 1, 256, 0, None, None, None)
    assert t.diff.shape == (256,)
    t = targets["blocks.1.norm3"]
    assert (t.tensor, t.bias, t.bias0, t.bias_n) == ("L1.norm3_w", "L1.norm3_b", 0, 256) and t.diff_b.shape == (256,)
    for name, (tensor, rows, cols) in {"text_embedding.0": ("text0", 256, 64), "text_embedding.2": ("text2", 256, 256),
                                       "time_embedding.0": ("time0", 256, 256), "time_embedding.2": ("time2", 256, 256),
                                       "time_projection.1": ("tproj", 1536, 256), "head.head": ("head", 64, 256)}.items():
        t = targets[name]
        assert (t.tensor, t.row0, t.rows, t.cols, t.bias, t.bias_n) == (tensor + "_w", 0, rows, cols, tensor + "_b", rows)


@pytest.mark.parametrize("prefix", xo.PREFIXES)
@pytest.mark.parametrize("style", xo.STYLES)
def test_every_prefix_and_style_gives_the_canonical_targets(shapes, adapter, prefix, style):
    want, _ = _parse(xo.spell(adapter, "canonical"), shapes)
    sd = xo.spell(adapter, style, prefix)
    if style == "diffusers":
        assert prefix + "blocks.0.attn1.to_out.0.lora_A.weight" in sd and prefix + "blocks.1.norm2.diff_b" in sd
        assert prefix + "condition_embedder.time_proj.lora_B.weight" in sd and prefix + "proj_out.diff" in sd
    if style == "kohya":
        assert prefix + "lora_unet_blocks_0_self_attn_q.lora_down.weight" in sd and prefix + "lora_unet_head_head.alpha" not in sd
    got, unexpected = _parse(sd, shapes)
    assert unexpected == []
    _same_targets(got, want)


def test_a_flattened_name_for_every_target_in_both_spellings(shapes):
    from realtime_video_amd.lora import flattened_names
    flat = flattened_names(shapes)
    linears, norms = xo.all_targets()
    for t in linears + norms:
        assert flat[t.replace(".", "_")] == t and flat[xo.to_diffusers(t).replace(".", "_")] == t
        part = ".diff" if t in norms else ".lora_down.weight"
        for spelling in (t, xo.to_diffusers(t)):
            sd = {"lora_unet_" + spelling.replace(".", "_") + part: torch.zeros(shapes[t + ".weight"][-1:] if t in norms else (4, shapes[t + ".weight"][1]))}
            if t not in norms:
                sd["lora_unet_" + spelling.replace(".", "_") + ".lora_up.weight"] = torch.zeros(shapes[t + ".weight"][0], 4)
            targets, unexpected = _parse(sd, shapes)
            assert list(targets) == [t] and unexpected == []
    assert len(flat) == 2 * 36              # every target is spelled differently by diffusers
    # nothing is found by splitting: a name that is no target stays unexpected
    _, unexpected = _parse({"lora_unet_blocks_0_self_attn_q_extra.lora_down.weight": torch.zeros(4, 256)}, shapes, strict=False)
    assert unexpected == ["lora_unet_blocks_0_self_attn_q_extra.lora_down.weight"]


@pytest.mark.parametrize("dora_key", [".dora_scale", ".lora_magnitude_vector", ".lora_magnitude_vector.weight"])
@pytest.mark.parametrize("column", [False, True])
def test_dora_key_spellings_and_shapes(shapes, adapter, dora_key, column):
    want, _ = _parse(xo.spell(adapter, "canonical"), shapes)
    got, unexpected = _parse(xo.spell(adapter, "canonical", dora_key=dora_key, column=column), shapes)
    assert unexpected == []
    _same_targets(got, want)
    assert sum(t.dora is not None for t in got.values()) == 3


def _pair(target="blocks.0.self_attn.q", out_f=256, in_f=256, r=4):
    return {target + ".lora_A.weight": torch.zeros(r, in_f), target + ".lora_B.weight": torch.zeros(out_f, r)}


@pytest.mark.parametrize("sd, words", [
    # what the default parser rejects
    ({"blocks.0.self_attn.q.lora_A.weight": torch.zeros(4, 256)}, ["blocks.0.self_attn.q.lora_A.weight"]),
    ({"lora_unet_blocks_0_ffn_0.alpha": torch.tensor(4.0)}, ["lora_unet_blocks_0_ffn_0.alpha"]),
    ({"head.head.lora_A.weight": torch.zeros(4, 512), "head.head.lora_B.weight": torch.zeros(64, 4)}, ["head.head.lora_A.weight"]),
    ({"transformer.proj_out.lora_A.weight": torch.zeros(4, 256), "transformer.proj_out.lora_B.weight": torch.zeros(256, 4)},
     ["transformer.proj_out.lora_B.weight"]),
    ({"blocks.1.cross_attn.o.lora_A.weight": torch.zeros(257, 256), "blocks.1.cross_attn.o.lora_B.weight": torch.zeros(256, 257)},
     ["cross_attn.o.lora_A.weight"]),
    ({**_pair(), "blocks.0.self_attn.q.alpha": torch.ones(2)}, ["blocks.0.self_attn.q.alpha"]),
    # two keys for one slot: both named
    ({**_pair(), "blocks.0.attn1.to_q.lora_A.weight": torch.zeros(4, 256)},
     ["blocks.0.self_attn.q.lora_A.weight", "blocks.0.attn1.to_q.lora_A.weight"]),
    ({**_pair(), "lora_unet_blocks_0_self_attn_q.lora_up.weight": torch.zeros(256, 4)},
     ["blocks.0.self_attn.q.lora_B.weight", "lora_unet_blocks_0_self_attn_q.lora_up.weight"]),
    ({"blocks.0.norm3.diff": torch.zeros(256), "diffusion_model.blocks.0.norm2.diff": torch.zeros(256)},
     ["'blocks.0.norm3.diff'", "diffusion_model.blocks.0.norm2.diff"]),
    ({**_pair(), "blocks.0.self_attn.q.dora_scale": torch.ones(256), "blocks.0.self_attn.q.lora_magnitude_vector": torch.ones(256)},
     ["blocks.0.self_attn.q.dora_scale", "blocks.0.self_attn.q.lora_magnitude_vector"]),
    # a DoRA vector without its pair
    ({"blocks.0.ffn.0.dora_scale": torch.ones(512)}, ["blocks.0.ffn.0.dora_scale", "pair"]),
    ({"blocks.0.ffn.0.dora_scale": torch.ones(512), "blocks.0.ffn.0.diff": torch.zeros(512, 256)}, ["blocks.0.ffn.0.dora_scale", "pair"]),
    # DoRA shapes: the per-input-column form is named as such, also where in == out
    ({**_pair("blocks.0.ffn.0", 512, 256), "blocks.0.ffn.0.dora_scale": torch.ones(1, 256)}, ["blocks.0.ffn.0.dora_scale", "per-input-column"]),
    ({**_pair(), "blocks.0.self_attn.q.dora_scale": torch.ones(1, 256)}, ["blocks.0.self_attn.q.dora_scale", "per-input-column"]),
    ({**_pair(), "blocks.0.self_attn.q.lora_magnitude_vector": torch.ones(255)}, ["blocks.0.self_attn.q.lora_magnitude_vector", "does not fit"]),
    # wrong-shape deltas
    ({"blocks.0.ffn.0.diff": torch.zeros(256, 512)}, ["blocks.0.ffn.0.diff", "does not fit"]),
    ({"blocks.0.ffn.0.diff_b": torch.zeros(256)}, ["blocks.0.ffn.0.diff_b", "does not fit"]),
    ({"blocks.0.self_attn.norm_q.diff": torch.zeros(1, 256)}, ["blocks.0.self_attn.norm_q.diff", "does not fit"]),
    ({"blocks.0.norm3.diff_b": torch.zeros(128)}, ["blocks.0.norm3.diff_b", "does not fit"]),
    ({"lora_unet_proj_out.diff": torch.zeros(64, 128)}, ["lora_unet_proj_out.diff", "does not fit"]),
    # alpha
    ({**_pair(), "blocks.0.self_attn.q.alpha": torch.tensor(math.inf)}, ["blocks.0.self_attn.q.alpha", "finite"]),
    ({**_pair(), "blocks.0.self_attn.q.alpha": torch.tensor(math.nan)}, ["blocks.0.self_attn.q.alpha", "finite"]),
])
def test_extended_parser_errors_name_the_key(shapes, sd, words):
    with pytest.raises(ValueError) as e:
        _parse(sd, shapes)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("key", [
    "patch_embedding.lora_A.weight", "patch_embedding.diff", "blocks.0.modulation.diff", "head.modulation.diff",
    "blocks.0.self_attn.norm_q.lora_A.weight", "blocks.0.self_attn.norm_q.diff_b", "blocks.0.norm1.diff", "blocks.2.self_attn.q.diff",
    "blocks.0.ffn.1.lora_A.weight", "blocks.0.self_attn.q.weight", "lora_unet_blocks_0_ffn_1.lora_down.weight",
    "lora_unet_blocks_0_self_attn_q.weight", "text_embedding.1.diff", "lora_te_text_model_encoder.lora_down.weight",
])
def test_unexpected_keys_strict_against_non_strict(shapes, key):
    sd = {**_pair(), key: torch.zeros(4, 256)}
    with pytest.raises(ValueError, match="unexpected"):
        _parse(sd, shapes)
    targets, unexpected = _parse(sd, shapes, strict=False)
    assert list(targets) == ["blocks.0.self_attn.q"] and unexpected == [key]


@pytest.mark.parametrize("style", xo.STYLES)
def test_default_parser_is_as_it_was(shapes, adapter, style):
    """extended=False (the default): the same dicts behave as before - every new key is unexpected, the old dialect parses
    into Targets whose leading fields are the old ones."""
    from realtime_video_amd.lora import parse_lora_state_dict
    sd = xo.spell(adapter, style, "transformer." if style == "diffusers" else "")
    with pytest.raises(ValueError, match="unexpected"):
        parse_lora_state_dict(sd, shapes)
    targets, unexpected = parse_lora_state_dict(sd, shapes, strict=False)
    old = {k for k in sd if style == "canonical" and k.startswith("blocks.") and ".norm" not in k
           and k.endswith((".lora_A.weight", ".lora_B.weight", ".alpha"))}
    assert sorted(unexpected) == sorted(set(sd) - old) and len(targets) == (20 if style == "canonical" else 0)
    for t in targets.values():
        assert t._fields[:8] == ("tensor", "row0", "rows", "cols", "rank", "factor", "A", "B")
        assert (t.diff, t.diff_b, t.bias, t.dora) == (None, None, None, None)


# ------------------------------------------------------------------ CPU model
def test_cpu_model_validates_an_extended_dict_and_refuses_to_merge(adapter):
    m = _model()
    sd = xo.spell(adapter, "kohya")
    with pytest.raises(ValueError, match="unexpected"):
        m.load_lora(sd)                                          # the default dialect does not know these keys
    with pytest.raises(ValueError, match="unexpected"):
        m.load_lora({**sd, "lora_unet_patch_embedding.diff": torch.zeros(4)}, extended=True)
    with pytest.raises(ValueError, match="per-input-column"):
        m.load_lora({**sd, "lora_unet_blocks_0_self_attn_k.dora_scale": torch.ones(1, 256)}, extended=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.load_lora(sd, extended=True)
    assert m.lora_adapters() == {} and m.lora_version == 0 and m._lora_base == {}
