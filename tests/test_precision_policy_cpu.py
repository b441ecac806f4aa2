"""The resolver of the per-Linear precision policy (realtime_video_amd/precision_policy.py): no GPU, no library."""
import pytest

from realtime_video_amd import precision_policy as pp

WIDTHS = pp.linear_widths(dim=256, ffn_dim=512, text_dim=256, freq_dim=256)


def test_order_is_that_of_the_scale_tables():
    from realtime_video_amd.causal_model import _FP8_LAYER, _FP8_TOP
    names = pp.linear_names(2)
    assert names[:6] == [k[:-2] for k in _FP8_TOP] and len(names) == 6 + 8 * 2
    assert names[6:14] == ["L0." + k[:-2] for k in _FP8_LAYER] and names[14:] == ["L1." + k[:-2] for k in _FP8_LAYER]
    # one distinct mode per position: the result is in that order
    policy = {"default": "bf16", "time0": "fp8", "head": "fp8_row", "L0.qkv": "mxfp4", "L0.ffn2": "mxfp6", "L1.o": "mxfp4_rot",
              "L1.ffn2": "mxfp6_rot"}
    modes = pp.resolve(policy, 2, WIDTHS)
    want = [0] * 22
    for key, mode in (("time0", 1), ("head", 2), ("L0.qkv", 3), ("L0.ffn2", 4), ("L1.o", 5), ("L1.ffn2", 6)):
        want[names.index(key)] = mode
    assert modes == want
    assert pp.MODE_NAMES == ("bf16", "fp8", "fp8_row", "mxfp4", "mxfp6", "mxfp4_rot", "mxfp6_rot") and pp.MIXED == 7
    assert pp.named(modes, 2)["L1.o"] == "mxfp4_rot" and list(pp.named(modes, 2)) == names


def test_precedence_layer_key_over_kind_over_default():
    modes = pp.named(pp.resolve({"default": "fp8_row", "ffn0": "mxfp4", "L1.ffn0": "mxfp6"}, 2, WIDTHS), 2)
    assert modes["L1.ffn0"] == "mxfp6" and modes["L0.ffn0"] == "mxfp4"
    assert all(v == "fp8_row" for k, v in modes.items() if not k.endswith("ffn0"))
    # whatever the order of the dict
    again = pp.named(pp.resolve({"L1.ffn0": "mxfp6", "ffn0": "mxfp4", "default": "fp8_row"}, 2, WIDTHS), 2)
    assert again == modes
    # no default: bf16
    modes = pp.named(pp.resolve({"head": "fp8"}, 2, WIDTHS), 2)
    assert modes.pop("head") == "fp8" and set(modes.values()) == {"bf16"}


def test_all_bf16_resolves_to_zeros():
    assert pp.resolve({}, 3, WIDTHS) == [0] * 30
    assert pp.resolve({"default": "bf16", "qkv": "bf16", "L2.co": "bf16"}, 3, WIDTHS) == [0] * 30


@pytest.mark.parametrize("policy,match", [
    ({"ffn1": "mxfp4"}, "unknown key 'ffn1'"),
    ({"L0.head": "fp8"}, "unknown key 'L0.head'"),                     # the top-level Linears belong to no layer
    ({"L0": "fp8"}, "unknown key 'L0'"),
    ({"qkv": "fp4"}, "unknown mode 'fp4'"),
    ({"default": 3}, "unknown mode 3"),
    ({"L2.qkv": "fp8"}, "layer 2 of a model with 2 layers"),
])
def test_unknown_keys_modes_and_layers_raise(policy, match):
    with pytest.raises(ValueError, match=match):
        pp.resolve(policy, 2, WIDTHS)


def test_width_errors_name_the_linear():
    w = pp.linear_widths(dim=384, ffn_dim=576, text_dim=256, freq_dim=128)
    with pytest.raises(ValueError, match=r"L0\.qkv has input width 384, mxfp4 needs a multiple of 256"):
        pp.resolve({"qkv": "mxfp4"}, 2, w)
    with pytest.raises(ValueError, match=r"time0 has input width 128, mxfp4_rot needs a multiple of 256"):
        pp.resolve({"time0": "mxfp4_rot"}, 2, w)
    with pytest.raises(ValueError, match=r"L1\.ffn2 has input width 576, mxfp6_rot needs a multiple of 128"):
        pp.resolve({"L1.ffn2": "mxfp6_rot"}, 2, w)
    with pytest.raises(ValueError, match=r"L0\.ffn2 has input width 576, mxfp6 needs a multiple of 128"):
        pp.resolve({"ffn2": "mxfp6"}, 2, w)
    # per Linear, not per model: the widths that fit are accepted beside ones that would not
    modes = pp.named(pp.resolve({"qkv": "mxfp6", "text0": "mxfp4", "time0": "mxfp6", "ffn2": "bf16", "L1.o": "fp8_row"}, 2, w), 2)
    assert modes["L1.qkv"] == "mxfp6" and modes["text0"] == "mxfp4" and modes["time0"] == "mxfp6" and modes["L0.ffn2"] == "bf16" and modes["L1.o"] == "fp8_row"
    assert pp.resolve({"qkv": "mxfp4"}, 2) == pp.resolve({"qkv": "mxfp4"}, 2, WIDTHS)      # no widths given: nothing to check
