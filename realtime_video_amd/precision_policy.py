"""Per-Linear precision policy of the DiT (CausalWanModel.set_linear_precision; rtv_dit_config.use_fp8 == 7 and the mode table
behind rtv_dit_weights.fp8_row_scales, include/rtv_hip.h).  Pure Python: no GPU, no library - the resolver turns a policy into the
list of mode numbers the native side reads, in the order of rtv_dit_weights.fp8_scales.

A policy is a dict.  Its values are mode names:

    "bf16", "fp8" (one scale per tensor), "fp8_row" (one per row), "mxfp4", "mxfp6", "mxfp4_rot", "mxfp6_rot"

Its keys, from the weakest to the strongest:

    "default"                       every Linear no other key names ("bf16" when absent)
    a Linear kind                   "text0", "text2", "time0", "time2", "tproj", "head" (one Linear each) and, in every layer,
                                    "qkv", "o", "cq", "ck", "cv", "co", "ffn0", "ffn2"
    "L<l>.<kind>"                   that Linear of layer l alone, e.g. "L0.ffn0"
"""
import re

MODE_NAMES = ("bf16", "fp8", "fp8_row", "mxfp4", "mxfp6", "mxfp4_rot", "mxfp6_rot")       # index = the value of rtv_dit_config.use_fp8
MIXED = 7                                                                                   # use_fp8: one mode per Linear
TOP_KINDS = ("text0", "text2", "time0", "time2", "tproj", "head")
LAYER_KINDS = ("qkv", "o", "cq", "ck", "cv", "co", "ffn0", "ffn2")
# what a Linear's input width must be a multiple of, per mode (enable_fp8 / enable_mxfp4 / enable_mxfp6 ask the same of every width)
K_MULTIPLE = (1, 128, 128, 256, 128, 256, 128)


def linear_names(num_layers):
    """The Linears in the order of rtv_dit_weights.fp8_scales: the six top-level ones, then eight per layer."""
    return list(TOP_KINDS) + [f"L{l}.{k}" for l in range(num_layers) for k in LAYER_KINDS]


def linear_widths(dim, ffn_dim, text_dim, freq_dim):
    """{kind: input width} of this architecture's Linears."""
    w = {k: dim for k in TOP_KINDS + LAYER_KINDS}
    w.update(text0=text_dim, time0=freq_dim, ffn2=ffn_dim)
    return w


def resolve(policy, num_layers, widths=None):
    """policy, number of layers -> [mode number per Linear] in the order of linear_names().  Precedence: "L<l>.<kind>" over "<kind>"
    over "default".  `widths` ({kind: input width}, linear_widths()): when given, a Linear whose width its mode cannot take is a
    ValueError that names it - as are unknown keys, unknown mode names and layer indices out of range."""
    if not isinstance(policy, dict):
        raise ValueError(f"a precision policy is a dict of Linear -> mode name, got {type(policy).__name__}")
    modes = {}
    for key, name in policy.items():
        if name not in MODE_NAMES:
            raise ValueError(f"precision policy: unknown mode {name!r} for {key!r} (one of {', '.join(MODE_NAMES)})")
        modes[key] = MODE_NAMES.index(name)
        if key == "default" or key in TOP_KINDS or key in LAYER_KINDS:
            continue
        m = re.fullmatch(r"L(\d+)\.(\w+)", key) if isinstance(key, str) else None
        if not m or m.group(2) not in LAYER_KINDS:
            raise ValueError(f"precision policy: unknown key {key!r} ('default', a Linear kind - {', '.join(TOP_KINDS + LAYER_KINDS)} - "
                             "or 'L<layer>.<kind>' for a kind of the layers)")
        if int(m.group(1)) >= num_layers:
            raise ValueError(f"precision policy: {key!r} names layer {int(m.group(1))} of a model with {num_layers} layers")
        modes[f"L{int(m.group(1))}.{m.group(2)}"] = modes.pop(key)      # ("L01.qkv" is "L1.qkv")
    default = modes.get("default", 0)
    out = [modes.get(name, modes.get(name.split(".")[-1], default)) for name in linear_names(num_layers)]
    if widths is not None:
        check_widths(out, num_layers, widths, "precision policy")
    return out


def check_widths(modes, num_layers, widths, who):
    """ValueError, in the name of `who`, for the first Linear whose input width (`widths`: linear_widths()) its mode cannot take."""
    for name, mode in zip(linear_names(num_layers), modes):
        width = widths[name.split(".")[-1]]
        if width % K_MULTIPLE[mode]:
            raise ValueError(f"{who}: {name} has input width {width}, {MODE_NAMES[mode]} needs a multiple of {K_MULTIPLE[mode]}")


def named(modes, num_layers):
    """[mode number per Linear] -> {Linear: mode name}, in the order of linear_names()."""
    return {n: MODE_NAMES[m] for n, m in zip(linear_names(num_layers), modes)}
