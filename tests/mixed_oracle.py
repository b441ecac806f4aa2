"""The oracle graph under a per-Linear precision policy (CausalWanModel.set_linear_precision): a dispatcher for
`monkeypatch.setattr(wan_oracle, "fp8_linear", ...)` that recognises each Linear by its weight tensor and evaluates it with the
restatement of that Linear's mode - the ones the tests of the pure modes install for the whole model:

    bf16        torch.nn.functional.linear
    fp8         oracle/wan_oracle.fp8_linear (the function the dispatcher replaces, taken before it is replaced)
    fp8_row     tests/fp8_rows_oracle.fp8_rows_linear
    mxfp4/6     tests/mxfp4_oracle.mx_linear, tests/mxfp6_oracle.mx_linear (tests/mx_oracle.py)
    *_rot       tests/mx_rotate_oracle.mx_linear_rot of the format

With weights[wan_oracle.FP8_FLAG] = True the oracle sends every nn.Linear through `fp8_linear`, the fused [3d, d] qkv weight as one
call; the Conv3d patch embedding never arrives here."""
import torch
import torch.nn.functional as F

import fp8_rows_oracle
import mx_rotate_oracle
import mxfp4_oracle
import mxfp6_oracle

TOP = {"text_embedding.0": "text0", "text_embedding.2": "text2", "time_embedding.0": "time0", "time_embedding.2": "time2",
       "time_projection.1": "tproj", "head.head": "head"}
LAYER = {"self_attn.q": "qkv", "self_attn.o": "o", "cross_attn.q": "cq", "cross_attn.k": "ck", "cross_attn.v": "cv", "cross_attn.o": "co",
         "ffn.0": "ffn0", "ffn.2": "ffn2"}


def linear_weights(weights, num_layers):
    """{policy key: the weight tensor of the oracle's weights dict that identifies it} - for qkv the q block, the first d rows of the
    fused weight."""
    out = {key: weights[name + ".weight"] for name, key in TOP.items()}
    for l in range(num_layers):
        out.update({f"L{l}.{key}": weights[f"blocks.{l}.{name}.weight"] for name, key in LAYER.items()})
    return out


def _fingerprint(row):
    return row.detach().float().cpu().numpy().tobytes()


def dispatcher(wo, weights, num_layers, modes):
    """-> (linear(x, weight, bias, shards=1) for wan_oracle.fp8_linear, the list of policy keys it has served, in call order).
    `modes`: {policy key: mode name} for every Linear (CausalWanModel.linear_precision()).  A weight that is none of the model's
    Linears raises."""
    restatement = {"bf16": lambda x, w_, b, shards=1: F.linear(x, w_, b), "fp8": wo.fp8_linear, "fp8_row": fp8_rows_oracle.fp8_rows_linear,
                   "mxfp4": mxfp4_oracle.mx_linear, "mxfp6": mxfp6_oracle.mx_linear,
                   "mxfp4_rot": mx_rotate_oracle.mx_linear_rot(mxfp4_oracle), "mxfp6_rot": mx_rotate_oracle.mx_linear_rot(mxfp6_oracle)}
    refs = linear_weights(weights, num_layers)
    assert set(refs) == set(modes)
    by_row = {}
    for key, ref in refs.items():
        by_row.setdefault((ref.shape[1], _fingerprint(ref[0])), []).append(key)
    assert all(len(v) == 1 for v in by_row.values()), "two Linears share their first weight row: the dispatcher cannot tell them apart"
    served = []

    def linear(x, weight, bias, shards=1):
        hit = by_row.get((weight.shape[1], _fingerprint(weight[0])))
        if not hit:
            raise AssertionError(f"mixed oracle: a Linear with an unknown weight {tuple(weight.shape)}")
        key, = hit
        ref = refs[key]
        assert weight.shape[0] == (3 if key.endswith(".qkv") else 1) * ref.shape[0]
        assert torch.equal(weight[:ref.shape[0]].detach().float().cpu(), ref.detach().float().cpu()), key      # the whole block, not its first row alone
        served.append(key)
        return restatement[modes[key]](x, weight, bias, shards)

    return linear, served
