"""Native text encoder (rtv_t5_encode behind realtime_video_amd.text_encoder.WanTextEncoder) vs the CPU oracle and the
golden minted from the reference's T5Encoder.  Tolerance: the reference computes in float32; here the
linears take bf16-rounded activations (weights are exact, accumulation / residual stream / norms / softmax float32), so the
result differs by bf16 input rounding only: rel-L2 <= 1e-2, max-abs <= 5e-2 on outputs of magnitude ~1."""
import pytest
import torch

from conftest import max_abs, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _encoder(cfg, w, text_len):
    from realtime_video_amd.text_encoder import WanTextEncoder
    enc = WanTextEncoder(device=DEV, text_len=text_len, **cfg)
    enc.load_state_dict(w)
    return enc


def test_text_encoder_matches_reference_golden(golden):
    from oracle import t5_oracle as to
    gold = golden("t5_encoder.pt")
    cfg = dict(to.TINY_T5)
    w = to.make_t5_weights(cfg, seed=0)
    enc = _encoder(cfg, w, text_len=48)
    out = enc.encode_ids(gold["ids"], gold["mask"])["prompt_embeds"]
    assert out.shape == (2, 48, cfg["dim"]) and out.dtype == torch.float32
    ref = gold["prompt_embeds"]
    assert rel_l2(out.cpu(), ref) <= 1e-2 and max_abs(out.cpu(), ref) <= 5e-2
    assert float(out[0, 29:].abs().max()) == 0.0          # padding rows are exactly zero (wan_wrapper.py:52-53)


@pytest.mark.parametrize("lens", [(512, 77), (1, 33, 300)])
def test_text_encoder_full_window_matches_oracle(lens):
    """512-slot window (the production text_len): every relative distance up to +-511, multi-block key loops, a one-token
    prompt, lengths that are not multiples of 32; 4 heads, 3 layers."""
    from oracle import t5_oracle as to
    cfg = dict(to.TINY_T5, num_heads=4, dim_attn=256, num_layers=3, vocab=300)
    w = to.make_t5_weights(cfg, seed=3)
    ids, mask = to.t5_inputs(cfg, seed=11, L=512, lens=lens)
    ref = to.text_encoder_forward(w, ids, mask, cfg)["prompt_embeds"]
    enc = _encoder(cfg, w, text_len=512)
    out = enc.encode_ids(ids, mask)["prompt_embeds"].cpu()
    for b, n in enumerate(lens):
        assert rel_l2(out[b, :n], ref[b, :n]) <= 1e-2, (b, n)
        assert max_abs(out[b, :n], ref[b, :n]) <= 5e-2
        assert float(out[b, n:].abs().max() if n < 512 else 0.0) == 0.0


def test_zero_layers_is_the_final_norm_of_the_embedding():
    """num_layers = 0: the output is T5LayerNorm(embedding) in float32, held per element to the RMSNorm bar of tests/t5_cases.py."""
    import row_cases as rc
    import t5_cases as tc
    from oracle import t5_oracle as to
    cfg = dict(to.TINY_T5, num_layers=0)
    w = tc.bf16_checkpoint(to.make_t5_weights(cfg, seed=2))
    ids, mask = to.t5_inputs(cfg, seed=5, L=48, lens=(29, 48))
    out = _encoder(cfg, w, text_len=48).encode_ids(ids, mask)["prompt_embeds"].cpu()
    for b, n in enumerate((29, 48)):
        ref, worst = tc.rms64(w["token_embedding.weight"][ids[b, :n]], w["norm.weight"], 1e-6, out_f32=True)
        ok, ratio, where = rc.within(out[b, :n], ref, worst)
        print(f"T5_RATIO kernel=encode_0_layers family=embedding shape={n}x{cfg['dim']} ratio={ratio:.3f}")
        assert ok, (b, ratio, where)
        assert float(out[b, n:].abs().max() if n < 48 else 0.0) == 0.0


def test_padding_queries_never_leave_the_bias_table(golden):
    """text_len = 48 and a 48-token prompt: rows = 64 > max_len, so a padding query row q indexing the table at (max_len - 1) - q +
    key would read up to 16 floats in front of it.  Every layer's table is a copy inside a NaN-filled buffer here: such a read
    makes the padding row of the residual stream NaN, the next layer's V^T padding columns NaN, and 0 * NaN every valid row."""
    from oracle import t5_oracle as to
    gold = golden("t5_encoder.pt")
    cfg = dict(to.TINY_T5)
    enc = _encoder(cfg, to.make_t5_weights(cfg, seed=0), text_len=48)
    guards = []
    for i in range(cfg["num_layers"]):
        table = enc._t[f"blocks.{i}.pos_bias"]
        buf = torch.full((table.numel() + 512,), float("nan"), dtype=torch.float32, device=DEV)
        buf[256:256 + table.numel()] = table.flatten()
        enc._layers[i].pos_bias = buf[256:].data_ptr()
        guards.append(buf)
    out = enc.encode_ids(gold["ids"], gold["mask"])["prompt_embeds"].cpu()
    assert bool(torch.isfinite(out).all()), f"{int((~torch.isfinite(out)).sum())} non-finite output elements"
    ref = gold["prompt_embeds"]
    assert rel_l2(out, ref) <= 1e-2 and max_abs(out, ref) <= 5e-2


def test_24_layers_at_tiny_width_within_twice_the_rounding_emulation():
    """The model's depth at TINY_T5's width.  The bar is measured: t5_cases.encoder_chain with the native path's bf16 rounding points
    (the input of every linear, and its output where the native path stores bf16), run on the CPU, lies some distance from the fp64
    chain; the native path must lie within twice that - the margin takes the summation order, exp2f and tanhf, as in
    test_error_vs_fp32_gold_is_within_twice_the_reference_error for the DiT."""
    import t5_cases as tc
    from oracle import t5_oracle as to
    cfg = dict(to.TINY_T5, **tc.DEEP_T5)
    w = tc.bf16_checkpoint(to.make_t5_weights(cfg, seed=5))
    ids, mask = to.t5_inputs(cfg, seed=13, L=tc.DEEP_TEXT_LEN, lens=tc.DEEP_LENS)
    out = _encoder(cfg, w, text_len=tc.DEEP_TEXT_LEN).encode_ids(ids, mask)["prompt_embeds"].cpu()
    for b, n in enumerate(tc.DEEP_LENS):
        gold = tc.encoder_chain(w, ids[b, :n], cfg)
        emulated = tc.rel_l2(tc.encoder_chain(w, ids[b, :n], cfg, torch.float32, native=True), gold)
        native = tc.rel_l2(out[b, :n], gold)
        print(f"T5_DEEP tokens={n} layers=24 rel_l2_native={native:.4e} rel_l2_emulated={emulated:.4e} ratio={native / emulated:.3f}")
        assert native <= 2.0 * emulated, (n, native, emulated)


def test_text_encoder_api_errors():
    from oracle import t5_oracle as to
    from realtime_video_amd.text_encoder import WanTextEncoder
    cfg = dict(to.TINY_T5)
    w = to.make_t5_weights(cfg, seed=0)
    enc = _encoder(cfg, w, text_len=48)
    ids, mask = to.t5_inputs(cfg)
    with pytest.raises(RuntimeError):
        enc(["a prompt"])                                  # no tokenizer files offline
    bad = mask.clone()
    bad[0, 3] = 0
    with pytest.raises(ValueError):
        enc.encode_ids(ids, bad)
    with pytest.raises(KeyError):
        WanTextEncoder(device=DEV, text_len=48, **cfg).load_state_dict({k: v for k, v in w.items() if k != "norm.weight"})
    with pytest.raises(RuntimeError):
        WanTextEncoder(device=DEV, text_len=48, **cfg).encode_ids(ids, mask)
