"""The cases of tests/t5_w8_cases.py hold what they claim, without a GPU: every exact case satisfies its exactness condition and its
reference is the kernel's structure restated; every named slip changes at least one output of at least one case (so the bit-level
acceptance of tests/test_t5_w8_gpu.py would notice it); the K plan covers K exactly once; the new binding tables parse beside the
ABI's; enable_fp8_weights() refuses what it cannot do."""
import pytest
import torch

import t5_w8_cases as W

CPU_CASES = W.SMALL_CASES                # the ring and model cases build where the GPU test runs (their references are large)


@pytest.fixture(scope="module")
def built():
    return {c.name: W.build(c) for c in CPU_CASES}


def test_every_case_builds_exact_and_the_restated_kernel_equals_the_reference(built):
    for c in CPU_CASES:
        o = built[c.name]
        assert 0 < o.max_int < W.EXACT_MAX
        assert W.mismatches(W.emulate(c, o), W.reference(c, o)) == 0, c.name
    for c in W.RING_CASES + W.MODEL_CASES:
        assert 64 * c.K < W.EXACT_MAX                       # |a|, |w| <= 8: the condition holds for any draw


def test_cases_are_what_their_names_say():
    seg = {c.name: W.segment_steps(c.N, c.K) for c in W.EXACT_CASES}
    assert seg["k_one_step"] == [(0, 1)] and seg["k_two_steps"] == [(0, 2)] and seg["k_three_steps"] == [(0, 3)]
    assert seg["k_smallest_cut"] == [(0, 2), (2, 4)] and W.segments(W.STRIP, 3 * W.KSTEP) == 1
    assert seg["k_unequal_segments"] == [(0, 2), (2, 5)]
    assert [b - a for a, b in seg["k_four_segments"]] == [2, 2, 2, 3]
    assert {b - a for a, b in seg["ring_round_and_one"]} == {W.RING + 1} and {b - a for a, b in seg["ring_round_and_three"]} == {W.RING + 3}
    assert [len(seg[n]) for n in ("model_qk", "model_o", "model_v_t", "model_gate_fc1", "model_fc2")] == [4, 8, 8, 2, 8]
    assert {b - a for a, b in seg["model_fc2"]} == {10}
    assert W.by_name("m_160").M > W.CHUNK and W.by_name("n_ragged_strips").N % W.STRIP == 16
    assert sorted({c.M for c in W.M_CASES}) == [32, 64, 96, 128, 160, 512]


@pytest.mark.parametrize("slip", sorted(W.SLIPS))
def test_every_slip_changes_an_output(built, slip):
    changed = []
    for c in CPU_CASES:
        if W.slip_applies(c, slip):
            o = built[c.name]
            bad = W.mismatches(W.emulate(c, o, slip), W.reference(c, o))
            assert bad > 0, (slip, c.name)
            changed.append(c.name)
    dc, do = W.decode_table()
    if W.slip_applies(dc, slip, decode=True):
        assert W.mismatches(W.emulate(dc, do, slip), W.decode_reference(do)) > 0, (slip, "decode_table")
        changed.append(dc.name)
    assert changed, slip


def test_decode_table_holds_every_code_and_its_reference_is_the_restated_kernel():
    c, o = W.decode_table()
    assert W.mismatches(W.emulate(c, o), W.decode_reference(o)) == 0
    ref = W.decode_reference(o)
    vals = W.value(o.codes)
    assert float(vals.max()) == 448.0 and float(vals.min()) == -448.0
    assert int(((o.codes & 0x78) == 0).sum()) >= 14 * W.DECODE_N          # the subnormal codes, both signs, in every row
    where = (o.codes == 0x80).nonzero()
    assert len(where) == W.DECODE_N and all(W.bits(ref)[k, n] == 0 for n, k in where.tolist())     # -0 comes back as +0
    assert bool(torch.isfinite(ref.float()).all())


@pytest.mark.parametrize("K", W.ENCODER_WIDTHS + (128, 256, 512))
def test_plan_covers_k_exactly_once(K):
    for N in (16, 64, 128, 256, 1024, 4096, 8192, 20480):
        segs = W.segment_steps(N, K)
        assert segs[0][0] == 0 and segs[-1][1] == K // W.KSTEP
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:])) and all(b - a >= (2 if len(segs) > 1 else 1) for a, b in segs)
        assert len(segs) <= W.MAX_SEGMENTS


def test_restated_plan_is_the_library_plan():
    """rtv_gemm_w8_segments is host code: the restatement the cases are named by is the plan the launcher takes."""
    from realtime_video_amd import _lib
    lib = _lib.load()
    for N in (16, 48, 64, 80, 208, 1024, 4096, 8192, 20480, 32768):
        for K in (128, 256, 384, 512, 640, 1152, 4096, 5120, 7168, 10240):
            assert lib.rtv_gemm_w8_segments(N, K) == W.segments(N, K), (N, K)
            assert lib.rtv_gemm_w8_workspace_bytes(32, N, K) == (W.segments(N, K) * 32 * N * 4 if W.segments(N, K) > 1 else 0)
    assert lib.rtv_gemm_w8_segments(24, 128) == 0 and lib.rtv_gemm_w8_segments(64, 192) == 0 and lib.rtv_gemm_w8_workspace_bytes(48, 64, 512) == 0


def test_binding_tables_parse_and_leave_the_abi_tables_alone():
    from realtime_video_amd import _lib
    assert set(_lib.T5_W8_PROTOTYPES) == {"rtv_gemm_w8_workspace_bytes", "rtv_gemm_w8", "rtv_gemm_w8_segments",
                                          "rtv_t5_w8_workspace_bytes", "rtv_t5_encode_w8"}
    assert set(_lib.T5_W8_STRUCTS) == {"rtv_t5_layer_weights_w8", "rtv_t5_weights_w8"}
    assert not set(_lib.T5_W8_PROTOTYPES) & set(_lib.PROTOTYPES) and not set(_lib.T5_W8_STRUCTS) & set(_lib.STRUCTS)
    assert len(_lib.PROTOTYPES) == 90 and len(_lib.STRUCTS) == 14
    layer = _lib.T5_W8_STRUCTS["rtv_t5_layer_weights_w8"]
    assert [f for f, _ in layer._fields_] == ["norm1_w", "qk_q", "qk_s", "v_q", "v_s", "o_q", "o_s", "norm2_w", "gate_fc1_q",
                                              "gate_fc1_s", "fc2_q", "fc2_s", "pos_bias"]
    assert len(_lib.T5_W8_PROTOTYPES["rtv_gemm_w8"][1]) == 14 and len(_lib.T5_W8_PROTOTYPES["rtv_t5_encode_w8"][1]) == 9


def test_dequantised_state_dict_replaces_the_seven_matrices_only():
    import t5_cases as tc
    from oracle import t5_oracle as to
    cfg = dict(to.TINY_T5)
    w = tc.bf16_checkpoint(to.make_t5_weights(cfg, seed=0))
    dq = W.dequantised(w)
    assert set(dq) == set(w)
    for key in w:
        linear = key.startswith("blocks.") and key.split(".", 2)[2] in W.LINEAR_KEYS
        assert torch.equal(dq[key].double(), w[key].double()) != linear, key
        if linear:
            rel = float((dq[key] - w[key].double()).abs().max() / w[key].abs().max())
            assert 0 < rel <= 2.0 ** -4                    # e4m3: 3 mantissa bits, half an ulp of the row's largest element
    assert sum(1 for k in w if k.startswith("blocks.0.") and k.split(".", 2)[2] in W.LINEAR_KEYS) == 7


def test_enable_fp8_weights_refuses_an_unloaded_encoder_and_a_cpu_device():
    from oracle import t5_oracle as to
    from realtime_video_amd.text_encoder import WanTextEncoder
    cfg = dict(to.TINY_T5)
    enc = WanTextEncoder(device="cpu", text_len=48, **cfg)
    with pytest.raises(RuntimeError, match="not loaded"):
        enc.enable_fp8_weights()
    enc.load_state_dict(to.make_t5_weights(cfg, seed=0))
    with pytest.raises(RuntimeError, match="GPU only"):
        enc.enable_fp8_weights()
    assert enc.weight_bytes()["linears"] == 2 * cfg["num_layers"] * (4 * cfg["dim_attn"] * cfg["dim"] + 3 * cfg["dim_ffn"] * cfg["dim"])
