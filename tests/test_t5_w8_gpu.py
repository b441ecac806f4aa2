"""The text encoder's e4m3 weight storage on the device: rtv_gemm_w8 (csrc/gemm_w8.hip) on the integer cases, the decode table and
the row-locality problems of tests/t5_w8_cases.py - every comparison is equality of bit patterns - its argument refusals, and
WanTextEncoder.enable_fp8_weights() / rtv_t5_encode_w8 against the fp64 chain on the dequantised weights.
tests/test_t5_w8_cpu.py proves that each named slip of t5_w8_cases.SLIPS would break the equalities used here.

RTV_T5_W8_PARITY_RECORD=<path> writes the distances of the 24-layer test (profiles/r24_t5_w8_parity.txt is such a record)."""
import ctypes
import os

import pytest
import torch

import t5_cases as tc
import t5_w8_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
c_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def ops():
    from realtime_video_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def workspace():
    """One slab buffer for every launch of this module, NaN-filled once: a slab the reduction reads and nobody wrote shows."""
    return torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device=DEV)


def _run_guarded(ops, c, o, workspace):
    """The case through strided operands between NaN guards into a window of a sentinel-filled buffer."""
    a_buf, a = W.guarded_a(o.a, DEV)
    w_buf, codes = W.guarded_codes(o.codes, DEV)
    assert a.stride(0) == c.K + W.PAD_A and codes.stride(0) == c.K + W.PAD_W and a.data_ptr() % 16 == 0 and codes.data_ptr() % 16 == 0
    rows, cols = (c.N, c.M) if c.transpose else (c.M, c.N)
    buf, out = W.output_window(rows, cols, DEV)
    ops.gemm_w8(a, codes, o.s.to(DEV), out=out, transpose_out=c.transpose, workspace=workspace)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()), f"{c.name}: {int((~torch.isfinite(out.float())).sum())} outputs not finite"
    assert W.sentinels_changed(buf, cols) == 0, f"{c.name}: written outside the output window"
    return out


def _report(c, out, ref):
    bad = W.mismatches(out, ref)
    if not bad:
        return ""
    first = (W.bits(out.cpu()) != W.bits(ref.cpu())).reshape(-1).nonzero()[0].item()
    r, col = divmod(first, out.shape[1])
    return f"{c.name}: {bad} of {out.numel()} outputs differ; first at [{r}][{col}]: got {float(out[r, col])}, expected {float(ref[r, col])}"


@pytest.mark.parametrize("c", W.EXACT_CASES, ids=lambda c: c.name)
def test_exact_case_bit_for_bit(ops, workspace, c):
    """Every K depth (one step, two, an odd count, the smallest K the plan cuts, unequal segments, four segments, segments of a ring
    round and one / three steps), every N class (16, one strip, a strip and 16, ragged strips), every row count (32 .. 128, two row
    chunks, 512), both stores and the five shapes of the model at 32 rows: the output equals bf16(exact * s) bit for bit, twice on
    different data with one workspace (a stale slab shows), nothing outside the window is written."""
    big = c.N * c.K > 1 << 22
    for launch in ((0,) if big else (0, 1)):
        o = W.build(c, launch, DEV if big else "cpu")
        msg = _report(c, _run_guarded(ops, c, o, workspace), W.reference(c, o))
        assert not msg, f"launch {launch}: {msg}"


def test_decode_table_every_code_bit_for_bit(ops, workspace):
    """One-hot rows pick single codes: all 254 non-NaN codes in every weight row, subnormals, +-448, 0x80 as a zero."""
    c, o = W.decode_table()
    out = _run_guarded(ops, c, o, workspace)
    msg = _report(c, out, W.decode_reference(o))
    assert not msg, msg
    t = W.Case("decode_table_t", c.M, c.N, c.K, True)
    msg = _report(t, _run_guarded(ops, t, o, workspace), W.decode_reference(o).t().contiguous())
    assert not msg, msg


def test_device_output_differs_from_every_slipped_emulation(ops, workspace):
    """The other half of the CPU proof on the device's own output: equal to the reference, different from every applicable slip."""
    for name in ("k_unequal_segments", "k_unequal_segments_t", "m_160", "odd_scales"):
        c = W.by_name(name)
        o = W.build(c)
        out = _run_guarded(ops, c, o, workspace).cpu()
        assert W.mismatches(out, W.reference(c, o)) == 0
        for slip in W.SLIPS:
            if W.slip_applies(c, slip):
                assert W.mismatches(out, W.emulate(c, o, slip)) > 0, (name, slip)


@pytest.mark.parametrize("N,K", W.LOCALITY_SHAPES)
@pytest.mark.parametrize("transpose", [False, True])
def test_rows_are_local_and_launches_repeat(ops, workspace, N, K, transpose):
    """Gaussian data: the first 32 rows of a 96-row and a 160-row launch (one chunk of another height; two chunks) equal the 32-row
    launch bit for bit, and two runs of every launch agree bit for bit."""
    a, codes, s = (t.to(DEV) for t in W.gaussian_problem(N, K))
    outs = {}
    for M in W.LOCALITY_MS:
        runs = [ops.gemm_w8(a[:M], codes.view(W.E4), s, transpose_out=transpose, workspace=workspace) for _ in range(2)]
        torch.cuda.synchronize()
        assert W.mismatches(runs[0], runs[1]) == 0, M
        outs[M] = runs[0].t() if transpose else runs[0]
        # the problem is not degenerate: close to the float64 product of the same operands
        ref = (a[:M].double() @ W.value(codes).double().t()) * s.double()
        assert tc.rel_l2(outs[M], ref) <= 2.0 ** -8
    for M in W.LOCALITY_MS[1:]:
        assert W.mismatches(outs[M][:32].contiguous(), outs[32].contiguous()) == 0, M


def test_refusals_leave_the_output_untouched():
    from realtime_video_amd import _lib
    M, N, K = 32, 80, 640                                    # the plan cuts this K
    assert _lib.load().rtv_gemm_w8_segments(N, K) == 2 and _lib.load().rtv_gemm_w8_segments(N, 256) == 1
    a = torch.zeros(M + 1, K + 16, dtype=W.BF, device=DEV)
    wq = torch.zeros(N + 1, K + 32, dtype=torch.uint8, device=DEV)
    s = torch.ones(N + 8, dtype=torch.float32, device=DEV)
    out = torch.full((N + 1, N + 16), W.SENTINEL, dtype=W.BF, device=DEV)
    ws = torch.zeros(_lib.load().rtv_gemm_w8_workspace_bytes(M, N, K) + 64, dtype=torch.uint8, device=DEV)
    assert ws.numel() == 2 * M * N * 4 + 64
    good = dict(A=a.data_ptr(), lda=K + 16, Wq=wq.data_ptr(), ldw=K + 32, s=s.data_ptr(), C=out.data_ptr(), ldc=N + 16, t=0,
                M=M, N=N, K=K, ws=ws.data_ptr(), ws_bytes=ws.numel())

    def call(**kw):
        g = dict(good, **kw)
        _lib.call("rtv_gemm_w8", c_vp(g["A"]), g["lda"], c_vp(g["Wq"]), g["ldw"], c_vp(g["s"]), c_vp(g["C"]), g["ldc"], g["t"],
                  g["M"], g["N"], g["K"], c_vp(g["ws"]), ctypes.c_size_t(g["ws_bytes"]), c_vp(torch.cuda.current_stream().cuda_stream))

    bad = [("M", dict(M=0)), ("M", dict(M=48)), ("K", dict(K=192)), ("K", dict(K=0)), ("N", dict(N=24)), ("N", dict(N=0)),
           ("transpose_out", dict(t=2)), ("lda", dict(lda=K - 8)), ("lda", dict(lda=K + 4)), ("ldw", dict(ldw=K + 8)),
           ("ldw", dict(ldw=K - 16)), ("ldc", dict(ldc=N + 2)), ("ldc", dict(ldc=N - 4)), ("ldc", dict(t=1, ldc=M - 2)),
           ("aligned", dict(A=a.data_ptr() + 8)), ("aligned", dict(Wq=wq.data_ptr() + 8)), ("aligned", dict(C=out.data_ptr() + 4)),
           ("aligned", dict(t=1, C=out.data_ptr() + 1)), ("aligned", dict(s=s.data_ptr() + 4)),
           ("workspace", dict(ws_bytes=2 * M * N * 4 - 1)), ("workspace", dict(ws=0)), ("workspace", dict(ws=ws.data_ptr() + 4)),
           ("null", dict(A=0)), ("null", dict(Wq=0)), ("null", dict(s=0)), ("null", dict(C=0))]
    for word, kw in bad:
        with pytest.raises(RuntimeError, match=word):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == W.SENTINEL).all())
    call()                                                    # and the arguments they were derived from are accepted
    call(K=256, ws=0, ws_bytes=0)                             # a K the plan does not cut needs no workspace
    torch.cuda.synchronize()
    assert bool((out[:M, :N] == 0).all()) and bool((out[:M, N:] == W.SENTINEL).all()) and bool((out[M:] == W.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ the encoder
def _encoder(cfg, w, text_len, fp8):
    from realtime_video_amd.text_encoder import WanTextEncoder
    enc = WanTextEncoder(device=DEV, text_len=text_len, **cfg)
    enc.load_state_dict(w)
    return enc.enable_fp8_weights() if fp8 else enc


def test_enable_fp8_weights_stores_the_oracle_codes_and_halves_the_bytes():
    from oracle import t5_oracle as to
    cfg = dict(to.TINY_T5)
    w = tc.bf16_checkpoint(to.make_t5_weights(cfg, seed=0))
    enc = _encoder(cfg, w, 48, False)
    before = enc.weight_bytes()
    assert enc.enable_fp8_weights() is enc
    torch.cuda.synchronize()
    after = enc.weight_bytes()
    rows = cfg["num_layers"] * (3 * cfg["dim_attn"] + 2 * cfg["dim"] + 2 * cfg["dim_ffn"])      # one fp32 scale per output channel
    assert after["linears"] == before["linears"] // 2 + 4 * rows
    assert after["embedding"] == before["embedding"] and after["other"] == before["other"]
    assert after["total"] == before["total"] - before["linears"] // 2 + 4 * rows
    parts = {"qk": ("attn.q.weight", "attn.k.weight"), "v": ("attn.v.weight",), "o": ("attn.o.weight",),
             "gate_fc1": ("ffn.gate.0.weight", "ffn.fc1.weight"), "fc2": ("ffn.fc2.weight",)}
    for i in range(cfg["num_layers"]):
        for name, keys in parts.items():
            q, s = zip(*(W.quantised(w, f"blocks.{i}.{k}") for k in keys))
            codes, scales = enc._t[f"blocks.{i}.{name}.codes"].cpu(), enc._t[f"blocks.{i}.{name}.scales"].cpu()
            assert f"blocks.{i}.{name}" not in enc._t                                           # the bf16 copy is gone
            assert W.mismatches(codes, torch.cat(q).view(torch.uint8)) == 0, (i, name)
            assert W.mismatches(scales, torch.cat(s).reshape(-1)) == 0, (i, name)
    ptrs = [enc._layers[0].qk_q, enc._layers[0].fc2_s]
    enc.enable_fp8_weights()                                                                    # twice: nothing happens
    assert [enc._layers[0].qk_q, enc._layers[0].fc2_s] == ptrs and enc.weight_bytes() == after
    ids, mask = to.t5_inputs(cfg)
    out8 = enc.encode_ids(ids, mask)["prompt_embeds"]
    enc.load_state_dict(w)                                                                      # back to bf16
    assert enc.weight_bytes() == before
    out16 = enc.encode_ids(ids, mask)["prompt_embeds"]
    ref = _encoder(cfg, w, 48, False).encode_ids(ids, mask)["prompt_embeds"]
    assert not enc._fp8 and isinstance(enc._w, type(_encoder(cfg, w, 48, False)._w))
    assert tc.rel_l2(out16, ref) < 1e-3 < tc.rel_l2(out8, ref)       # e4m3 rounds every weight by up to 2^-4: far above 1e-3


@pytest.fixture(scope="module")
def deep():
    """The 24-layer problem of tests/test_text_encoder_gpu.py, its weights dequantised, and the two CPU chains per prompt."""
    from oracle import t5_oracle as to
    cfg = dict(to.TINY_T5, **tc.DEEP_T5)
    w = tc.bf16_checkpoint(to.make_t5_weights(cfg, seed=5))
    ids, mask = to.t5_inputs(cfg, seed=13, L=tc.DEEP_TEXT_LEN, lens=tc.DEEP_LENS)
    dq = W.dequantised(w)
    gold = [tc.encoder_chain(dq, ids[b, :n], cfg) for b, n in enumerate(tc.DEEP_LENS)]
    emulated = [tc.rel_l2(tc.encoder_chain(dq, ids[b, :n], cfg, torch.float32, native=True), gold[b]) for b, n in enumerate(tc.DEEP_LENS)]
    return cfg, w, ids, mask, gold, emulated


def test_24_layers_on_e4m3_weights_within_twice_the_rounding_emulation(deep):
    """The bar form of the bf16 path's 24-layer test, against a reference that is not the code under test: `gold` is the fp64 chain
    on the DEQUANTISED weights (value(c) * s_w: what the mode computes with), `emulated` the distance of the fp32 chain with the
    native path's bf16 rounding points on the same weights; the e4m3 encoder must lie within twice that.  Padding rows are zero, a
    prompt encoded alone equals its rows in the two-prompt batch bit for bit.  The distance to the bf16 encoder on the same
    checkpoint is printed and recorded: it is the price of the mode (no bar; synthetic weights say nothing about the checkpoint)."""
    cfg, w, ids, mask, gold, emulated = deep
    enc = _encoder(cfg, w, tc.DEEP_TEXT_LEN, True)
    out = enc.encode_ids(ids, mask)["prompt_embeds"]
    bf16_out = _encoder(cfg, w, tc.DEEP_TEXT_LEN, False).encode_ids(ids, mask)["prompt_embeds"].cpu()
    lines = []
    for b, n in enumerate(tc.DEEP_LENS):
        native = tc.rel_l2(out[b, :n].cpu(), gold[b])
        price = tc.rel_l2(out[b, :n].cpu(), bf16_out[b, :n])
        lines.append(f"T5_W8_DEEP tokens={n} layers=24 width={cfg['dim']} rel_l2_w8_vs_fp64_dequantised={native:.4e} "
                     f"rel_l2_emulated={emulated[b]:.4e} ratio={native / emulated[b]:.3f} rel_l2_w8_vs_bf16_encoder={price:.4e}")
        print(lines[-1])
        assert native <= 2.0 * emulated[b], (n, native, emulated[b])
        assert float(out[b, n:].abs().max() if n < tc.DEEP_TEXT_LEN else 0.0) == 0.0
        alone = enc.encode_ids(ids[b:b + 1], mask[b:b + 1])["prompt_embeds"]
        assert torch.equal(alone[0], out[b]), n
    path = os.environ.get("RTV_T5_W8_PARITY_RECORD")
    if path:
        with open(path, "w") as f:
            f.write("# TINY_T5 width, 24 layers, synthetic weights (oracle.t5_oracle.make_t5_weights seed 5): no claim for the checkpoint\n")
            f.write("".join(line + "\n" for line in lines))
