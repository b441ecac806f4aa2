"""What tests/test_mxfp4_gpu.py and tests/test_mxfp6_gpu.py share: the tiny model both block-scaled modes run (every Linear input
width a multiple of 256, so that both modes accept it), its inputs, and the three-forward sequence through the model and through
the oracle graph.  The tests and their assertions stay in the two files."""
import torch

DEV = "cuda"
BF = torch.bfloat16


def dev_operands(mx, c):
    """An exact_case of the oracle module `mx` in that format's storage, on the device: (a codes, a scales, w codes, w scales)."""
    return (mx.pack_codes(c["a"]).to(DEV), mx.pack_scales(c["ea"]).to(DEV), mx.pack_codes(c["w"]).to(DEV),
            mx.pack_scales(c["ew"]).to(DEV))


CFG = dict(dim=256, ffn_dim=512, num_heads=2, num_layers=2, freq_dim=256, text_len=512, eps=1e-6, num_frame_per_block=3)
TEXT_DIM = 256


def inputs():
    from oracle.make_golden import tiny_inputs
    lat, _ = tiny_inputs()
    ctx = torch.randn(64, TEXT_DIM, generator=torch.Generator().manual_seed(43)).to(BF)
    return lat, ctx


def build(weights):
    from realtime_video_amd.causal_model import CausalWanModel
    from realtime_video_amd.wan_wrapper import WanDiffusionWrapper
    m = CausalWanModel(dim=CFG["dim"], ffn_dim=CFG["ffn_dim"], num_heads=CFG["num_heads"], num_layers=CFG["num_layers"],
                       text_dim=TEXT_DIM, freq_dim=CFG["freq_dim"])
    m.load_state_dict(weights)
    return m, WanDiffusionWrapper(m, timestep_shift=5.0)


def caches(kv_size=9360):
    hd, L, H = CFG["dim"] // CFG["num_heads"], CFG["num_layers"], CFG["num_heads"]
    kv = [{"k": torch.zeros(1, kv_size, H, hd, dtype=BF, device=DEV), "v": torch.zeros(1, kv_size, H, hd, dtype=BF, device=DEV),
           "global_end_index": 0, "local_end_index": 0} for _ in range(L)]
    ca = [{"k": torch.zeros(1, 512, H, hd, dtype=BF, device=DEV), "v": torch.zeros(1, 512, H, hd, dtype=BF, device=DEV),
           "is_init": False} for _ in range(L)]
    return kv, ca


def three_forwards(model, wr, lat, ctx, t, t0):
    """Denoise at cache offset 0, block-causal recompute, second-block denoise (tests/test_fp8_rows_gpu.py's sequence)."""
    kv, ca = caches()
    cond = {"prompt_embeds": [ctx.to(DEV)]}
    a, _ = wr(lat[0].to(DEV), cond, t.to(DEV), kv, ca, current_start=0)
    for c in kv:
        c["global_end_index"] = 0
        c["local_end_index"] = 0
    model.block_mask = model._prepare_blockwise_causal_attn_mask(device=DEV, num_frames=3, frame_seqlen=1560, num_frame_per_block=3)
    rc, _ = wr(lat[2].to(DEV), cond, t0.to(DEV), kv, ca, current_start=4680)
    model.block_mask = None
    b, _ = wr(lat[3].to(DEV), cond, t.to(DEV), kv, ca, current_start=4680)
    return [x.cpu() for x in (a, rc, b)]


def oracle_forwards(wo, w, lat, ctx, t, t0, dtype):
    """The same three forwards through the oracle graph (evaluated by torch on the device, like tests/test_dit_gpu.py), in bf16 or in
    the oracle's fp32 gold arithmetic."""
    gold = dtype == torch.float32
    wd = {k: (v.to(DEV).to(dtype) if torch.is_tensor(v) else v) for k, v in w.items()}
    kvc = wo.initialize_kv_cache(CFG["num_layers"], 1, 9360, CFG["num_heads"], 128, dtype, DEV)
    cac = wo.initialize_crossattn_cache(CFG["num_layers"], 1, CFG["num_heads"], 128, dtype, device=DEV)
    kw = dict(attn_fn=lambda q, k, v: wo.attention_sdpa(q, k, v, dtype=None)) if gold else {}
    sched, c = wo.FlowMatchScheduler(), [ctx.to(DEV).to(dtype)]
    x = [v.to(DEV).to(dtype) for v in lat]
    a, _ = wo.wrapper_forward(wd, CFG, sched, x[0], c, t.to(DEV), kvc, cac, 0, **kw)
    wo.reset_kv_cache(kvc)
    rc, _ = wo.wrapper_forward(wd, CFG, sched, x[2], c, t0.to(DEV), kvc, cac, 4680, recompute=True, **kw)
    b, _ = wo.wrapper_forward(wd, CFG, sched, x[3], c, t.to(DEV), kvc, cac, 4680, **kw)
    return [v.float().cpu() for v in (a, rc, b)]
