"""Where the folded cross-attention stops paying: the 14B cross-attention + output projection at M = 4680 rows, H = 40,
  unfolded  rtv_attn_fwd_dup over text_rows + 1 keys  +  rtv_gemm [4680, 5120] x [5120, 5120]^T (+ bias + residual)
  folded    rtv_attn_probs_dup -> P [4680, k_fold]    +  rtv_gemm [4680, k_fold] x [5120, k_fold]^T (+ bias + residual)
for kh = 40, 72, 88, 104, 120 (text_rows = kh - 8, the longest prompt of that width), interleaved launch by launch, weights
rotated over four layers' worth so that no call finds its weight in the caches, three repeats per width; and what the folded
weight costs per layer and prompt (rtv_cross_fold_weight).  -> the table behind RTV_CROSS_FOLD_KH_MAX (include/rtv_hip_cross_fold.h).
usage: python scripts/cross_fold_kh_sweep.py > profiles/cross_fold_kh_sweep.txt"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from realtime_video_amd import ops  # noqa: E402

DEV, M, H, D, NW, ITERS, REPEATS = "cuda", 4680, 40, 5120, 4, 40, 3
g = torch.Generator(device=DEV).manual_seed(0)
rnd = lambda *s, std=1.0: (torch.randn(*s, generator=g, device=DEV) * std).to(torch.bfloat16)
q, x, bias = rnd(1, M, H, 128), rnd(M, D), rnd(D)
k, v = rnd(1, 512, H, 128), rnd(1, 512, H, 128)
co_w = [rnd(D, D, std=0.02) for _ in range(NW)]
ao, out = torch.empty(1, M, H, 128, dtype=torch.bfloat16, device=DEV), torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
ops.ensure_gemm_workspace(torch.device(DEV))


def timed(fns):
    """us per call of each fn, the fns interleaved call by call."""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)] for _ in fns]
    for i in range(-3, ITERS):
        for j, f in enumerate(fns):
            if i >= 0:
                ev[j][i][0].record()
            f(i)
            if i >= 0:
                ev[j][i][1].record()
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(b) * 1e3 for a, b in e)[ITERS // 2] for e in ev]


print("# us per launch (median of %d, events around each launch), three repeats each; M = %d, H = %d, d = %d" % (ITERS, M, H, D))
print("#  kh  k_fold  text_rows | attn_fwd_dup   gemm K=5120 | attn_probs_dup  gemm K=k_fold | unfolded  folded  saved   | fold weight us/layer")
for kh in (40, 72, 88, 104, 120):
    rows = kh - 8
    kf = (H * kh + 63) // 64 * 64
    vo = [ops.cross_fold_weight(w, v[0].view(512, D), rows + 1, kh, kf) for w in co_w]
    p = torch.empty(M, kf, dtype=torch.bfloat16, device=DEV)
    kk, vv = k[:, :rows + 1], v[:, :rows + 1]
    fns = [lambda i: ops.attn_fwd_dup(q, kk, vv, rows, 512 - rows, out=ao),
           lambda i: ops.gemm(ao.view(M, D), co_w[i % NW], bias=bias, residual=x, out=out),
           lambda i: ops.attn_probs_dup(q[0], kk[0], rows, 512 - rows, kh, kf, out=p),
           lambda i: ops.gemm(p, vo[i % NW], bias=bias, residual=x, out=out),
           lambda i: ops.cross_fold_weight(co_w[i % NW], v[0].view(512, D), rows + 1, kh, kf, out=vo[i % NW])]
    for _ in range(REPEATS):
        a, b, c, d, e = timed(fns)
        print(f"  {kh:4d} {kf:6d} {rows:9d} | {a:10.1f}   {b:10.1f}   | {c:10.1f}     {d:10.1f}    | {a + b:7.1f}  {c + d:7.1f} {a + b - c - d:7.1f} | {e:8.1f}")
