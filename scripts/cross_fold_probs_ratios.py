"""Error of softmax PROBABILITIES against the fp64 definition on the inputs of tests/test_cross_fold_gpu.py, as the ratio
|P - P_ref| / (u P_ref + tiny), u = 2^-8 (tests/cross_fold_cases.py):
  today  rtv_attn_fwd_dup with V = identity columns (V[t, h, :] = e_t), whose output row IS its normalised P - the number the
         test's bound factor is taken from (twice its largest ratio, at most 4);
  new    rtv_attn_probs_dup.
usage: python scripts/cross_fold_probs_ratios.py > profiles/cross_fold_probs_ratios.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cross_fold_cases as cf  # noqa: E402
from realtime_video_amd import ops  # noqa: E402

DEV = "cuda"
print("# family   H  keys  count   today (fwd_dup, V = I)   new (probs_dup)     [largest ratio over Lq in %s]" % (cf.LQ,))
worst = [0.0, 0.0]
for family in cf.FAMILIES:
    for H in cf.HEADS:
        for keys in cf.KEYS:
            for count in cf.COUNTS:
                r = [0.0, 0.0]
                for Lq in cf.LQ:
                    q, k, dup = cf.probs_inputs(family, Lq, H, keys, count)
                    q, k = q.to(DEV), k.to(DEV)
                    ref = cf.probs_ref64(q, k, dup, count)
                    v = torch.zeros(keys, H, 128, dtype=torch.bfloat16, device=DEV)
                    v[torch.arange(keys), :, torch.arange(keys)] = 1.0
                    today = ops.attn_fwd_dup(q[None], k[None], v[None], dup, count)[0][..., :keys]
                    kh = cf.round_up(keys, 8)
                    cols = cf.round_up(H * kh, 64)
                    new = ops.attn_probs_dup(q, k, dup, count, kh, cols)[:, :H * kh].view(Lq, H, kh)[..., :keys]
                    r = [max(r[0], cf.probs_ratio(today, ref)), max(r[1], cf.probs_ratio(new, ref))]
                worst = [max(worst[0], r[0]), max(worst[1], r[1])]
                print(f"{family:9s} {H:2d} {keys:5d} {count:6d}   {r[0]:10.3f}               {r[1]:10.3f}")
print(f"# largest: today {worst[0]:.3f}, new {worst[1]:.3f}  ->  bound factor min(2 x today, 4) = {min(2 * worst[0], 4.0):.2f}")
