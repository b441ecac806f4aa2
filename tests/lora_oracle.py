"""float64 oracle of the LoRA merge (include/rtv_hip_lora.h) and the per-element criterion the kernel is held to.

    ref = base + sum_a scale_a * B_a @ A_a                 (float64 throughout)
    mag = |base| + sum_a |scale_a| * (|B_a| @ |A_a|)       (what fp32 accumulation error scales with)

Criterion: |W - ref| <= 2^(floor(log2 |ref|) - 8) + 2^-16 * mag  - half a bf16 ulp of the reference (8 significand bits) plus
fp32 accumulation slack - and at least 99.9 % of the elements equal bf16(ref) exactly (a cap against a systematic bias: an
element may only differ where the fp32 sum falls on the other side of a rounding boundary than the exact one)."""
import torch

BASE_STD, AB_STD = 0.02, 0.05


def make_inputs(N, K, ranks, seed):
    """base ~ 0.02 N(0,1) [N, K], per rank A ~ 0.05 N(0,1) [r, K] and B ~ 0.05 N(0,1) [N, r]; all bf16, seeded."""
    g = torch.Generator().manual_seed(seed)
    base = (BASE_STD * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    ab = [((AB_STD * torch.randn(r, K, generator=g)).to(torch.bfloat16), (AB_STD * torch.randn(N, r, generator=g)).to(torch.bfloat16))
          for r in ranks]
    return base, ab


def merge_oracle(base, adapters):
    """base bf16 [N, K], adapters [(A [r, K], B [N, r], scale)] -> (ref, mag), float64 on the CPU."""
    ref = base.detach().cpu().double()
    mag = ref.abs()
    for A, B, scale in adapters:
        A, B = A.detach().cpu().double(), B.detach().cpu().double()
        ref = ref + float(scale) * (B @ A)
        mag = mag + abs(float(scale)) * (B.abs() @ A.abs())
    return ref, mag


def fp32_emulation(base, adapters):
    """The kernel's arithmetic in torch on the CPU: fp32 products of the bf16 operands, one accumulation per adapter, the scale
    applied in fp32, one rounding to bf16."""
    tot = torch.zeros(base.shape, dtype=torch.float32)
    for A, B, scale in adapters:
        tot = tot + torch.tensor(float(scale), dtype=torch.float32) * (B.float() @ A.float())
    return (base.float() + tot).to(torch.bfloat16)


def criterion(W, ref, mag):
    """-> (fraction of elements within the bound, fraction equal to bf16(ref), worst |W - ref| / bound)."""
    W = W.detach().cpu().double()
    a = ref.abs()
    half_ulp = torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp(min=1e-300))) - 8), torch.zeros_like(a))
    bound = half_ulp + 2.0 ** -16 * mag
    err = (W - ref).abs()
    within = float((err <= bound).double().mean())
    exact = float((W == ref.to(torch.bfloat16).double()).double().mean())
    worst = float((err / bound.clamp(min=1e-300)).max())
    return within, exact, worst


def assert_meets(W, ref, mag, what=""):
    within, exact, worst = criterion(W, ref, mag)
    print(f"lora criterion {what}: within bound {within:.6%}, exact {exact:.6%}, worst err / bound {worst:.3f}")
    assert within == 1.0, f"{what}: {1 - within:.3%} of the elements outside the bound (worst err / bound {worst:.3f})"
    assert exact >= 0.999, f"{what}: only {exact:.4%} of the elements equal bf16(ref)"
