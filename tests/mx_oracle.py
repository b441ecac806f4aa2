"""Restatement of the OCP Microscaling Formats (MX) v1.0 conversion with the floor rule, for any element format given by its
table of magnitudes - the part tests/mxfp4_oracle.py and tests/mxfp6_oracle.py share - in plain torch, evaluated in float64 by
search over the value table (no bit tricks):

    per block of 32 consecutive elements of the last dim
    amax = max |x|                e = clamp(floor(log2 amax) - 2, -127, 127)      (an all-zero block: e = -127, codes 0)
    code = nearest magnitude of the table to x * 2^-e; ties to the even code; saturating at the largest
    y[m,n] = bf16(sum_k dq(x)[m, k] dq(w)[n, k] + bias[n])      dq = code value * 2^e

Both tables end below 8 = 2^(2 + 1), which is what "- 2" in e is for.  The format modules bind a Format and keep what is their
own: the table, the packers of the header's storage, the structured inputs."""
import torch
import torch.nn.functional as F

BLOCK = 32


def _blocks(t):
    if t.shape[-1] % BLOCK:
        raise ValueError("the last dim must be a multiple of 32")
    return t.detach().double().reshape(*t.shape[:-1], t.shape[-1] // BLOCK, BLOCK)


def mx_dequantize(values, e):
    return torch.ldexp(_blocks(values), e.unsqueeze(-1)).reshape(values.shape)


def product_fp64(a, ea, w, ew):
    """-> (sum_k dq(a) dq(w) in float64 [M, N], sum_k |terms| [M, N])"""
    da, dw = mx_dequantize(a, ea), mx_dequantize(w, ew)
    return da @ dw.t(), da.abs() @ dw.abs().t()


def pack_scales(e, scale_pos, scale_bytes):
    """block exponents int64 [M, K / 32] -> uint8 [M, scale_bytes(K)] in the header's order (unowned bytes 0)."""
    M, nb = e.shape
    out = torch.zeros(M, scale_bytes(nb * BLOCK), dtype=torch.uint8, device=e.device)
    pos = torch.tensor([scale_pos(b) for b in range(nb)], device=e.device)
    out[:, pos] = (e + 127).to(torch.uint8)
    return out


class Format:
    """`values`: magnitude of code c, increasing.  `wrap_from`: where a format without saturation would round to the next binade,
    8, whose magnitude code wraps to 0 (the midpoint of the largest magnitude and 8) - the `saturate=False` mutant."""

    def __init__(self, values, wrap_from):
        self.values, self.wrap_from = values, wrap_from
        n = len(values)
        self.even_first = tuple(range(0, n, 2)) + tuple(range(1, n, 2))   # torch.argmin returns the first of equal minima: the even code wins a tie
        self.large_first = tuple(range(n - 1, -1, -1))                    # mutant: the larger magnitude wins a tie (round half away from zero)

    def _nearest(self, a, order):
        grid = torch.tensor([self.values[c] for c in order], dtype=torch.float64, device=a.device)
        k = (a.unsqueeze(-1) - grid).abs().argmin(dim=-1)                 # exact: a has at most 24 significant bits
        return torch.tensor(order, device=a.device)[k]

    def mx_quantize(self, t, tie_order=None, ceil_scale=False, saturate=True):
        """-> (code values, +- the table's, as float64, shape of t; block exponents e as int64 [..., K / 32]).
        The keyword arguments build the mutants of the CPU tests; the defaults are the format."""
        x = _blocks(t)
        amax = x.abs().amax(dim=-1)
        mant, ex = torch.frexp(amax)                                      # amax = mant * 2^ex, mant in [0.5, 1): floor(log2) = ex - 1
        lg = ex.long() - 1
        if ceil_scale:
            lg = lg + (mant != 0.5).long()
        e = torch.where(amax > 0, (lg - 2).clamp(-127, 127), torch.full_like(lg, -127))
        y = torch.ldexp(x, -e.unsqueeze(-1))                              # exact in float64
        a = y.abs()
        c = self._nearest(a, self.even_first if tie_order is None else tie_order)
        if not saturate:
            c = torch.where(a >= self.wrap_from, torch.zeros_like(c), c)
        val = torch.tensor(self.values, dtype=torch.float64, device=t.device)[c]
        val = torch.where(torch.signbit(y), -val, val)
        return val.reshape(t.shape), e

    def mx_linear(self, x, weight, bias, shards=1):
        """nn.Linear on operands of this format.  `shards` is accepted and ignored: a block needs nothing but itself."""
        xq = mx_dequantize(*self.mx_quantize(x)).float()
        wq = mx_dequantize(*self.mx_quantize(weight)).float()
        y = F.linear(xq, wq)
        if bias is not None:
            y = y + bias.float()
        return y.to(x.dtype)

    def exact_case(self, M, N, K, seed=0):
        """Operands of the exact GEMM case: codes uniform over all magnitudes with random signs, block exponents in {-1, 0, 1},
        distinct per row and per block, no symmetry between the operands.  -> dict of code values [M, K] / [N, K] (float64),
        exponents [M, K / 32] / [N, K / 32] (int64)."""
        g = torch.Generator().manual_seed(seed)
        val = torch.tensor(self.values, dtype=torch.float64)

        def operand(rows):
            c = val[torch.randint(0, len(self.values), (rows, K), generator=g)]
            c = torch.where(torch.rand(rows, K, generator=g) < 0.5, -c, c)
            e = torch.randint(-1, 2, (rows, K // BLOCK), generator=g)
            return c, e

        a, ea = operand(M)
        w, ew = operand(N)
        return dict(a=a, ea=ea, w=w, ew=ew)
