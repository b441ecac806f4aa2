"""profiles/attn_peaked_bound_ratios.txt from the printed output of the peaked attention tests.

    pytest -m gpu tests/test_attention_peaked_gpu.py -s > run.log
    python scripts/attn_peaked_ratios.py run.log > profiles/attn_peaked_bound_ratios.txt

Every case prints `ATTN_RATIO family=.. kernel=.. dtype=.. splits=.. case=.. ratio=..`: ratio = the largest
|out - ref| / (u * ref_abs + 2.5e-7) of the case, u = 2^-8 (bf16) / 2^-11 (f16), ref_abs = P @ |V| in fp64.  The bar of
tests/attn_cases.within_bound is 4; the worst case of the kernels' arithmetic is 2.
"""
import collections
import re
import sys

FAMILIES = {"a": "every key position", "b": "block-causal boundary", "c": "nothing outside the window", "d": "two-range windows",
            "e": "counted key", "f": "split and combine", "g": "rescale path (staircase)", "h": "output rows", "i": "Gaussian data"}
LINE = re.compile(r"ATTN_RATIO family=(\w) kernel=(.*?) dtype=(\w+) splits=(\d+) case=(\S+) ratio=(\S+)")


def main(path):
    worst = collections.defaultdict(lambda: (0.0, ""))
    count = collections.Counter()
    for line in open(path, errors="replace"):
        for m in LINE.finditer(line):
            key = (m[1], m[2], m[3])
            count[key] += 1
            if float(m[6]) >= worst[key][0]:
                worst[key] = (float(m[6]), m[5] + (f" S={m[4]}" if m[4] != "1" else ""))
    print("Largest |out - ref| / (u * ref_abs) per family, kernel and dtype over one run of tests/test_attention_peaked_gpu.py on an MI355X")
    print("(u = 2^-8 bf16, 2^-11 f16; ref = the fp64 definition, ref_abs = P @ |V|).  Bar: 4.  Worst case of the arithmetic: 2.")
    print(f"{sum(count.values())} launches.\n")
    print(f"{'family':<32} {'kernel':<76} {'dtype':<5} {'cases':>5} {'ratio':>7}  worst case")
    for key in sorted(worst):
        fam, kernel, dt = key
        print(f"{fam + '. ' + FAMILIES.get(fam, ''):<32} {kernel:<76} {dt:<5} {count[key]:>5} {worst[key][0]:>7.3f}  {worst[key][1]}")


if __name__ == "__main__":
    main(sys.argv[1])
