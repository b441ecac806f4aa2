"""profiles/t5_kernel_bound_ratios.txt from the printed output of the text-encoder kernel tests.

    pytest -m gpu tests/test_t5_kernels_gpu.py tests/test_text_encoder_gpu.py -s > run.log
    python scripts/t5_kernel_ratios.py run.log > profiles/t5_kernel_bound_ratios.txt

Every launch that is held to a bar prints `T5_RATIO kernel=.. family=.. shape=.. ratio=..` (tests/t5_cases.py has the bars): for
attention ratio = the largest |out - ref| / (u P|V| + 2.5e-7) of the launch, bar 4; for rmsnorm, geglu and the zero-layer encoder
the largest |out - ref| / worst case, bar 2; embed and add are bit-exact (ratio 0).  The 24-layer run prints `T5_DEEP ...`: the
native path's and the CPU rounding emulation's rel-L2 against the fp64 chain, bar native <= 2 x emulated.
"""
import collections
import re
import sys

LINE = re.compile(r"T5_RATIO kernel=(\S+) family=(\S+) shape=(\S+) ratio=(\S+)")
DEEP = re.compile(r"T5_DEEP tokens=(\d+) layers=(\d+) rel_l2_native=(\S+) rel_l2_emulated=(\S+) ratio=(\S+)")
BAR = collections.defaultdict(lambda: 2.0, attention=4.0, embed=0.0, add=0.0)


def main(path):
    worst = collections.defaultdict(lambda: (-1.0, ""))
    count = collections.Counter()
    deep = []
    for line in open(path, errors="replace"):
        for m in LINE.finditer(line):
            key = (m[1], m[2])
            count[key] += 1
            if float(m[4]) > worst[key][0]:
                worst[key] = (float(m[4]), m[3])
        deep += DEEP.findall(line)
    print("Largest ratio per kernel and family over one run of tests/test_t5_kernels_gpu.py and tests/test_text_encoder_gpu.py on an")
    print("MI355X (ref = the fp64 definition on the tensors the kernel receives; tests/t5_cases.py has the bars).  attention: |out - ref|")
    print("over u P|V| + 2.5e-7, bar 4.  rmsnorm, geglu, encode_0_layers: |out - ref| over the worst case of the arithmetic, bar 2.")
    print("embed, add: bit-exact.  shape: valid/rows,heads,max_len for attention, rows x width otherwise.")
    print(f"{sum(count.values())} launches, each run twice with equal bits.")
    print(f"\n{'kernel':<16} {'family':<16} {'launches':>8} {'ratio':>7} {'bar':>4}  at shape")
    for key in sorted(worst):
        print(f"{key[0]:<16} {key[1]:<16} {count[key]:>8} {worst[key][0]:>7.3f} {BAR[key[0]]:>4.0f}  {worst[key][1]}")
    if deep:
        print("\n24 layers of TINY_T5 (dim 256), rel-L2 against the fp64 chain; bar: native <= 2 x emulated")
        print(f"{'tokens':>6} {'native':>11} {'emulated':>11} {'ratio':>6}")
        for tokens, _, native, emulated, ratio in deep:
            print(f"{tokens:>6} {native:>11} {emulated:>11} {ratio:>6}")


if __name__ == "__main__":
    main(sys.argv[1])
