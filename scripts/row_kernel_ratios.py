"""profiles/row_kernel_bound_ratios.txt from the printed output of the row-kernel tests.

    pytest -m gpu tests/test_row_kernels_gpu.py -s > run.log
    python scripts/row_kernel_ratios.py run.log > profiles/row_kernel_bound_ratios.txt

Every launch that is held to a bar prints `ROW_RATIO kernel=.. form=.. family=.. d=.. ratio=..`: ratio = the largest
|out - ref| / worst case of the launch, ref = the fp64 definition on the bf16 rows, worst case = the per-element sum of the
kernel's rounding errors (tests/row_cases.py: ln64, rms64, rope64).  The bar is 2.
"""
import collections
import re
import sys

LINE = re.compile(r"ROW_RATIO kernel=(\S+) form=(\S+) family=(\S+) d=(\d+) ratio=(\S+)")
WALL = re.compile(r"(\d+) passed.* in ([0-9.]+)s")


def main(path):
    worst = collections.defaultdict(lambda: (-1.0, ""))
    count = collections.Counter()
    wall = None
    for line in open(path, errors="replace"):
        wall = WALL.search(line) or wall
        for m in LINE.finditer(line):
            key = (m[1], m[2], m[3])
            count[key] += 1
            if float(m[5]) > worst[key][0]:
                worst[key] = (float(m[5]), m[4])
    print("Largest |out - ref| / worst case per kernel, form and family over one run of tests/test_row_kernels_gpu.py on an MI355X")
    print("(ref = the fp64 definition on the bf16 rows the kernel receives; worst case = the per-element sum of the kernel's rounding")
    print("errors, tests/row_cases.py).  Bar: 2.  Worst case of the arithmetic: 1.")
    print(f"{sum(count.values())} launches under a bar" + (f"; {wall[1]} tests, wall time of the file {wall[2]} s." if wall else "."))
    print(f"\n{'kernel':<10} {'form':<18} {'family':<16} {'launches':>8} {'ratio':>7}  at d")
    for key in sorted(worst):
        print(f"{key[0]:<10} {key[1]:<18} {key[2]:<16} {count[key]:>8} {worst[key][0]:>7.3f}  {worst[key][1]}")


if __name__ == "__main__":
    main(sys.argv[1])
