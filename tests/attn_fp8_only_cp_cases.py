"""Restatements for the tests of the code exchange on the e4m3-only KV cache (include/rtv_hip_attn_fp8_only_cp.h), in numpy: the
staging layout kv8 [world][2][M / world][H * 128], the commit of a gathered kv8 into k8 / v8t - the ring mapping of rtv_dit_step
plus RTV_ATTN_FP8_SLOT - and the case list of tests/test_attn_fp8_only_cp_gpu.py.  Nothing here computes a code: the feature moves
codes that existing kernels define, so every comparison that uses these functions is bit for bit."""
import numpy as np

D, KT = 128, 64            # head dimension; rows per storage tile of v8t
SENTINEL = 0x5A            # what every array holds before a kernel writes: bytes that must stay untouched are compared as well


def slot(key):
    """RTV_ATTN_FP8_SLOT (include/rtv_hip_attn_fp8.h), restated from its text: key 32 kb + 8 i + 4 g + j -> slot 32 g + 16 kb + 4 i + j."""
    return ((key >> 2) & 1) * 32 + (key >> 5) * 16 + ((key >> 3) & 3) * 4 + (key & 3)


SLOT = np.array([slot(k) for k in range(KT)])


# ------------------------------------------------------------------------------------------------ staging
def empty_staging(M, H, world, fill=SENTINEL):
    assert M % world == 0
    return np.full((world, 2, M // world, H * D), fill, dtype=np.uint8)


def stage(kv8, k_codes, v_codes, row_begin):
    """The codes [rows, H * 128] of the logical rows [row_begin, row_begin + rows) into the segment of the rank that owns them."""
    S = kv8.shape[2]
    for i in range(k_codes.shape[0]):
        r, m = divmod(row_begin + i, S)
        kv8[r, 0, m], kv8[r, 1, m] = k_codes[i], v_codes[i]
    return kv8


def staged_rows(kv8):
    """A gathered kv8 -> (K codes [M, H * 128], V codes [M, H * 128]) in the order of the block's rows."""
    world, _, S, d = kv8.shape
    return kv8[:, 0].reshape(world * S, d), kv8[:, 1].reshape(world * S, d)


# ------------------------------------------------------------------------------------------------ commit
def physical_rows(cache_row0, M, ring=(0, 0, 0)):
    """Physical cache row of each logical row cache_row0 + m (rtv_dit_step): sink rows in place, ring rows rotated by ring_shift."""
    lo, size, shift = ring
    rows = cache_row0 + np.arange(M)
    if size > 0:
        in_ring = rows >= lo
        rows = np.where(in_ring, lo + (rows - lo + shift) % size, rows)
    return rows


def segments(cache_row0, M, ring=(0, 0, 0)):
    """Runs of consecutive physical rows, in logical order: [(first physical row, rows)]."""
    p = physical_rows(cache_row0, M, ring)
    cuts = [0] + [i for i in range(1, M) if p[i] != p[i - 1] + 1] + [M]
    return [(int(p[a]), b - a) for a, b in zip(cuts[:-1], cuts[1:])]


def commit(kv8, k8, v8t, cache_row0, ring=(0, 0, 0)):
    """A gathered kv8 into k8 [cache_rows, H, 128] / v8t [tiles, H, 128, 64], in place: K rows byte for byte, V rows transposed per
    storage tile into the slots of their physical rows; no other byte is written."""
    k, v = staged_rows(kv8)
    H = k8.shape[1]
    p = physical_rows(cache_row0, k.shape[0], ring)
    k8[p] = k.reshape(-1, H, D)
    v8t[p >> 6, :, :, SLOT[p & 63]] = v.reshape(-1, H, D)
    return k8, v8t


def empty_cache(cache_rows, H, fill=SENTINEL):
    return (np.full((cache_rows, H, D), fill, dtype=np.uint8), np.full(((cache_rows + KT - 1) // KT, H, D, KT), fill, dtype=np.uint8))


def ungather_v(v8t, rows):
    """Codes of the physical V rows `rows` out of v8t -> [len(rows), H, 128]."""
    rows = np.asarray(rows)
    return v8t[rows >> 6, :, :, SLOT[rows & 63]]


# ------------------------------------------------------------------------------------------------ cases
# Stage: M = 150 rows as F x gh x gw = 3 x 5 x 10, three ranks of 50 rows - both shard boundaries (50, 100) inside a 64-row storage
# tile -, RoPE from frame 2.
STAGE_GRID, STAGE_START, STAGE_WORLD = (3, 5, 10), 2, 3
STAGE_M = STAGE_GRID[0] * STAGE_GRID[1] * STAGE_GRID[2]
WIDTHS = [(256, 2), (640, 5)]      # (d, H): the smallest width, and one whose head count is odd

# Commit: name -> (M, world, cache_rows, cache_row0, (ring_lo, ring_size, ring_shift))
COMMIT_CASES = {
    "no_ring_partial_tiles": (150, 3, 256, 37, (0, 0, 0)),          # physical 37 .. 186: first and last tile partly covered
    "sink_ring_no_wrap": (150, 3, 320, 30, (64, 256, 100)),         # sink rows 30 .. 63, ring rows 164 .. 279
    "sink_ring_one_wrap": (150, 3, 320, 30, (64, 256, 200)),        # sink rows 30 .. 63, ring rows 264 .. 319, then 64 .. 123
    "whole_tiles": (128, 2, 256, 64, (0, 0, 0)),                    # physical 64 .. 191: two whole tiles, nothing partial
}
COMMIT_SEGMENTS = {
    "no_ring_partial_tiles": [(37, 150)],
    "sink_ring_no_wrap": [(30, 34), (164, 116)],
    "sink_ring_one_wrap": [(30, 34), (264, 56), (64, 60)],
    "whole_tiles": [(64, 128)],
}
