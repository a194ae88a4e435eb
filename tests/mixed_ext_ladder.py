"""The cases at which the 2D and real plans are checked with their 7-smooth lengths on the mixed-radix engine (csrc/fft_plans_ext.h:
AnyPlan / Plan2D / RealPlan with smooth set), on the GPU
(tests/test_gpu_mixed_ext.py) and in the CPU emulation (tests/test_emulated_mixed_ext.py).  Inputs and float64 references are
those of tests/ext_ladder.py.  Test infrastructure only.

Every case names the property it is there for and the path it must take; the tests assert the path.

Engines: MIXED the mixed-radix plan, POW2 the power-of-two engine, CHIRPZ Bluestein.
Column paths of a 2D plan: DIRECT the power-of-two column pass, STRIDED its two-pass form, TRANSPOSE the transposed image
(n_passes = 0; every row count that is no power of two), ROWS a single row.
"""
import numpy as np

from ext_ladder import C64, C128, F32, F64  # noqa: F401
from mixed_radix_ladder import is_smooth7

MIXED, POW2, CHIRPZ = 1, 2, 3
ROWS, DIRECT, TRANSPOSE, STRIDED = 0, 1, 2, 3
SMALL = -1          # emulated cases: an LDS budget of 8192 (fp32) / 16384 (fp64) bytes, whose longest single pass is 76
MAX_L = 4096        # the longest single-pass length under the device's 160 KiB of LDS


def small_budget(dtype):
    return 8192 if np.dtype(dtype) in (C64, F32) else 16384


def engine(n):
    """The engine of a batched 1D transform of length n under FFT_GPU_ALGO_MIXED_RADIX."""
    return POW2 if n & (n - 1) == 0 else MIXED if is_smooth7(n) and n <= 1 << 23 else CHIRPZ


# (rows, cols, matrices, column path, engine of the transposed-image columns or None, property)
GPU_2D = [
    (6, 10, 3, TRANSPOSE, MIXED, "the smallest image that is mixed in both dimensions"),
    (15, 9, 3, TRANSPOSE, MIXED, "odd cols: 8-byte accesses on the fp32 side"),
    (360, 64, 3, TRANSPOSE, MIXED, "mixed columns, power-of-two rows of the image"),
    (1000, 64, 2, TRANSPOSE, MIXED, "mixed columns of 1000 rows: four transforms per tile (fp32), two (fp64)"),
    (360, 6, 3, TRANSPOSE, MIXED, "six columns per matrix: the last tile of the transposed image is ragged"),
    (64, 1000, 3, DIRECT, None, "mixed rows with the power-of-two column pass"),
    (1080, 30, 2, TRANSPOSE, MIXED, "1080 rows"),
    (1080, 1920, 1, TRANSPOSE, MIXED, "a full-HD frame"),
    (4200, 6, 2, TRANSPOSE, MIXED, "rows above a single pass: a two-pass mixed core on the transposed image"),
    (1009, 90, 2, TRANSPOSE, CHIRPZ, "chirp-z columns, mixed rows"),
    (1, 1000, 3, ROWS, None, "rows only"),
    (30, 64, 4000, TRANSPOSE, MIXED, "256000 column transforms of length 30: more tiles than 256 CUs x 8 workgroups, the persistent tile loop"),
]
# (rows, cols, matrices, lds_budget, column path, engine of the transposed-image columns, passes of that core, property); the
# emulated grid is 3 workgroups
EMU_2D = [
    (6, 10, 3, 0, TRANSPOSE, MIXED, 1, "the smallest image mixed in both dimensions"),
    (15, 9, 3, 0, TRANSPOSE, MIXED, 1, "odd cols: 8-byte accesses in fp32"),
    (36, 64, 3, 0, TRANSPOSE, MIXED, 1, "mixed columns, power-of-two rows of the image"),
    (100, 12, 2, 0, TRANSPOSE, MIXED, 1, "mixed columns, mixed rows of the image"),
    (36, 6, 3, 0, TRANSPOSE, MIXED, 1, "six columns per matrix: the last tile of the transposed image is ragged"),
    (1000, 8, 2, 0, TRANSPOSE, MIXED, 1, "1000 rows"),
    (64, 100, 3, 0, DIRECT, None, 0, "mixed rows with the power-of-two column pass"),
    (1080, 6, 1, 0, TRANSPOSE, MIXED, 1, "1080 rows"),
    (210, 6, 2, SMALL, TRANSPOSE, MIXED, 2, "rows above a single pass of this budget: a two-pass mixed core on the transposed image"),
    (101, 90, 2, 0, TRANSPOSE, CHIRPZ, 0, "chirp-z columns, mixed rows"),
    (1, 100, 3, 0, ROWS, None, 0, "rows only"),
    (30, 8, 40, 0, TRANSPOSE, MIXED, 1, "320 column transforms: more tiles than the 3 workgroups"),
]

# real transforms: (n, batch, policy, engine of the core, passes of a mixed core or None, property)
GPU_REAL = [
    (6, 5, {}, MIXED, 1, "h = 3"),
    (10, 5, {}, MIXED, 1, "h = 5"),
    (12, 5, {}, MIXED, 1, "h = 6: the pairs k = 0 and 2k = h"),
    (30, 5, {}, MIXED, 1, "h = 15: odd half length"),
    (1000, 37, {}, MIXED, 1, "odd batch, a ragged last tile"),
    (1080, 37, {}, MIXED, 1, "odd batch, a ragged last tile"),
    (2000, 37, {}, MIXED, 1, "h = 1000, even"),
    (7938, 7, {}, MIXED, 1, "h = 3969 = 3^4 7^2: the longest odd single-pass half length"),
    (8190, 7, {}, CHIRPZ, None, "h = 4095 = 3^2 5 7 13 is not 7-smooth: chirp-z whatever the algorithm"),
    (1000, 20001, {}, MIXED, 1, "2501 tiles of 8 rows > 256 CUs x 8 workgroups: the persistent tile loop of the row pass"),
    (44100, 3, {}, MIXED, 2, "a two-pass core"),
    (10 ** 6, 3, {"chunk_mb": 4}, MIXED, 2, "a two-pass core in launch groups of one transform"),
    (945, 5, {}, MIXED, 1, "odd n = 3^3 5 7: promoted to length n"),
    (64, 250000, {}, POW2, None, "a power of two keeps the power-of-two plan"),
    (1006, 5, {}, CHIRPZ, None, "h = 503 is prime: chirp-z whatever the algorithm"),
]
# (n, batch, lds_budget, engine, passes, property)
EMU_REAL = [(n, b, 0, MIXED, 1, "small half lengths") for n in (6, 10, 12, 30) for b in (1, 5)] + [
    (200, 37, 0, MIXED, 1, "odd batch, ragged last tile"),
    (360, 140, 0, MIXED, 1, "more tiles than the 3 workgroups"),
    (90, 5, 0, MIXED, 1, "h = 45: odd half length"),
    (420, 3, SMALL, MIXED, 2, "h = 210 above a single pass of this budget: a two-pass core"),
    (945, 3, 0, MIXED, 1, "odd n: promoted"),
    (105, 5, 0, MIXED, 1, "odd n: promoted"),
    (64, 5, 0, POW2, None, "a power of two keeps the power-of-two plan"),
    (1006, 3, 0, CHIRPZ, None, "h = 503: chirp-z"),
]
