"""The batch ladder of the single-pass sizes n = 2^0 ... 2^12: the batches at which the GPU tests run every LDS algorithm, chosen so
that the single-pass kernel meets every tile shape the planner gives it.  Test infrastructure only.

The single-pass tile holds C transforms, C = min(next_pow2(batch), Cmax(n)) (csrc/fft_engine.h: the batch extent rounded up and
passed to choose_tile), so the kernel's shape -- thread count, LDS layout, instantiation -- depends on the batch.  CMAX is the
tile the planner picks at large batches under the 160 KiB LDS budget of gfx950; it is the same for auto, radix2, radix4 and
split_radix.  For fp32 n = 128 ... 4096 it is the full tile log2 C = 13 - log2 n, the only tile that the instantiations with the
shape baked in (ROWS_FIX, ROWS_FIX8) run.  tests/test_emulated_kernels.py checks this table, and that the ladder reaches every
tile, against the planner on the CPU.

The ladder of n >= 2:
  - 1, 2, 3;
  - C - 1, C, C + 1 for C = 4, 8, ..., Cmax (a partly filled, a full, and the next tile);
  - 2 Cmax + 1 (two full tiles and a ragged one);
  - many(n) = 6145 Cmax - ceil(Cmax / 2): a ragged tail behind more than three tiles per workgroup of the persistent grid, which has
    at most 256 CUs x 8 resident workgroups = 2048 workgroups.
n = 1 has no tile (a scale copy whose grid stops at 16384 x 256 threads): 1, 2, 3 and 2^22 + 3.
"""
import numpy as np

LDS_BUDGET = 160 << 10  # bytes of LDS per workgroup the gfx950 backend plans with (fft_hip_backend.hip)

# Cmax by log2 n (index 0: n = 1 has no tile)
CMAX = {
    np.dtype(np.complex64): (None, 512, 512, 256, 128, 64, 64, 64, 32, 16, 8, 4, 2),
    np.dtype(np.complex128): (None, 256, 256, 128, 64, 32, 32, 32, 16, 8, 4, 2, 1),
}
N1_LADDER = (1, 2, 3, (1 << 22) + 3)
LOG2N = tuple(range(13))
DTYPES = (np.dtype(np.complex64), np.dtype(np.complex128))
ALGOS = ("auto", "radix2", "radix4", "split_radix")


def cmax(log2n, dtype):
    return CMAX[np.dtype(dtype)][log2n]


def many(log2n, dtype):
    c = cmax(log2n, dtype)
    return 6145 * c - (c + 1) // 2


def ladder(log2n, dtype):
    """The ladder of one size and precision, ascending."""
    if log2n == 0:
        return N1_LADDER
    c = cmax(log2n, dtype)
    b = {1, 2, 3, 2 * c + 1, many(log2n, dtype)}
    t = 4
    while t <= c:
        b |= {t - 1, t, t + 1}
        t *= 2
    return tuple(sorted(b))


LADDER = {(log2n, dt): ladder(log2n, dt) for log2n in LOG2N for dt in DTYPES}


def explicit_batches(log2n, dtype):
    """The thinner set of the explicit families: 1, 3, Cmax - 1, Cmax + 1, many(n)."""
    if log2n == 0:
        return N1_LADDER
    c = cmax(log2n, dtype)
    return tuple(sorted({1, 3, max(1, c - 1), c + 1, many(log2n, dtype)}))
