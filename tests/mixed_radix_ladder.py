"""Sizes and batch ladders of the mixed-radix tests (csrc/fft_mixed_radix.h, ffteng::MixedRadixPlan).  Test infrastructure only.

tile_rows() restates the planner's choice of C, the transforms per tile of a single-pass plan (MixedRadixPlan::make_pass, rows in
and rows out); tests/test_emulated_mixed_radix.py checks it against the planner on the CPU.  A workgroup needs
lds_bytes() of LDS, so at most 160 KiB // lds_bytes() of them (and at most 8: 32 waves of 64 lanes, 4 per workgroup) share a CU;
fill_batch() is the batch that fills a grid of 256 CUs once."""
import numpy as np

MAX_L = 4096
MAX_N = 1 << 23
LDS_BUDGET = 160 << 10
DTYPES = (np.dtype(np.complex64), np.dtype(np.complex128))


def is_smooth7(n):
    if n < 1:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def smooth_numbers(limit):
    out = []
    a = 1
    while a <= limit:
        b = a
        while b <= limit:
            c = b
            while c <= limit:
                d = c
                while d <= limit:
                    out.append(d)
                    d *= 7
                c *= 5
            b *= 3
        a *= 2
    return sorted(out)


# every 7-smooth n <= 4096 that is no power of two: the single-pass sizes of the plan (235 of them)
SINGLE_PASS = tuple(n for n in smooth_numbers(MAX_L) if n & (n - 1))
# every radix and the alignment cases (odd n, odd n with an even tile, n just under the limit)
LADDER_SIZES = (6, 15, 35, 49, 105, 243, 343, 625, 1000, 1029, 1080, 1920, 2187, 2401, 3000, 3125, 3600, 4000, 4032, 4050)
TWO_PASS = (4200, 4375, 5000, 6561, 10000, 16807, 44100, 65610, 100000, 117649, 10 ** 6, 2073600, 5764801, 8294400)


def tile_rows(n, dtype, batch):
    dt = np.dtype(dtype)
    v = 16 // dt.itemsize
    cap = 8192 if v == 2 else 4096
    target = 4096 if v == 2 else 2048
    c = max(1, min(target // n, batch))
    if v == 2 and (c * n) % 2 and c < batch and (c + 1) * n <= cap:
        c += 1
    return c


def lds_bytes(n, dtype, c):
    dt = np.dtype(dtype)
    tables = n if n <= 1024 else 64 + ((n - 1) >> 6) + 1
    tables += tables & 1
    image = (c * (n | 1) + 1) & ~1
    return (2 * image + tables) * dt.itemsize


def fill_batch(n, dtype):
    c = tile_rows(n, dtype, 1 << 30)
    per_cu = max(1, min(8, LDS_BUDGET // lds_bytes(n, dtype, c)))
    return c * 256 * per_cu


def ladder(n, dtype):
    f = fill_batch(n, dtype)
    return tuple(sorted({1, 7, f - 1, f + 1, (1 << 24) // n + 3}))
