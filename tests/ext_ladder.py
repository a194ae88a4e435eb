"""The cases at which the plans built on the batched engine (csrc/fft_plans_ext.h: Plan2D, RealPlan, FusedPlan) are checked row by
row against float64, on the GPU (tests/test_gpu_ext_every_row.py) and in the CPU emulation (tests/test_emulated_ext.py), with the
inputs and the float64 references both files share.  Test infrastructure only.

Every case names the property it is there for, and the path it must take: the tests assert the path (plan.info() on the device,
the emulation's info words), so a planner change that moves a case off its path fails here and the case gets a new size.

2D paths (Plan2D::build): the DIRECT column pass needs rows a power of two, cols % V == 0 (V = 2 values for fp32, 1 for fp64) and
a column tile with >= 64-byte segments (rows <= 1024 under the device's LDS budget); power-of-two rows beyond that with
cols % V == 0 take two STRIDED passes; everything else the TRANSPOSE path; a single row has no column transform (ROWS).
"""
import numpy as np

import accuracy as A

C64, C128 = np.dtype(np.complex64), np.dtype(np.complex128)
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DIRECT, TRANSPOSE, STRIDED, ROWS = 1, 2, 3, 0  # the emulation's info[0]; on the device n_passes = 1, 0, 2, 0

# (rows, cols, matrices, dtype, path, property)
GPU_2D = [
    (1024, 8, 3, C64, DIRECT, "the narrowest column segment the direct pass accepts (64 bytes)"),
    (64, 6, 3, C64, DIRECT, "column count not a power of two: the last column tile is part padding, rows through Bluestein"),
    (2, 2, 5, C64, DIRECT, "the smallest image"),
    (2048, 8, 3, C64, STRIDED, "two strided passes, fp32"),
    (2048, 4, 3, C128, STRIDED, "two strided passes, fp64"),
    (8192, 6, 2, C64, STRIDED, "unequal factors and a padded column tile"),
    (64, 5, 3, C64, TRANSPOSE, "odd column count: no 16-byte lane access"),
    (12, 32, 3, C128, TRANSPOSE, "rows not a power of two: Bluestein on the transposed image"),
    (2048, 3, 2, C64, TRANSPOSE, "long columns, odd count"),
    (33, 17, 3, C64, TRANSPOSE, "transpose tiles ragged in both dimensions"),
    (33, 33, 16400, C64, TRANSPOSE, "65600 transpose tiles > the 65536-workgroup grid: the tile loop (barrier at its head) runs twice"),
    (1, 4096, 3, C64, ROWS, "a single row: rows only"),
]
# (rows, cols, matrices, dtype, lds_budget, path, property)
EMU_2D = [
    (32, 64, 3, C64, 0, DIRECT, "direct column pass"),
    (64, 32, 1, C128, 0, DIRECT, "direct column pass, one matrix"),
    (16, 6, 5, C64, 0, DIRECT, "last column tile part padding, rows through Bluestein"),
    (2, 2, 5, C64, 0, DIRECT, "the smallest image"),
    (8, 5, 3, C64, 0, TRANSPOSE, "odd column count"),
    (12, 32, 3, C128, 0, TRANSPOSE, "rows not a power of two"),
    (33, 17, 3, C64, 0, TRANSPOSE, "tiles ragged in both dimensions"),
    (33, 33, 5, C64, 0, TRANSPOSE, "nine ragged tiles per matrix"),
    (256, 8, 3, C64, 1024, STRIDED, "rows do not fit one tile of this budget: 16 x 16"),
    (64, 32, 3, C128, 4096, STRIDED, "the one-pass tile would be narrow: 8 x 8"),
    (512, 8, 1, C64, 2048, STRIDED, "32 x 16: unequal factors"),
    (128, 6, 5, C64, 1024, STRIDED, "padded column tile"),
    (1, 64, 37, C64, 0, ROWS, "rows only"),
]

# real transforms: (n, batch, dtype, policy, expect, property); policy: fftlib.set_policy arguments, expect: plan.info() fields
# of the complex core (chunk_lt: chunk_batch below it)
GPU_REAL = [
    (1, 5, F64, {}, {}, "h = 0: the odd-length kernels at n = 1"),
    (2, 5, F32, {}, {}, "h = 1: a length-1 core"),
    (4, 5, F64, {}, {}, "h = 2: only the pairs k = 0 and 2k = h"),
    (6, 5, F32, {}, {"bluestein": True}, "h = 3"),
    (1006, 5, F32, {}, {"bluestein": True}, "h = 503 is prime: Bluestein on the half length"),
    (1006, 5, F64, {}, {"bluestein": True}, "h = 503, fp64"),
    (1009, 5, F32, {}, {"bluestein": True}, "odd n: promote / extend / copy kernels"),
    (1009, 3, F64, {}, {"bluestein": True}, "odd n, fp64"),
    (4096, 37, F32, {}, {"n_passes": 1}, "single-pass core, odd batch"),
    (8192, 37, F64, {}, {"n_passes": 1}, "single-pass core, odd batch, fp64"),
    (1 << 17, 5, F32, {"chunk_mb": 1}, {"n_passes": 2, "chunk_lt": 5}, "the half-length core runs in several launch groups"),
    (1 << 16, 9, F32, {"team": 2, "min_batch": 1}, {"team_kernel": True}, "the core runs on a team kernel and writes the plan's work buffer"),
    (64, 250000, F32, {}, {"n_passes": 1}, "batch * (h/2 + 1) = 4.25 M pairs > launch_flat's 4194304 threads: a second grid-stride trip"),
]
EMU_REAL = [(n, b) for n in (1, 2, 3, 4, 6, 8, 9, 31, 64, 100, 101, 1006, 1024) for b in (1, 5)] + [(64, 37), (6, 37), (9, 37)]

# fused consumers: (kind, nx, nh, batch, dtype, policy, fused, expect, property); fused: info().fused of the default plan
GPU_FUSED = [
    ("conv", 999, 27, 1031, C64, {}, 3, {"n_passes": 1}, "one-kernel round trip, odd pitch on both sides (ny = 1025, m = 2048)"),
    ("conv", 999, 27, 1031, C128, {}, 3, {"n_passes": 1}, "the same in fp64"),
    ("conv", 1000, 25, 37, C64, {}, 3, {"n_passes": 1}, "ny == m exactly"),
    ("conv", 1000, 26, 37, C64, {}, 3, {"n_passes": 1}, "ny = m/2 + 1"),
    ("conv", 25, 1000, 37, C64, {}, 3, {"n_passes": 1}, "kernel longer than the signal"),
    ("conv", 1, 1, 5, C64, {}, 0, {}, "m = 1 is not hook-capable"),
    ("conv", 1, 7, 5, C64, {}, 3, {"n_passes": 1}, "nx = 1"),
    ("conv", 9001, 101, 7, C64, {}, 2, {"n_passes": 2}, "two-pass hooked ends with odd pitches (ny = 9101, m = 16384)"),
    ("xcorr", 4097, 0, 19, C64, {"chunk_mb": 1}, 2, {"n_passes": 2, "chunk": 8}, "launch groups 8 + 8 + 3: the table offset b0 * post_tab_b"),
    ("autocorr", 4097, 0, 19, C128, {"chunk_mb": 1}, 2, {"n_passes": 2, "chunk": 4}, "launch groups, fp64"),
    ("xcorr", 1500001, 0, 3, C64, {"chunk_mb": 64}, 2, {"n_passes": 3, "chunk": 2}, "three passes, launch groups of 2 + 1"),
    ("circ", 4096, 0, 37, C64, {}, 3, {"n_passes": 1}, "circular, single pass"),
    # 8192 fp32 is a wide_row_kernel size, and that kernel has no hooks: a plan that wants hooks never builds it (Pow2Plan::build
    # skips build_wide under wants_hooks) and keeps the two-pass hooked schedule instead of dropping to the unfused kernels
    ("circ", 8192, 0, 37, C64, {}, 2, {"n_passes": 2}, "a wide-row size: the fused plan keeps the two-pass hooked schedule"),
    ("circ", 65536, 0, 5, C64, {}, 2, {"n_passes": 2}, "circular, two passes"),
    ("psd", 2, 0, 37, C64, {}, None, {}, "nx = 2: no bin is doubled (k = 0 and k = nx/2 only)"),
    ("psd", 4096, 0, 37, C64, {}, 1, {"n_passes": 1}, "rows of 2049 reals: row starts only 4-byte aligned"),
    ("psd", 8192, 0, 37, C128, {}, None, {}, "rows of 4097 doubles"),
    ("psd", 65536, 0, 37, C64, {}, 1, {"n_passes": 2}, "two passes"),
    ("psd", 64, 0, 131000, C64, {}, 1, {"n_passes": 1}, "batch * (nx/2 + 1) = 4.3 M > launch_flat's 4194304 threads"),
]
# (kind, nx, nh, batch, dtype, lds_budget, fused, passes, property); fused / passes: the emulation's info[1] / info[0]
EMU_FUSED = [
    ("conv", 99, 27, 37, C64, 0, 3, 1, "one-kernel round trip, odd pitch on both sides (ny = 125)"),
    ("conv", 99, 27, 5, C128, 0, 3, 1, "the same in fp64"),
    ("conv", 101, 8, 5, C64, 0, 3, 1, "odd input pitch, even output pitch"),
    ("conv", 100, 29, 1, C64, 0, 3, 1, "ny == m, batch 1"),
    ("conv", 100, 30, 5, C64, 0, 3, 1, "ny = m/2 + 1 (m = 256)"),
    ("conv", 25, 100, 5, C64, 0, 3, 1, "kernel longer than the signal"),
    ("conv", 1, 1, 5, C64, 0, 0, 0, "m = 1 is not hook-capable"),
    ("conv", 1, 7, 5, C64, 0, 3, 1, "nx = 1"),
    ("conv", 901, 101, 5, C64, 4096, 2, 2, "two-pass hooked ends with odd pitches (ny = 1001)"),
    ("conv", 700, 401, 5, C128, 8192, 2, 2, "two passes, fp64"),
    ("conv", 2000, 148, 5, C64, 4096, 2, 3, "three passes"),
    ("circ", 64, 0, 5, C128, 0, 3, 1, "circular, single pass"),
    ("circ", 2048, 0, 5, C64, 4096, 2, 2, "circular, two passes"),
    ("autocorr", 100, 0, 5, C128, 0, 3, 1, "autocorrelation, single pass"),
    ("autocorr", 1001, 0, 5, C64, 4096, 2, 2, "autocorrelation, odd pitch, two passes"),
    ("xcorr", 333, 0, 37, C64, 0, 1, 1, "per-transform product: two kernels, odd pitch"),
    ("xcorr", 100, 0, 1, C128, 0, 1, 1, "batch 1"),
    ("xcorr", 1500, 0, 5, C128, 4096, 2, 3, "three passes"),
    ("psd", 2, 0, 37, C64, 0, 0, 1, "nx = 2"),
    ("psd", 64, 0, 37, C128, 0, 1, 1, "rows of 33 doubles"),
    ("psd", 1024, 0, 5, C64, 0, 1, 1, "rows of 513 floats: 4-byte aligned row starts"),
    ("psd", 4096, 0, 5, C128, 4096, 1, 3, "three passes"),
]

FUSED_FAMILY = {"conv": "fused_conv", "circ": "fused_conv", "autocorr": "fused_corr", "xcorr": "fused_corr", "psd": "psd"}


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def complex_rows(width, batch, dtype, seed):
    """[batch][width] complex normal values; neighbouring rows differ (accuracy.block_normal_rows)."""
    return A.block_normal_rows(width, 0, batch, dtype, seed)


def real_rows(width, batch, dtype, seed):
    """[batch][width] real normal values of dtype float32 / float64."""
    cdt = C64 if np.dtype(dtype) == F32 else C128
    return np.ascontiguousarray(A.block_normal_rows((width + 1) // 2, 0, batch, cdt, seed).view(dtype)[:, :width])


def half_spectra(n, batch, dtype, seed):
    """[batch][n/2 + 1] random Hermitian half spectra (complex dtype) of real signals of length n: the imaginary parts of bin 0 and,
    for even n, of bin n/2 are zero.  c2r_merge_kernel propagates those imaginary parts into the result where numpy's irfft ignores
    them, so only spectra that a real signal can have are compared."""
    X = complex_rows(n // 2 + 1, batch, dtype, seed).copy()
    X[:, 0] = X[:, 0].real
    if n % 2 == 0:
        X[:, -1] = X[:, -1].real
    return X


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references (numpy / scipy on the complex128 or float64 copy of the input rows)
# ---------------------------------------------------------------------------------------------------------------------------
def _fft(x, n=None, inverse=False):
    if A._sfft is not None:
        return (A._sfft.ifft if inverse else A._sfft.fft)(x, n=n, axis=-1, workers=A.WORKERS)
    return (np.fft.ifft if inverse else np.fft.fft)(x, n=n, axis=-1)


def ref_2d(rows, cols, direction):
    def ref(xs):
        xs = np.asarray(xs, dtype=np.complex128).reshape(-1, rows, cols)
        return (np.fft.fft2(xs) if direction < 0 else np.fft.ifft2(xs)).reshape(xs.shape[0], -1)
    return ref


def ref_r2c(xs):
    return np.fft.rfft(np.asarray(xs, dtype=np.float64), axis=-1)


def ref_c2r(n):
    return lambda Xs: np.fft.irfft(np.asarray(Xs, dtype=np.complex128), n, axis=-1)


def fused_m(kind, nx, nh):
    """The padded power-of-two length of FusedPlan::build."""
    need = nx + nh - 1 if kind == "conv" else 2 * nx if kind in ("autocorr", "xcorr") else nx
    m = 1
    while m < need:
        m <<= 1
    return m


def fused_out(kind, nx, nh, dtype):
    """(row width, dtype) of the result."""
    if kind == "psd":
        return nx // 2 + 1, (F32 if np.dtype(dtype) == C64 else F64)
    return (nx + nh - 1 if kind == "conv" else nx), np.dtype(dtype)


def hann(nx):
    """The window of the periodogram (FusedPlan::build), in float64."""
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(nx) / (nx - 1))) if nx > 1 else np.ones(1)


def ref_fused(kind, nx, nh, h=None, fs=1.0):
    """ref(xs) (xcorr: ref(xs, ys)) of the fused consumer, from np.fft on the complex128 copy of the rows."""
    m = fused_m(kind, nx, nh)
    if kind in ("conv", "circ"):
        H = _fft(np.asarray(h, dtype=np.complex128), n=m)
        ny = nx + nh - 1 if kind == "conv" else nx
        return lambda xs: _fft(_fft(np.asarray(xs, dtype=np.complex128), n=m) * H, inverse=True)[:, :ny]
    if kind == "autocorr":
        return lambda xs: _fft(np.abs(_fft(np.asarray(xs, dtype=np.complex128), n=m)) ** 2, inverse=True)[:, :nx]
    if kind == "xcorr":
        return lambda xs, ys: _fft(np.conj(_fft(np.asarray(xs, dtype=np.complex128), n=m)) * _fft(np.asarray(ys, dtype=np.complex128), n=m),
                                   inverse=True)[:, :nx]
    w = hann(nx)

    def psd(xs):
        p = np.abs(_fft(np.asarray(xs, dtype=np.complex128) * w)[:, :nx // 2 + 1]) ** 2 / (fs * 0.375 * nx)
        p[:, 1:nx // 2] *= 2.0  # doubled for 0 < k < nx/2: never bin 0, never bin nx/2
        return p
    return psd
