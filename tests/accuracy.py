"""Per-transform, per-bin accuracy checks of the engine against a float64 (or longer) reference.  Test infrastructure only.

The metric of transform b is its worst bin in units of the transform's RMS bin magnitude:

    e_b = max_k |y[b, k] - X[b, k]| / (||X_b||_2 / sqrt(n))

It is scale-free, so the same definition serves forward, inverse (1/n), r2c / c2r and 2D results; a NaN or Inf gives
e_b = inf.  Unlike a rel-L2 over a whole batch it does not average a defect confined to a few bins of one transform over
sqrt(batch * n) values: one wrong bin, a value pair from a neighbouring transform or two swapped transforms all fail.

The bound is K * u * log2(n) (Bluestein: log2(m), m the padded length), u = 2^-24 for fp32 and 2^-53 for fp64, one K per path
family (BOUND_K).  The reference of an fp32 result is the complex128 transform of the fp32 input itself, so input rounding is not
charged to the kernel; fp64 results are also compared, on a few transforms, with a long-double transform (numpy >= 2 computes
np.fft in the input's precision), which shows that the float64 reference's own error is small against the fp64 bound.

check_execute() runs a batch through a raw-pointer execute into a NaN-filled output that sits between two guard transforms of a
sentinel pattern, and checks every transform, the guards, the untouched input of an out-of-place execute and the bit identity of
the in-place result with the out-of-place one.

check_execute_io() is the same for executes whose input and output rows differ in width or type (2D, r2c / c2r, the fused
consumers; an optional second input): every buffer has guards of its own size.  The fused families measure bin k's error in units
of max(RMS_b, |X[b, k]|) (row_errors(scale="rms_or_bin")): a correlation's lag 0 is ~ n sigma^2 where the other lags are
~ sqrt(n) sigma^2, so the peak's own rounding error, in units of the row's RMS, grows like sqrt(n) and says nothing about the
kernel (CPU emulation, autocorrelation of nx = 4095, RMS units: 18.4 / 16.2 u log2 m; nx = 100: about 3); a periodogram's bins are
exponentially distributed and show the same, milder.  A wrong bin, a neighbour's value or swapped rows still fail.

The measured columns of the K tables below come from a GPU-suite run with FFT_ACCURACY_REPORT=<file>: at exit every process
merges the worst e_b / (u log2 n) it saw per family and precision into that JSON file.
"""
import atexit
import ctypes as C
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

try:
    import scipy.fft as _sfft
except ImportError:  # numpy's pocketfft is the same algorithm, only slower
    _sfft = None

WORKERS = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", 16))))  # never os.cpu_count(): a shared host has many more
SLICE_BYTES = 1 << 30  # complex128 reference computed in slices of at most 1 GiB

U = {np.dtype(np.complex64): 2.0 ** -24, np.dtype(np.complex128): 2.0 ** -53,
     np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}

# K of the bound K * u * log2(n) per path family, and the worst e_b / (u * log2 n) measured on the MI355X over the GPU suite
# (fp32 / fp64).  Each K is at least twice the worst measured value; caps: 16 for the power-of-two paths (r2c, c2r and 2d among
# them), 64 for Bluestein and for the fused families, which have its structure: two transforms of length m with a product between.
BOUND_K = {
    "multipass": 8,    # multi-pass and single-pass schedules (csrc/fft_kernels.h)       measured 2.16 (2^4) / 2.58 (2^4)
    "radix2_global": 8,  # bitrev_kernel + radix2_dit_stage_kernel, one launch per stage   measured 1.98 (2^6) / 2.06 (2^3)
    "radix2_shfl": 8,    # wave_dit_kernel: one wavefront per transform, n = 128 ... 1024  measured 1.57 (2^9) / 2.18 (2^7)
    "wide_row": 9,     # wide_row_kernel: fp32 n = 8192, 16384, fp64 n = 8192              measured 4.21 / 1.25 (2^13); fp32 2^13 x (2^18 + 1): 5.25, over K / 2 (open)
    "team_quad": 8,    # team_quad_kernel (csrc/fft_team_quad.h)                          measured 3.74 (2^20) / 2.18 (2^16)
    "team_defer": 8,   # team_defer_kernel / team_fft_kernel (csrc/fft_team*.h)          measured   -  / 1.91 (2^17); no fp32 size runs them
    "bluestein": 32,   # chirp-z over a power-of-two core of length m                     measured 1.81 (1000) / 2.41 (100003)
    "r2c": 8,          # r2c / c2r on a half-length complex transform                     measured 1.50 (1009) / 1.58 (1000)
    "2d": 8,           # rows + strided columns, log2(rows * cols)                         measured 0.78 / 0.80 (256 x 512)
    # the families below: worst over the emulated cases of tests/ext_ladder.py (tests/test_emulated_ext.py), fp32 / fp64, as merged in
    # profiles/ext_accuracy_report.json; r2c and 2d there: 1.77 / 2.69 (n = 6) and 1.49 (33 x 33) / 1.10 (12 x 32)
    "c2r": 8,          # c2r_merge_kernel + half-length inverse (odd n: extend + full length)      measured 1.94 (9) / 2.60 (1006)
    "fused_conv": 8,   # linear / circular convolution, log2(m); error / max(RMS, |bin|)           measured 1.20 (circular 2048) / 1.21 (99 + 27)
    "fused_corr": 8,   # auto- / cross-correlation, log2(m); error / max(RMS, |bin|)               measured 1.81 (1500) / 1.25 (1500)
    "psd": 8,          # Hann periodogram, log2(nx); error / max(RMS, |bin|)                       measured 0.74 (1024) / 2.07 (64)
}
# Two-tone inputs (oracle_lib.gen_two_tone: all the energy in two bins) against their analytic spectrum.  On them the device's
# worst bin is NOT bounded by K u log2(n): twiddles formed as powers of one table value (quad_stage1 / quad_twiddle_kb in
# csrc/fft_team_quad.h) err coherently, and the error of the two peaks gathers into spurs that grow with sqrt(n); the
# multi-pass schedule shows the same, smaller (its cause not traced) (numpy's fp32 FFT: worst bin 0.03 - 0.16 u log2(n) on the same inputs).  An open accuracy finding; these bounds
# pin it against regressions: max |y - X| / RMS <= K2 * u * log2(n) * sqrt(n), K2 at least twice the worst measured value.
TWO_TONE_K = {
    "multipass": 0.25,  # measured 0.121 (2^16, config 2 in chunks of 256)
    "team_quad": 1.0,   # measured 0.461 (worst of 2^16, 2^18, 2^20: at 2^18)
}
CAP = {"bluestein": 64, "fused_conv": 64, "fused_corr": 64, "psd": 64}
POW2_CAP = 16
# Unit impulses against the closed-form column of the DFT matrix (tests/operator_ladder.py; check_rows(kind="impulse")): the bound
# is the family's BOUND_K unless a family is pinned here with a K of its own (at least twice its measured value, within the caps).
# The measured column is operator_ladder.MEASURED; no family needs an entry.
IMPULSE_K = {}

# worst measured e_b / (u * log2 n) per (family, precision) in this process; FFT_ACCURACY_REPORT=<file> writes it out as JSON
WORST = {}


def bound(family, dtype, n, m=None, kind=None):
    """K * u * log2(n) (log2(m) for Bluestein, m = the padded power-of-two length).  kind="impulse": K from IMPULSE_K where the
    family has an entry there."""
    length = m if m else n
    K = IMPULSE_K.get(family, BOUND_K[family]) if kind == "impulse" else BOUND_K[family]
    return K * U[np.dtype(dtype)] * max(1.0, np.log2(length))


def bound_two_tone(family, dtype, n):
    """TWO_TONE_K * u * log2(n) * sqrt(n): the worst bin of a two-tone transform, in units of its RMS bin magnitude."""
    return TWO_TONE_K[family] * U[np.dtype(dtype)] * max(1.0, np.log2(n)) * np.sqrt(n)


def _note(family, dtype, n, m, e, unit=None):
    e = float(np.max(e)) if np.size(e) else 0.0
    key = "%s/%s" % (family, "fp32" if np.dtype(dtype) in (np.dtype(np.complex64), np.dtype(np.float32)) else "fp64")
    k = e / (unit or U[np.dtype(dtype)] * max(1.0, np.log2(m if m else n)))
    if k > WORST.get(key, (0.0,))[0]:
        WORST[key] = (k, n)


@atexit.register
def _write_report():
    """FFT_ACCURACY_REPORT=<file>: merge this process's worst values into the JSON file (several test processes share it)."""
    path = os.environ.get("FFT_ACCURACY_REPORT")
    if not path or not WORST:
        return
    try:
        with open(path) as f:
            rep = json.load(f)
    except (OSError, ValueError):
        rep = {}
    for key, (k, n) in WORST.items():
        if k > rep.get(key, {}).get("K_measured", -1.0):
            rep[key] = {"K_measured": k, "n": n}
    with open(path, "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)


def check_two_tone(y, b0, n, family, label=""):
    """Every transform of y (rows b0 ..; two-tone inputs of oracle_lib.gen_two_tone) against its analytic spectrum X[f_b] = n,
    X[g_b] = n / 2, 0 elsewhere, bin by bin, the two peaks included: max |y - X| / RMS <= bound_two_tone(family) for every
    transform (RMS = sqrt(1.25 n)).  In slices of 64 rows: no complex128 copy of a 4 GiB batch."""
    import oracle_lib as O
    lim = bound_two_tone(family, y.dtype, n)
    rms = np.sqrt(1.25 * n)
    es, ks = [], []
    for s in range(0, y.shape[0], 64):
        yy = y[s:s + 64].astype(np.complex128)
        rows = np.arange(yy.shape[0])
        fg = np.array([O.two_tone_bins(n, b0 + s + i) for i in rows])
        yy[rows, fg[:, 0]] -= n
        yy[rows, fg[:, 1]] -= n / 2
        d = np.abs(yy)
        d = np.where(np.isnan(d), np.inf, d)
        k = np.argmax(d, axis=1)
        es.append(d[rows, k] / rms)
        ks.append(k)
    e, k = np.concatenate(es), np.concatenate(ks)
    _note("two_tone:" + family, y.dtype, n, None, e, unit=U[np.dtype(y.dtype)] * np.log2(n) * np.sqrt(n))
    assert_within(e, k, lim, "%s two-tone %s n=%d" % (label, family, n), b0)
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------------
def normal_rows(n, b0, count, dtype, seed):
    """Rows b0 .. b0 + count - 1 of a batch of complex normal values, row b drawn from default_rng((seed, b)): every transform
    differs from its neighbours, and any slice can be regenerated on its own.  dtype complex64 draws float32 values directly."""
    dt = np.dtype(dtype)
    real = np.float32 if dt == np.dtype(np.complex64) else np.float64
    out = np.empty((count, n), dtype=dt)

    def one(i):
        out[i] = np.random.default_rng((seed, b0 + i)).standard_normal(2 * n, dtype=real).view(dt)

    with ThreadPoolExecutor(WORKERS) as ex:
        list(ex.map(one, range(count)))
    return out


BLOCK_BYTES = 2 << 20  # block_normal_rows draws its rows in blocks of about 2 MiB, one generator per block


def block_rows(n, dtype):
    """Rows per block of block_normal_rows (at least one)."""
    return max(1, BLOCK_BYTES // (n * np.dtype(dtype).itemsize))


def block_normal_rows(n, b0, count, dtype, seed):
    """Rows b0 .. b0 + count - 1 of a batch of complex normal values drawn block by block: block j (rows j*R .. (j+1)*R - 1,
    R = block_rows(n, dtype)) comes from default_rng((seed, j)).  Any row range can be regenerated on its own, neighbouring
    transforms differ, and a batch of 2^27 rows needs only 2^27 / R generators (normal_rows makes one per row)."""
    dt = np.dtype(dtype)
    real = np.float32 if dt == np.dtype(np.complex64) else np.float64
    R = block_rows(n, dt)
    out = np.empty((count, n), dtype=dt)
    if count == 0:
        return out

    def one(j):
        lo, hi = max(b0, j * R), min(b0 + count, (j + 1) * R)
        blk = np.random.default_rng((seed, j)).standard_normal(2 * n * (hi - j * R), dtype=real).view(dt).reshape(-1, n)
        out[lo - b0:hi - b0] = blk[lo - j * R:]

    with ThreadPoolExecutor(WORKERS) as ex:
        list(ex.map(one, range(b0 // R, (b0 + count - 1) // R + 1)))
    return out


def fft_ref(x, direction, workers=WORKERS):
    """complex128 transform of the rows of x (inverse: scaled by 1/n, as the engine)."""
    x = np.asarray(x, dtype=np.complex128)
    if _sfft is not None:
        return _sfft.fft(x, axis=-1, workers=workers) if direction < 0 else _sfft.ifft(x, axis=-1, workers=workers)
    return np.fft.fft(x, axis=-1) if direction < 0 else np.fft.ifft(x, axis=-1)


def fft_ref_long(x, direction):
    """The same transform in extended precision (np.clongdouble)."""
    x = np.asarray(x).astype(np.clongdouble)
    return np.fft.fft(x, axis=-1) if direction < 0 else np.fft.ifft(x, axis=-1)


def row_errors(y, X, scale="rms"):
    """e_b of every row, and the bin of each row's worst error.  y: result rows (any precision), X: reference rows.
    scale="rms" (default): every bin's error in units of the row's RMS bin magnitude.  scale="rms_or_bin": bin k's error in
    units of max(RMS_b, |X[b, k]|) -- for rows with a few bins far above the rest (the lag 0 of a correlation, the peaks of a
    periodogram), whose own rounding error would otherwise be charged in units of the small bins."""
    y = np.asarray(y)
    X = np.asarray(X)
    d = np.abs(y.astype(X.dtype) - X)
    rms = np.maximum(np.sqrt(np.mean(np.abs(X) ** 2, axis=-1)), 1e-300)
    finite = np.all(np.isfinite(y.view(y.real.dtype) if np.iscomplexobj(y) else y).reshape(y.shape[0], -1), axis=-1)
    d = np.where(np.isnan(d), np.inf, d)
    if scale == "rms_or_bin":
        d = d / np.maximum(rms[:, None], np.abs(X))
    elif scale != "rms":
        raise ValueError("scale: 'rms' or 'rms_or_bin'")
    k = np.argmax(d, axis=-1)
    worst = d[np.arange(d.shape[0]), k]
    if scale == "rms":
        worst = worst / rms
    e = np.where(finite, worst, np.inf).astype(np.float64)
    return e, k


def errors_vs(y, x, direction, ref=None, b0=0, rows_per_task=None, scale="rms"):
    """e_b and worst bins of the rows y against ref(x rows) (default: the complex transform of x in `direction`), computed
    in row chunks on WORKERS threads (numpy and scipy release the GIL on whole arrays)."""
    nrows = y.shape[0]
    if nrows == 0:
        return np.zeros(0), np.zeros(0, dtype=np.int64)
    ref = ref or (lambda xs: fft_ref(xs, direction, workers=1))
    row_bytes = 16 * max(y.shape[-1], x.shape[-1])
    step = rows_per_task or max(1, min(-(-nrows // WORKERS), (64 << 20) // row_bytes))
    e = np.empty(nrows)
    k = np.empty(nrows, dtype=np.int64)

    def one(s):
        e[s:s + step], k[s:s + step] = row_errors(y[s:s + step], ref(x[s:s + step]), scale)

    with ThreadPoolExecutor(WORKERS) as ex:
        list(ex.map(one, range(0, nrows, step)))
    return e, k


class AccuracyError(AssertionError):
    pass


def assert_within(e, k, limit, label, b0=0):
    """Every e_b <= limit; else name the worst transform, its worst bin and the distribution of e_b over the batch."""
    e = np.asarray(e)
    bad = np.flatnonzero(~(e <= limit))
    if bad.size == 0:
        return
    w = int(np.argmax(np.where(np.isnan(e), np.inf, e)))
    fin = e[np.isfinite(e)]
    q = np.percentile(fin, [50, 90, 99, 100]) if fin.size else [np.inf] * 4
    raise AccuracyError(
        "%s: %d of %d transforms over the bound %.3g; worst transform %d (bin %d, e_b = %.3g = %.1f x bound); failing transforms %s%s; "
        "e_b median %.3g, p90 %.3g, p99 %.3g, max finite %.3g, non-finite %d"
        % (label, bad.size, e.size, limit, b0 + w, int(k[w]), e[w], e[w] / limit, [int(b0 + i) for i in bad[:12]],
           " ..." if bad.size > 12 else "", q[0], q[1], q[2], q[3], int(e.size - fin.size)))


def check_rows(y, x, direction, family, dtype=None, n=None, m=None, label="", ref=None, b0=0, long_rows=0, scale="rms", kind=None):
    """Check result rows y of input rows x against the reference: e_b <= bound(family) for every row.  Returns e.
    scale: the unit of a bin's error, see row_errors().  kind (e.g. "impulse"): the worst value is recorded under
    "<kind>:<family>" and the bound is bound(family, kind=kind).
    long_rows > 0 (fp64 results): also compare the first rows with a long-double reference, and show that the float64
    reference's own error is below a quarter of the bound."""
    dtype = np.dtype(dtype or y.dtype)
    n = n or y.shape[-1]
    lim = bound(family, dtype, n, m, kind)
    e, k = errors_vs(y, x, direction, ref, scale=scale)
    _note("%s:%s" % (kind, family) if kind else family, dtype, n, m, e)
    if kind and e.size:  # the figure before anything asserts on it
        w = int(np.argmax(np.where(np.isnan(e), np.inf, e)))
        print("%s %s %s: worst e / (u log2 %s) = %.3f (row %d, bin %d)" % (kind, label, np.dtype(dtype).name, "m" if m else "n",
              float(e[w]) / (U[np.dtype(dtype)] * max(1.0, np.log2(m if m else n))), b0 + w, int(k[w])))
    assert_within(e, k, lim, "%s %s n=%d dir=%+d" % (label, family, n, direction), b0)
    if long_rows and ref is None:
        rows = min(long_rows, y.shape[0])
        XL = fft_ref_long(x[:rows], direction)
        e64, k64 = row_errors(fft_ref(x[:rows], direction), XL)
        assert_within(e64, k64, lim / 4, "float64 reference vs long double, n=%d" % n, b0)
        eL, kL = row_errors(y[:rows].astype(np.clongdouble), XL)
        assert_within(eL, kL, lim, "%s %s n=%d dir=%+d vs long double" % (label, family, n, direction), b0)
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# device side: guarded buffers and raw-pointer executes
# ---------------------------------------------------------------------------------------------------------------------------
class HipMemory:
    """Device memory of the product library, and copies at byte offsets through the HIP runtime that library is linked
    against (a process may hold more than one HIP runtime, e.g. one that came with torch)."""

    def __init__(self):
        import fftlib
        self.lib = fftlib.load()  # hipMemcpy looked up through the product library: the runtime it is linked against
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipMemcpy.restype = C.c_int

    def alloc(self, nbytes):
        import fftlib
        buf = fftlib.DeviceBuffer(nbytes)
        return buf.ptr, buf

    def free(self, handle):
        handle.free()

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        if self.lib.hipMemcpy(dptr, arr.ctypes.data, arr.nbytes, 1) != 0:  # hipMemcpyHostToDevice
            raise RuntimeError("hipMemcpy h2d failed")

    def d2h(self, dptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if self.lib.hipMemcpy(out.ctypes.data, dptr, out.nbytes, 2) != 0:  # hipMemcpyDeviceToHost
            raise RuntimeError("hipMemcpy d2h failed")
        return out


MEMORY = None  # the memory Guarded buffers live in (tests/test_accuracy_checker.py puts host memory here)


def memory():
    global MEMORY
    if MEMORY is None:
        MEMORY = HipMemory()
    return MEMORY


def h2d(dptr, arr):
    memory().h2d(dptr, arr)


def d2h(dptr, shape, dtype):
    return memory().d2h(dptr, shape, dtype)


SENTINEL = np.uint32(0x7F8A5A5A)  # a NaN payload no kernel writes


def _slice_rows(row_bytes):
    return max(1, SLICE_BYTES // max(1, row_bytes))


class Guarded:
    """`rows` rows of `row_bytes` bytes with one guard row of SENTINEL words before and one after, in one allocation.
    ptr = the first payload row; with row_bytes >= 16 it keeps the allocation's 16-byte alignment.
    align16=True (rows of any width, check_execute_io): each guard is the smallest multiple of 16 bytes >= one row, so that
    the payload starts 16-byte aligned, like a plain allocation's, whatever row_bytes is; the trailing guard starts right
    behind the last payload byte."""

    def __init__(self, rows, row_bytes, align16=False):
        assert row_bytes % 4 == 0 and row_bytes > 0
        self.rows, self.row_bytes = rows, row_bytes
        self.guard_bytes = -(-row_bytes // 16) * 16 if align16 else row_bytes
        self.base, self.handle = memory().alloc(rows * row_bytes + 2 * self.guard_bytes)
        self.ptr = self.base + self.guard_bytes
        g = np.full(self.guard_bytes // 4, SENTINEL, dtype=np.uint32)
        h2d(self.base, g)
        h2d(self.ptr + rows * row_bytes, g)

    def fill(self, value_rows):
        """Fill every payload row with one row pattern (e.g. NaN)."""
        step = _slice_rows(self.row_bytes)
        for r0 in range(0, self.rows, step):
            cnt = min(step, self.rows - r0)
            h2d(self.ptr + r0 * self.row_bytes, np.broadcast_to(value_rows, (cnt,) + value_rows.shape[-1:]))

    def upload(self, x, r0=0):
        h2d(self.ptr + r0 * self.row_bytes, x)

    def rows_at(self, r0, cnt, dtype, width):
        return d2h(self.ptr + r0 * self.row_bytes, (cnt, width), dtype)

    def guards_intact(self):
        w = self.guard_bytes // 4
        a = d2h(self.base, (w,), np.uint32)
        b = d2h(self.ptr + self.rows * self.row_bytes, (w,), np.uint32)
        return bool(np.all(a == SENTINEL) and np.all(b == SENTINEL))

    def free(self):
        memory().free(self.handle)


def upload_rows(g, x):
    step = _slice_rows(g.row_bytes)
    for r0 in range(0, x.shape[0], step):
        g.upload(x[r0:r0 + step], r0)


def input_unchanged(g, x):
    """True if the device rows still hold x byte for byte (compared in slices)."""
    step = _slice_rows(g.row_bytes)
    for r0 in range(0, x.shape[0], step):
        xs = x[r0:r0 + step]
        if not np.array_equal(g.rows_at(r0, xs.shape[0], x.dtype, x.shape[1]).view(np.uint8), np.ascontiguousarray(xs).view(np.uint8)):
            return False
    return True


def check_device_rows(g, x, direction, family, out_dtype=None, out_width=None, m=None, label="", ref=None, long_rows=0, kind=None):
    """Download the result rows of g in slices and check every one against the reference of the matching rows of x."""
    dt = np.dtype(out_dtype or x.dtype)
    width = out_width or x.shape[1]
    step = max(1, min(_slice_rows(16 * width), _slice_rows(16 * x.shape[1])))
    es = []
    for r0 in range(0, g.rows, step):
        cnt = min(step, g.rows - r0)
        y = g.rows_at(r0, cnt, dt, width)
        es.append(check_rows(y, x[r0:r0 + cnt], direction, family, dt, n=max(width, x.shape[1]), m=m, label=label, ref=ref, b0=r0,
                             long_rows=long_rows if r0 == 0 else 0, kind=kind))
    return np.concatenate(es)


def same_bits(ga, gb, dtype, width):
    step = _slice_rows(ga.row_bytes)
    for r0 in range(0, ga.rows, step):
        cnt = min(step, ga.rows - r0)
        a = ga.rows_at(r0, cnt, dtype, width)
        b = gb.rows_at(r0, cnt, dtype, width)
        if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            diff = np.flatnonzero(np.any(a.view(np.uint8).reshape(cnt, -1) != b.view(np.uint8).reshape(cnt, -1), axis=1))
            return r0 + int(diff[0])
    return None


def check_execute_streamed(plan, n, batch, dtype, seed, family, direction=None, inplace=True, label="", expect=None, long_rows=0,
                           exact=False):
    """check_execute() for batches that do not fit the host: the input rows are block_normal_rows(n, ., ., dtype, seed), and
    every transfer and check runs in slices of at most SLICE_BYTES of complex128 reference rows, so that host memory stays at a
    few slices whatever the batch.  The same checks:
      - the output is NaN-filled and sits between two guard rows, both intact afterwards;
      - the input of the out-of-place execute is unchanged;
      - every transform: e_b <= bound(family) (fp64 and long_rows > 0: the first rows also against a long-double reference);
        exact=True: also every output word equal to the input word (n = 1);
      - inplace=True: the in-place result (guarded too) bit-identical to the out-of-place one;
      - expect() after each sync.
    Returns the largest e_b of the out-of-place run."""
    direction = plan.direction if direction is None else direction
    dt = np.dtype(dtype)
    rb = n * dt.itemsize
    step = _slice_rows(16 * n)  # rows per slice: complex128 reference rows of at most SLICE_BYTES

    def rows(r0, cnt):
        return block_normal_rows(n, r0, cnt, dt, seed)

    def upload(g):
        for r0 in range(0, batch, step):
            g.upload(rows(r0, min(step, batch - r0)), r0)

    gin, gout = Guarded(batch, rb), Guarded(batch, rb)
    gip = None
    try:
        upload(gin)
        gout.fill(np.full(n, np.nan, dtype=dt))
        plan.execute_ptr(gin.ptr, gout.ptr)
        assert plan.sync() == 0, label
        if expect:
            expect()
        assert gout.guards_intact(), "%s: out-of-place execute wrote outside [out, out + batch * n)" % label
        assert gin.guards_intact(), "%s: out-of-place execute wrote next to its input" % label
        worst = 0.0
        for r0 in range(0, batch, step):
            cnt = min(step, batch - r0)
            x = rows(r0, cnt)
            xd = gin.rows_at(r0, cnt, dt, n)
            if not np.array_equal(xd.view(np.uint8), x.view(np.uint8)):
                bad = int(np.flatnonzero(np.any(xd.view(np.uint8).reshape(cnt, -1) != x.view(np.uint8).reshape(cnt, -1), axis=1))[0])
                raise AssertionError("%s: out-of-place execute changed its input (transform %d)" % (label, r0 + bad))
            del xd
            y = gout.rows_at(r0, cnt, dt, n)
            if exact and not np.array_equal(y.view(np.uint8), x.view(np.uint8)):
                bad = int(np.flatnonzero(np.any(y.view(np.uint8).reshape(cnt, -1) != x.view(np.uint8).reshape(cnt, -1), axis=1))[0])
                raise AssertionError("%s: output differs from the input at transform %d" % (label, r0 + bad))
            e = check_rows(y, x, direction, family, dt, n=n, label=label + " out-of-place", b0=r0, long_rows=long_rows if r0 == 0 else 0)
            worst = max(worst, float(np.max(e)))
            del x, y
        gin.free()
        gin = None
        if inplace:
            gip = Guarded(batch, rb)
            upload(gip)
            plan.execute_ptr(gip.ptr, gip.ptr)
            assert plan.sync() == 0, label
            if expect:
                expect()
            assert gip.guards_intact(), "%s: in-place execute wrote outside [buf, buf + batch * n)" % label
            b = same_bits(gip, gout, dt, n)
            assert b is None, "%s: in-place result differs from the out-of-place one at transform %d" % (label, b)
        return worst
    finally:
        for g in (gin, gout, gip):
            if g is not None:
                g.free()


def check_execute(plan, x, family, direction=None, inplace=True, m=None, label="", expect=None, long_rows=0, ref=None, kind=None):
    """Run the batch x through plan (raw-pointer execute, out of place into a guarded NaN-filled output) and check
      - every transform: e_b <= bound(family) (fp64 and long_rows > 0: the first rows also against a long-double reference),
      - the input bytes are unchanged,
      - both guard rows still hold the sentinel;
    inplace=True: also in place (guarded too), bit-identical to the out-of-place result.
    expect: a callable run after each sync (asserts on plan.team_status() / plan.info()); ref: the reference of a row batch
    (default: the 1D transform of every row); kind: see check_rows().  Returns e of the out-of-place run."""
    direction = plan.direction if direction is None else direction
    batch, n = x.shape
    rb = n * x.dtype.itemsize
    nan_row = np.full(n, np.nan, dtype=x.dtype)
    gin, gout = Guarded(batch, rb), Guarded(batch, rb)
    gip = None
    try:
        upload_rows(gin, x)
        gout.fill(nan_row)
        plan.execute_ptr(gin.ptr, gout.ptr)
        assert plan.sync() == 0, label
        if expect:
            expect()
        assert gout.guards_intact(), "%s: out-of-place execute wrote outside [out, out + batch * n)" % label
        assert gin.guards_intact(), "%s: out-of-place execute wrote next to its input" % label
        assert input_unchanged(gin, x), "%s: out-of-place execute changed its input" % label
        e = check_device_rows(gout, x, direction, family, m=m, label=label + " out-of-place", ref=ref, long_rows=long_rows, kind=kind)
        gin.free()
        gin = None
        if inplace:
            gip = Guarded(batch, rb)
            upload_rows(gip, x)
            plan.execute_ptr(gip.ptr, gip.ptr)
            assert plan.sync() == 0, label
            if expect:
                expect()
            assert gip.guards_intact(), "%s: in-place execute wrote outside [buf, buf + batch * n)" % label
            b = same_bits(gip, gout, x.dtype, n)
            assert b is None, "%s: in-place result differs from the out-of-place one at transform %d" % (label, b)
        return e
    finally:
        for g in (gin, gout, gip):
            if g is not None:
                g.free()


def _flat_rows(ptr, r0, cnt, dtype, width):
    """Rows r0 .. r0 + cnt - 1 of a packed [rows][width] array of dtype that starts at ptr."""
    return d2h(ptr + r0 * width * np.dtype(dtype).itemsize, (cnt, width), dtype)


def check_execute_io(run, x, w_out, dtype_out, family, ref, x2=None, n=None, m=None, scale="rms", inplace=False, label="",
                     expect=None, expected=None, kind=None):
    """check_execute() for executes whose input and output rows differ in width or type (2D, r2c, c2r, fused consumers).
      x: input rows [batch][w_in]; x2: optional second input of the same shape (cross-correlation's y);
      run(in_ptr, in2_ptr, out_ptr): enqueue the execute and wait for it (in2_ptr is None without x2);
      ref(xs) -- ref(xs, x2s) with a second input -- the float64 reference [rows][w_out] of a slice of input rows;
      expected: the whole reference [batch][w_out], computed once by the caller (several variants of one plan), instead of ref;
      n / m: the length the bound K u log2(.) is taken at (default: the wider of the two rows); scale: see row_errors().
    Inputs and output each live in a Guarded of their own row size (guards a multiple of 16 bytes, so every payload starts where
    a plain allocation's would: 16-byte aligned, its rows packed).  Checked:
      - the NaN-filled output: every row's e_b <= bound(family), so no row keeps a NaN;
      - the guards of the output and of every input still hold the sentinel; the inputs are unchanged byte for byte;
      - inplace=True: the same execute with in_ptr == out_ptr on ONE buffer of batch * max(input row, output row) bytes, the
        input rows packed at its start (as r2c / c2r in place need it; equal rows: plainly in place): guards intact, result
        bit-identical to the out-of-place one;
      - expect() after every run.
    Returns e of the out-of-place run."""
    x = np.ascontiguousarray(x)
    batch, w_in = x.shape
    dt_out = np.dtype(dtype_out)
    rb_in, rb_out = w_in * x.dtype.itemsize, w_out * dt_out.itemsize
    n = n or max(w_in, w_out)
    if x2 is not None:
        x2 = np.ascontiguousarray(x2)
        assert x2.shape == x.shape and x2.dtype == x.dtype
    if expected is not None:
        assert expected.shape == (batch, w_out)
        xx, ref_rows = expected, (lambda r: r)
    elif x2 is not None:
        xx = np.concatenate([x, x2], axis=1)  # one array of input rows for the sliced reference
        ref_rows = lambda r: ref(r[:, :w_in], r[:, w_in:])
    else:
        xx, ref_rows = x, ref
    nan_row = np.full(w_out, np.nan, dtype=dt_out)
    gin, gout = Guarded(batch, rb_in, align16=True), Guarded(batch, rb_out, align16=True)
    gin2 = Guarded(batch, rb_in, align16=True) if x2 is not None else None
    gip = None
    try:
        upload_rows(gin, x)
        if gin2:
            upload_rows(gin2, x2)
        gout.fill(nan_row)
        run(gin.ptr, gin2.ptr if gin2 else None, gout.ptr)
        if expect:
            expect()
        assert gout.guards_intact(), "%s: out-of-place execute wrote outside [out, out + batch * %d)" % (label, w_out)
        assert gin.guards_intact(), "%s: out-of-place execute wrote next to its input" % label
        assert input_unchanged(gin, x), "%s: out-of-place execute changed its input" % label
        if gin2:
            assert gin2.guards_intact(), "%s: out-of-place execute wrote next to its second input" % label
            assert input_unchanged(gin2, x2), "%s: out-of-place execute changed its second input" % label
        step = max(1, _slice_rows(16 * max(w_out, xx.shape[1])))
        es = []
        for r0 in range(0, batch, step):
            cnt = min(step, batch - r0)
            y = gout.rows_at(r0, cnt, dt_out, w_out)
            es.append(check_rows(y, xx[r0:r0 + cnt], 0, family, dt_out, n=n, m=m, label=label + " out-of-place", ref=ref_rows, b0=r0,
                                 scale=scale, kind=kind))
        e = np.concatenate(es)
        gin.free()
        gin = None
        if inplace:
            assert x2 is None
            rb = max(rb_in, rb_out)
            gip = Guarded(batch, rb, align16=True)
            gip.fill(np.frombuffer(np.full(rb // 4, np.nan, dtype=np.float32).tobytes(), dtype=np.uint8))
            h2d(gip.ptr, x)  # input rows packed at the start of the buffer
            run(gip.ptr, None, gip.ptr)
            if expect:
                expect()
            assert gip.guards_intact(), "%s: in-place execute wrote outside its buffer" % label
            for r0 in range(0, batch, step):
                cnt = min(step, batch - r0)
                a = _flat_rows(gip.ptr, r0, cnt, dt_out, w_out)
                b = gout.rows_at(r0, cnt, dt_out, w_out)
                if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
                    diff = np.flatnonzero(np.any(a.view(np.uint8).reshape(cnt, -1) != b.view(np.uint8).reshape(cnt, -1), axis=1))
                    raise AssertionError("%s: in-place result differs from the out-of-place one at row %d" % (label, r0 + int(diff[0])))
        return e
    finally:
        for g in (gin, gin2, gout, gip):
            if g is not None:
                g.free()


# ---------------------------------------------------------------------------------------------------------------------------
# exact conditions on a linear operator: neighbours of a poisoned transform, power-of-two scaling, zeros
# ---------------------------------------------------------------------------------------------------------------------------
POISONS = ("nan", "inf0", "huge")
# "huge": every sample 2^120 / 2^1000, finite.  A transform's bin 0 is n times that and overflows only from n = 256 in fp32 (never in
# fp64 at the sizes used); the quadratic consumers (autocorr, xcorr, psd, conv products) overflow at every n.  Below that the row is
# a finite value 2^100 and more above its neighbours', which a lane that adds or multiplies where it should select cannot absorb.
HUGE_EXP = {np.dtype(np.float32): 120, np.dtype(np.float64): 1000}
SCALE_EXP = {np.dtype(np.float32): 20, np.dtype(np.float64): 200}   # check_scaling: s = +-20 in fp32, +-200 in fp64


def poisoned(x, rows, poison):
    """A copy of x whose `rows` are poisoned: "nan" every sample NaN; "inf0" the real part of sample 0 +Inf, the rest untouched;
    "huge" every sample 2^120 (fp32) / 2^1000 (fp64)."""
    x = np.array(x, copy=True, order="C")
    v = x.view(x.real.dtype).reshape(x.shape[0], -1)
    rows = np.asarray(sorted(rows), dtype=np.int64)
    if poison == "nan":
        v[rows] = np.nan
    elif poison == "inf0":
        v[rows, 0] = np.inf
    elif poison == "huge":
        v[rows] = np.ldexp(1.0, HUGE_EXP[v.dtype])
    else:
        raise ValueError("poison: one of %s" % (POISONS,))
    return x


class _Runs:
    """Repeated runs of run(in_ptr, in2_ptr, out_ptr) on ONE set of guarded buffers: every call uploads its inputs, NaN-fills the
    output, runs, and checks the guards and the untouched inputs.  Returns the result rows [rows_out][w_out]."""

    def __init__(self, run, x, w_out, dtype_out, rows_out, x2, label):
        self.run, self.label = run, label
        self.w_out, self.dt_out, self.rows_out = w_out, np.dtype(dtype_out), rows_out
        self.gin = Guarded(x.shape[0], x.shape[1] * x.dtype.itemsize, align16=True)
        self.gin2 = Guarded(x2.shape[0], x2.shape[1] * x2.dtype.itemsize, align16=True) if x2 is not None else None
        self.gout = Guarded(rows_out, w_out * self.dt_out.itemsize, align16=True)

    def __call__(self, x, x2=None):
        upload_rows(self.gin, np.ascontiguousarray(x))
        if self.gin2:
            upload_rows(self.gin2, np.ascontiguousarray(x2))
        self.gout.fill(np.full(self.w_out, np.nan, dtype=self.dt_out))
        self.run(self.gin.ptr, self.gin2.ptr if self.gin2 else None, self.gout.ptr)
        assert self.gout.guards_intact(), "%s: the execute wrote outside its output" % self.label
        assert self.gin.guards_intact(), "%s: the execute wrote next to its input" % self.label
        assert input_unchanged(self.gin, x), "%s: the execute changed its input" % self.label
        if self.gin2:
            assert self.gin2.guards_intact(), "%s: the execute wrote next to its second input" % self.label
            assert input_unchanged(self.gin2, x2), "%s: the execute changed its second input" % self.label
        return self.gout.rows_at(0, self.rows_out, self.dt_out, self.w_out)

    def free(self):
        for g in (self.gin, self.gin2, self.gout):
            if g is not None:
                g.free()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


def _differing_rows(a, b):
    return np.flatnonzero(np.any(_bits(a) != _bits(b), axis=1))


def check_neighbours(run, x, poison_rows, poison, w_out=None, dtype_out=None, x2=None, poison_second=False, out_rows=None,
                     rows_out=None, label=""):
    """A poisoned transform leaves its neighbours bit-identical.
      run(in_ptr, in2_ptr, out_ptr): one execute of ONE plan, finished when it returns (as check_execute_io's);
      x [batch][w_in] (x2: a second input of the same shape); poison_rows: the input rows replaced by `poison` (see poisoned())
      in x -- poison_second=True: in x2 instead -- for the second run, on the same buffers;
      w_out / dtype_out / rows_out: the result rows (default: as the input); out_rows(b): the result rows input row b feeds
      (default: row b alone; a frames plan: the frames of signal b).
    Every result row no poisoned input row feeds must equal the first run's bit for bit; under the "nan" poison every bin of every
    fed row must be non-finite; guards intact, inputs unchanged.  Bit identity is a condition, not a tolerance: the same plan at
    the same position sees the same data in every untouched row.  Returns (first result, second result)."""
    x = np.ascontiguousarray(x)
    w_out, dtype_out = w_out or x.shape[1], np.dtype(dtype_out or x.dtype)
    rows_out = rows_out or x.shape[0]
    out_rows = out_rows or (lambda b: (b,))
    label = "%s poison=%s rows %s" % (label, poison, sorted(poison_rows))
    r = _Runs(run, x, w_out, dtype_out, rows_out, x2, label)
    try:
        y0 = r(x, x2)
        assert np.all(np.isfinite(y0)), "%s: the unpoisoned run is not finite" % label
        if poison_second:
            y1 = r(x, poisoned(x2, poison_rows, poison))
        else:
            y1 = r(poisoned(x, poison_rows, poison), x2)
    finally:
        r.free()
    fed = np.zeros(rows_out, dtype=bool)
    for b in poison_rows:
        fed[list(out_rows(b))] = True
    bad = [int(i) for i in _differing_rows(y0, y1) if not fed[i]]
    if bad:
        i = bad[0]
        k = int(np.flatnonzero(np.any(_bits(y0[i].reshape(w_out, 1)) != _bits(y1[i].reshape(w_out, 1)), axis=1))[0])
        raise AccuracyError("%s: %d untouched result rows changed with their neighbour: rows %s%s; row %d bin %d was %r, is %r"
                            % (label, len(bad), bad[:12], " ..." if len(bad) > 12 else "", i, k, y0[i, k], y1[i, k]))
    if poison == "nan":
        clean = np.flatnonzero(fed & np.any(np.isfinite(y1), axis=1))
        if clean.size:
            i = int(clean[0])
            raise AccuracyError("%s: result row %d of an all-NaN transform has %d finite bins (first: bin %d)"
                                % (label, i, int(np.sum(np.isfinite(y1[i]))), int(np.flatnonzero(np.isfinite(y1[i]))[0])))
    return y0, y1


def check_scaling(run, x, degree=1, w_out=None, dtype_out=None, x2=None, rows_out=None, label=""):
    """execute(2^s x) == 2^(s * degree) execute(x) bit for bit, s = +-SCALE_EXP (20 in fp32, 200 in fp64); degree 2: results
    quadratic in x (autocorrelation, power).  x2 is not scaled.  The data path is mul / add / fma only, so a power of two commutes
    with every rounding as long as nothing leaves the normal range; a hidden absolute threshold or a lossy intermediate breaks it."""
    x = np.ascontiguousarray(x)
    w_out, dtype_out = w_out or x.shape[1], np.dtype(dtype_out or x.dtype)
    rows_out = rows_out or x.shape[0]
    s = SCALE_EXP[np.dtype(x.real.dtype)]
    r = _Runs(run, x, w_out, dtype_out, rows_out, x2, label)
    try:
        y0 = r(x, x2)
        assert np.all(np.isfinite(y0)), "%s: the unscaled run is not finite" % label
        for e in (s, -s):
            xs = np.ldexp(x.view(x.real.dtype), e).view(x.dtype)
            want = np.ldexp(y0.view(y0.real.dtype), e * degree).view(y0.dtype)
            tiny = np.finfo(y0.real.dtype).tiny
            v = np.abs(want.view(y0.real.dtype))
            assert np.all((v == 0) | (v >= tiny)) and np.all(np.isfinite(v)), "%s: the scaled result leaves the normal range" % label
            y1 = r(xs, x2)
            bad = _differing_rows(want, y1)
            if bad.size:
                i = int(bad[0])
                k = int(np.flatnonzero(want[i] != y1[i])[0]) if np.any(want[i] != y1[i]) else 0
                raise AccuracyError("%s: execute(2^%d x) differs from 2^%d execute(x) in %d rows: %s; row %d bin %d: %r, expected %r"
                                    % (label, e, e * degree, bad.size, [int(b) for b in bad[:12]], i, k, y1[i, k], want[i, k]))
    finally:
        r.free()
    return y0


def check_zeros(run, x, w_out=None, dtype_out=None, x2=None, rows_out=None, label=""):
    """An all-zero batch (of the shape of x, and of x2) returns zeros of either sign and no NaN."""
    x = np.ascontiguousarray(x)
    w_out, dtype_out = w_out or x.shape[1], np.dtype(dtype_out or x.dtype)
    rows_out = rows_out or x.shape[0]
    r = _Runs(run, x, w_out, dtype_out, rows_out, x2, label)
    try:
        y = r(np.zeros_like(x), None if x2 is None else np.zeros_like(x2))
    finally:
        r.free()
    bad = np.flatnonzero(np.any(~(y == 0), axis=1))
    if bad.size:
        i = int(bad[0])
        k = int(np.flatnonzero(~(y[i] == 0))[0])
        raise AccuracyError("%s: zeros in, but %d result rows are not zero: %s; row %d bin %d = %r"
                            % (label, bad.size, [int(b) for b in bad[:12]], i, k, y[i, k]))
