"""The cases at which the frames plans on REAL signals (csrc/fft_plans_ext.h FramesPlan with real_input: one-sided STFT, spectrogram,
Welch) are checked frame by frame against float64, on the GPU (tests/test_gpu_rframes.py) and in the CPU emulation
(tests/test_emulated_rframes.py), with the inputs, the float64 reference and the checker both files share.  Test infrastructure only.

Every shape is the smallest that reaches its hazard.  The reference is numpy: the frames are an as_strided view of the float64 copy of
the input (cast BEFORE the transform: numpy >= 2 transforms in the input's precision), then the window (frames_ladder.window_values),
np.fft.rfft and
    power[k] = |X[k]|^2 / (fs * P), doubled for 0 < k < n/2, k <= n/2;   P = 0.375 n (Hann) or sum w^2;   Welch = mean over the frames.

Bounds: K u log2(n) per row, n the frame length, K = 8 for every output kind, the frames ladder's bound: the transform is that ladder's
single- or multi-pass schedule at half the length, plus the split's three roundings per bin.  STFT rows in units of the row's RMS,
power and Welch rows in units of max(RMS, |bin|).  Worst e / (u log2 n) measured over this ladder (profiles/rframes_accuracy_report.json):
                 STFT fp32 / fp64     POWER fp32 / fp64    WELCH fp32 / fp64
    MI355X       1.19 / 1.87          1.52 / 3.06          1.09 / 2.14
    emulation    1.13 / 1.87          1.54 / 3.06          1.16 / 2.14
(the fp64 worsts are at n = 4, where log2 n = 2 leaves the unit small; the fp32 ones at n = 64.)
All are <= 4, so K stays 8 (tests/accuracy.py's rule: K at least twice the worst measured value).
"""
import numpy as np
from numpy.lib.stride_tricks import as_strided

import accuracy as A
import frames_ladder as L
from frames_ladder import BLACKMAN, HAMMING, HANN, POWER, RECT, STFT, USER, WELCH, Case, KIND_NAMES, WINDOW_NAMES  # noqa: F401

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BOTH = (F32, F64)
BOUND_K = {STFT: 8, POWER: 8, WELCH: 8}
FAMILY = {STFT: "rframes_stft", POWER: "rframes_power", WELCH: "rframes_welch"}  # keys of the FFT_ACCURACY_REPORT file
FS = L.FS


def complex_dtype(dtype):
    return L.C64 if np.dtype(dtype) == F32 else L.C128


# the shapes both the device and the emulation run (n = 64: a half-length core of 32, tiles of 64 (fp32) / 32 (fp64) frames)
SMALL = [
    Case("a", 64, 16, 30, 5, why="150 frames: tiles straddle signals, the last tile is ragged"),
    Case("b-hop18", 64, 18, 30, 5, why="frames start 8-byte but not 16-byte aligned in fp32"),
    Case("b-hop15", 64, 15, 30, 5, why="odd hop: frames start at odd reals, component loads"),
    Case("c-pad1", 64, 16, 30, 5, pad=1, why="odd signal starts: in_vec_ok must be 0"),
    Case("c-pad2", 64, 16, 30, 5, pad=2, why="signal starts 8 bytes off a 16-byte boundary in fp32: in_vec_ok must be 0 there"),
    Case("d-nooverlap", 64, 64, 3, 5, why="hop = n"),
    Case("d-hop1", 64, 1, 3, 3, why="hop = 1"),
    Case("d-oneframe", 64, 16, 37, 1, why="one frame per signal, 37 signals: the quotient by frames_per_signal = 1"),
    Case("e", 64, 16, 5, 4, tail=15, why="signal_len = n + 3 hop + (hop - 1): a NaN tail no frame may read"),
    Case("h-rect", 256, 64, 2, 3, window=RECT, why="window kind"),
    Case("h-hann", 256, 64, 2, 3, window=HANN, why="window kind"),
    Case("h-hamming", 256, 64, 2, 3, window=HAMMING, why="window kind"),
    Case("h-blackman", 256, 64, 2, 3, window=BLACKMAN, why="window kind"),
    Case("h-user", 256, 64, 2, 3, window=USER, why="a random, asymmetric window: a swapped or complex-multiplied pair of window values fails"),
    Case("n4", 4, 2, 3, 5, why="n = 4: L = 2, the smallest"),
    Case("j", 64, 16, 3, 37, kinds=(WELCH,), why="the mean kernel over an odd frame count"),
]
CASE_A = SMALL[0]
OFFSET_CASE = Case("a-offset1", 64, 16, 30, 5, why="the input starts one real behind a 16-byte boundary")
IMPULSES = Case("impulses", 64, 64, 1, 64, window=RECT, kinds=(STFT,), why="frame w = a unit impulse at sample w: X[k] = W_n^(w k)")
# on the device: the largest frames of the one-launch path, and the fallback
GPU_F = [Case("f-fp32", 8192, 4096, 3, 5, dtypes=(F32,), why="the largest fused frame, fp32"),
         Case("f-fp64", 4096, 2048, 3, 5, dtypes=(F64,), why="the largest fused frame, fp64")]
GPU_G = [Case("g", 16384, 8192, 3, 3, why="the fallback: pack, multi-pass core, split")]
# in the emulation: the same at n = 512, and the fallback under an LDS budget that gives the half-length core two passes (n = 512:
# a core of 256 under 4096 bytes) and three (n = 8192: a core of 4096 under 4096 bytes) -- the cores of frames_ladder.EMU_G
EMU_F = [Case("f", 512, 256, 3, 5, why="the one-launch path at n = 512")]
EMU_G = [(Case("g-2pass", 512, 256, 3, 3, why="fallback, two passes"), 4096, 2),
         (Case("g-3pass", 8192, 4096, 3, 3, why="fallback, three passes"), 4096, 3)]


def user_window(case, dtype):
    """The n values handed to the plan for a USER window (None otherwise), in the plan's precision."""
    return np.ascontiguousarray(L.window_values(USER, case.n).astype(np.dtype(dtype))) if case.window == USER else None


def make_input(case, dtype, seed=7):
    """[n_signals][signal_pitch] real normal values; every sample no frame covers -- the tail of each signal and the
    signal_pitch - signal_len padding -- is NaN, so a frame that reads one fails its row."""
    x = np.random.default_rng((seed, case.n, case.hop)).standard_normal((case.n_signals, case.pitch)).astype(np.dtype(dtype))
    covered = (case.nw - 1) * case.hop + case.n
    x[:, covered:] = np.nan
    return x


def impulse_input(case, dtype):
    """IMPULSES: frame w of the one signal is a unit impulse at its sample w; the rows expected of it, X[w][k] = exp(-2 pi i w k / n)."""
    n = case.n
    x = np.zeros((1, case.pitch), dtype=np.dtype(dtype))
    w = np.arange(case.nw)
    x[0, w * case.hop + w] = 1.0
    X = np.exp(-2j * np.pi * (np.outer(w, np.arange(n // 2 + 1)) % n) / n)  # (w k mod n: the argument stays below 2 pi, its rounding below u)
    return x, X


def reference(case, x, kind, dtype, fs=FS):
    """The float64 result rows: STFT [S * nw][n/2 + 1] complex128, POWER [S * nw][n/2 + 1], WELCH [S][n/2 + 1] float64."""
    n, nw, S = case.n, case.nw, case.n_signals
    xs = np.ascontiguousarray(x.astype(np.float64))
    fr = as_strided(xs, shape=(S, nw, n), strides=(case.pitch * 8, case.hop * 8, 8), writeable=False)
    w = user_window(case, dtype).astype(np.float64) if case.window == USER else L.window_values(case.window, n)
    X = np.fft.rfft(fr * w, axis=-1)
    if kind == STFT:
        return X.reshape(S * nw, n // 2 + 1)
    P = 0.375 * n if case.window == HANN else float(np.sum(w * w))
    p = np.abs(X) ** 2 / (fs * P)
    p[:, :, 1:n // 2] *= 2.0
    if kind == POWER:
        return p.reshape(S * nw, n // 2 + 1)
    return p.mean(axis=1)


def out_shape(case, kind, dtype):
    """(rows, width, dtype) of the result."""
    if kind == STFT:
        return case.n_signals * case.nw, case.n // 2 + 1, complex_dtype(dtype)
    if kind == POWER:
        return case.n_signals * case.nw, case.n // 2 + 1, np.dtype(dtype)
    return case.n_signals, case.n // 2 + 1, np.dtype(dtype)


def bound(kind, dtype, n):
    return BOUND_K[kind] * A.U[np.dtype(dtype)] * max(1.0, np.log2(n))


def vec_loads_allowed(case, dtype, offset=0):
    """The issue's alignment rule: 16-byte loads only where EVERY frame starts 16-byte aligned -- the base, and hop and signal_pitch
    multiples of 16 / sizeof(real)."""
    q = 16 // np.dtype(dtype).itemsize
    return offset % q == 0 and case.hop % q == 0 and case.pitch % q == 0


def check(run, case, kind, dtype, x=None, expected=None, label="", fs=FS, report=True, offset=0):
    """run(x_ptr, signal_pitch, out_ptr): one execute of a real frames plan of `kind` for `case`, finished when it returns.
    The input lives in a Guarded of its own, `offset` reals (a NaN each) behind its 16-byte aligned start; the output is NaN-filled
    between guards.  Checked: every row within bound(kind) (the STFT in units of the row's RMS, power and Welch rows in units of
    max(RMS, |bin|)) -- so no row keeps a NaN and no frame has read a NaN sample; DC and Nyquist bins of STFT rows have an imaginary
    part == 0.0; the guards of input and output; the input byte for byte; a second execute of the same plan bit-identical to the
    first.  Prints e / (u log2 n) before it asserts.  Returns the result rows."""
    dt = np.dtype(dtype)
    x = make_input(case, dt) if x is None else x
    X = reference(case, x, kind, dt, fs) if expected is None else expected
    rows, width, odt = out_shape(case, kind, dt)
    assert X.shape == (rows, width)
    label = label or "%s %s %s" % (case, KIND_NAMES[kind], "fp32" if dt == F32 else "fp64")
    flat = np.concatenate([np.full(offset, np.nan, dtype=dt), x.reshape(-1)]).reshape(1, -1)
    gin = A.Guarded(1, flat.nbytes, align16=True)
    outs = [A.Guarded(rows, width * odt.itemsize, align16=True) for _ in range(2)]
    try:
        A.upload_rows(gin, flat)
        for g in outs:
            g.fill(np.full(width, np.nan, dtype=odt))
            run(gin.ptr + offset * dt.itemsize, case.pitch, g.ptr)
            assert g.guards_intact(), "%s: the execute wrote outside its output" % label
        assert gin.guards_intact(), "%s: the execute wrote next to its input" % label
        assert A.input_unchanged(gin, flat), "%s: the execute changed its input" % label
        y = outs[0].rows_at(0, rows, odt, width)
        e, k = A.row_errors(y, X, scale="rms" if kind == STFT else "rms_or_bin")
        unit = A.U[dt] * max(1.0, np.log2(case.n))
        print("%s: worst e / (u log2 n) = %.3f (row %d, bin %d)" % (label, float(np.max(e)) / unit, int(np.argmax(e)), int(k[int(np.argmax(e))])))
        if report:
            A._note(FAMILY[kind], dt, case.n, None, e)
        A.assert_within(e, k, bound(kind, dt, case.n), label)
        if kind == STFT:
            assert np.all(y[:, 0].imag == 0.0) and np.all(y[:, -1].imag == 0.0), "%s: a DC or Nyquist bin with an imaginary part" % label
        b = A.same_bits(outs[0], outs[1], odt, width)
        assert b is None, "%s: two executes of one plan differ at row %d" % (label, b)
        return y
    finally:
        gin.free()
        for g in outs:
            g.free()


def check_consistency(run_real, run_complex, case, kind, dtype):
    """The real plan's rows against bins 0 ... n/2 of the complex frames plan fed the same signal with a zero imaginary part
    (power and Welch rows: the same rows); the tolerance is the sum of the two plans' bounds.
    run_*(x_ptr, signal_pitch, out_ptr) as in check()."""
    dt = np.dtype(dtype)
    cdt = complex_dtype(dt)
    x = make_input(case, dt)
    rows, width, odt = out_shape(case, kind, dt)
    crows, cwidth, codt = L.out_shape(case, kind, cdt)
    gr, gc = A.Guarded(case.n_signals, case.pitch * dt.itemsize, align16=True), A.Guarded(case.n_signals, case.pitch * cdt.itemsize, align16=True)
    yr, yc = A.Guarded(rows, width * odt.itemsize, align16=True), A.Guarded(crows, cwidth * codt.itemsize, align16=True)
    try:
        A.upload_rows(gr, x)
        A.upload_rows(gc, x.astype(cdt))
        run_real(gr.ptr, case.pitch, yr.ptr)
        run_complex(gc.ptr, case.pitch, yc.ptr)
        a = yr.rows_at(0, rows, odt, width)
        b = yc.rows_at(0, crows, codt, cwidth)[:, :width]
        e, k = A.row_errors(a, b.astype(np.complex128 if kind == STFT else np.float64), scale="rms" if kind == STFT else "rms_or_bin")
        A.assert_within(e, k, bound(kind, dt, case.n) + L.bound(kind, cdt, case.n), "real vs complex frames plan, %s %s" % (case, KIND_NAMES[kind]))
    finally:
        for g in (gr, gc, yr, yc):
            g.free()
