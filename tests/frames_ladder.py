"""The cases at which the plans on overlapping frames (csrc/fft_plans_ext.h FramesPlan: STFT, spectrogram, Welch) are checked frame
by frame against float64, on the GPU (tests/test_gpu_frames.py) and in the CPU emulation (tests/test_emulated_frames.py), with the
inputs, the float64 reference and the checker both files share.  Test infrastructure only.

Every shape is the smallest that reaches its hazard.  The reference is numpy: the frames are an as_strided view of the complex128
copy of the input, then the window (the reference project's formulas with their n - 1 denominators), np.fft.fft and
    power[k] = |X[k]|^2 / (fs * P), doubled for 0 < k < n/2, k <= n/2;   P = 0.375 n (Hann) or sum w^2;   Welch = mean over the frames.

Bounds: K u log2(n) per frame, K = 8 for every output kind -- accuracy.BOUND_K's "multipass" K for the STFT (the transform is the
same single- or multi-pass schedule) and its "psd" K for power and Welch rows (a Welch row averages power rows: its error is at
most theirs).  The table below is this ladder's own.
"""
import ctypes as C

import numpy as np
from numpy.lib.stride_tricks import as_strided

import accuracy as A

C64, C128 = np.dtype(np.complex64), np.dtype(np.complex128)
BOTH = (C64, C128)
RECT, HANN, HAMMING, BLACKMAN, USER = range(5)
WINDOW_NAMES = {RECT: "rect", HANN: "hann", HAMMING: "hamming", BLACKMAN: "blackman", USER: "user"}
STFT, POWER, WELCH = range(3)
KIND_NAMES = {STFT: "stft", POWER: "power", WELCH: "welch"}
BOUND_K = {STFT: 8, POWER: 8, WELCH: 8}
FAMILY = {STFT: "frames_stft", POWER: "frames_power", WELCH: "frames_welch"}  # keys of the FFT_ACCURACY_REPORT file
FS = 48000.0


class Case:
    """n, hop, n_signals, nw frames per signal; tail: samples behind the last frame of every signal (< hop, so nw stands);
    pad: signal_pitch - signal_len; window; kinds: the output kinds the case runs."""

    def __init__(self, name, n, hop, n_signals, nw, tail=0, pad=0, window=HANN, kinds=(STFT, POWER, WELCH), dtypes=BOTH, why=""):
        assert 0 <= tail < hop
        self.name, self.n, self.hop, self.n_signals, self.nw, self.tail, self.pad = name, n, hop, n_signals, nw, tail, pad
        self.window, self.kinds, self.dtypes, self.why = window, kinds, dtypes, why
        self.signal_len = n + (nw - 1) * hop + tail
        self.pitch = self.signal_len + pad

    def __repr__(self):
        return self.name


# (a) - (e), (h), (j): the shapes both the device and the emulation run
SMALL = [
    Case("a", 64, 16, 30, 5, why="150 frames: tiles of 64 (fp32) / 32 (fp64) frames straddle signals, the last tile is ragged"),
    Case("b", 64, 15, 30, 5, why="odd hop: frame starts are not 16-byte aligned in fp32, the scalar load path"),
    Case("c", 64, 16, 30, 5, pad=1, why="signal_pitch = signal_len + 1: odd signals start unaligned, in_vec_ok must be 0"),
    Case("d-nooverlap", 64, 64, 3, 5, why="hop = n"),
    Case("d-hop1", 64, 1, 3, 3, why="hop = 1"),
    Case("d-oneframe", 64, 16, 37, 1, why="one frame per signal, 37 signals: the quotient by frames_per_signal = 1"),
    Case("e", 64, 16, 5, 4, tail=15, why="signal_len = n + 3 hop + (hop - 1): a NaN tail no frame may read"),
    Case("h-rect", 256, 64, 2, 3, window=RECT, why="window kind"),
    Case("h-hann", 256, 64, 2, 3, window=HANN, why="window kind"),
    Case("h-hamming", 256, 64, 2, 3, window=HAMMING, why="window kind"),
    Case("h-blackman", 256, 64, 2, 3, window=BLACKMAN, why="window kind"),
    Case("h-user", 256, 64, 2, 3, window=USER, why="a random positive window: P = sum w^2"),
    Case("j", 64, 16, 3, 37, kinds=(WELCH,), why="the mean kernel over an odd frame count"),
]
# (f), (g) on the device
GPU_F = [Case("f-fp32", 4096, 2048, 3, 5, dtypes=(C64,), why="the largest single-pass frame, fp32"),
         Case("f-fp64", 2048, 1024, 3, 5, dtypes=(C128,), why="the largest single-pass frame, fp64")]
GPU_G = [Case("g", 8192, 4096, 3, 3, why="the multi-pass fallback")]
# ... and in the emulation: (f) at n = 256; (g) at n = 256 under an LDS budget of 4096 bytes (two passes), and with a three-pass
# core.  No budget gives n = 256 three passes (the planner keeps two passes down to 640 bytes fp32 / 896 bytes fp64 and refuses the
# plan below), so the three-pass core is n = 4096 under 4096 bytes, the shape tests/ext_ladder.py uses for its three-pass rows.
EMU_F = [Case("f", 256, 128, 3, 5, why="single pass at n = 256")]
EMU_G = [(Case("g-2pass", 256, 128, 3, 3, why="multi-pass fallback, two passes"), 4096, 2),
         (Case("g-3pass", 4096, 2048, 3, 3, why="multi-pass fallback, three passes"), 4096, 3)]
CASE_A = SMALL[0]


def window_values(kind, n, seed=5):
    """The window in float64 (the reference project's formulas, applications/power_spectrum.c:5-25 there)."""
    i = np.arange(n, dtype=np.float64)
    a = 2.0 * np.pi * i / (n - 1)
    if kind == RECT:
        return np.ones(n)
    if kind == HANN:
        return 0.5 * (1.0 - np.cos(a))
    if kind == HAMMING:
        return 0.54 - 0.46 * np.cos(a)
    if kind == BLACKMAN:
        return 0.42 - 0.5 * np.cos(a) + 0.08 * np.cos(2.0 * a)
    return np.random.default_rng(seed).uniform(0.25, 1.0, n)


def real_dtype(dtype):
    return np.dtype(np.float32) if np.dtype(dtype) == C64 else np.dtype(np.float64)


def user_window(case, dtype):
    """The n values handed to the plan for a USER window (None otherwise), in the plan's precision."""
    return np.ascontiguousarray(window_values(USER, case.n).astype(real_dtype(dtype))) if case.window == USER else None


def make_input(case, dtype, seed=7):
    """[n_signals][signal_pitch] complex normal values; every sample no frame covers -- the tail of each signal and the
    signal_pitch - signal_len padding -- is NaN, so a frame that reads one fails its row."""
    x = A.block_normal_rows(case.pitch, 0, case.n_signals, dtype, seed).copy()
    covered = (case.nw - 1) * case.hop + case.n
    x[:, covered:] = np.nan + 1j * np.nan
    return x


def reference(case, x, kind, dtype, fs=FS):
    """The float64 result rows: STFT [S * nw][n] complex128, POWER [S * nw][n/2 + 1], WELCH [S][n/2 + 1] float64."""
    n, nw, S = case.n, case.nw, case.n_signals
    xs = np.ascontiguousarray(x.astype(np.complex128))
    fr = as_strided(xs, shape=(S, nw, n), strides=(case.pitch * 16, case.hop * 16, 16), writeable=False)
    w = user_window(case, dtype).astype(np.float64) if case.window == USER else window_values(case.window, n)
    X = np.fft.fft(fr * w, axis=-1)
    if kind == STFT:
        return X.reshape(S * nw, n)
    P = 0.375 * n if case.window == HANN else float(np.sum(w * w))
    p = np.abs(X[:, :, :n // 2 + 1]) ** 2 / (fs * P)
    p[:, :, 1:n // 2] *= 2.0
    if kind == POWER:
        return p.reshape(S * nw, n // 2 + 1)
    return p.mean(axis=1)


def out_shape(case, kind, dtype):
    """(rows, width, dtype) of the result."""
    if kind == STFT:
        return case.n_signals * case.nw, case.n, np.dtype(dtype)
    if kind == POWER:
        return case.n_signals * case.nw, case.n // 2 + 1, real_dtype(dtype)
    return case.n_signals, case.n // 2 + 1, real_dtype(dtype)


def bound(kind, dtype, n):
    return BOUND_K[kind] * A.U[np.dtype(dtype)] * max(1.0, np.log2(n))


class HostMemory:
    """accuracy.MEMORY for the emulation: Guarded buffers in host memory (16-byte aligned, like a device allocation)."""

    def __init__(self):
        self.live = {}

    def alloc(self, nbytes):
        a = np.empty(nbytes + 16, dtype=np.uint8)
        ptr = a.ctypes.data + (-a.ctypes.data) % 16
        self.live[ptr] = a
        return ptr, ptr

    def free(self, handle):
        self.live.pop(handle, None)

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        C.memmove(dptr, arr.ctypes.data, arr.nbytes)

    def d2h(self, dptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        C.memmove(out.ctypes.data, dptr, out.nbytes)
        return out


def check(run, case, kind, dtype, x=None, expected=None, label="", fs=FS, report=True):
    """run(x_ptr, signal_pitch, out_ptr): one execute of a plan of `kind` for `case`, finished when it returns.
    The input lives in a Guarded of its own; the output is NaN-filled between guards.  Checked: every frame's row within
    bound(kind) (the STFT in units of the row's RMS, power and Welch rows in units of max(RMS, |bin|)) -- so no row keeps a NaN and
    no frame has read a NaN sample; the guards of input and output; the input byte for byte; a second execute of the same plan
    bit-identical to the first.  Prints e / (u log2 n) before it asserts.  Returns the result rows."""
    dt = np.dtype(dtype)
    x = make_input(case, dt) if x is None else x
    X = reference(case, x, kind, dt, fs) if expected is None else expected
    rows, width, odt = out_shape(case, kind, dt)
    assert X.shape == (rows, width)
    label = label or "%s %s %s" % (case, KIND_NAMES[kind], "fp32" if dt == C64 else "fp64")
    gin = A.Guarded(case.n_signals, case.pitch * dt.itemsize, align16=True)
    outs = [A.Guarded(rows, width * odt.itemsize, align16=True) for _ in range(2)]
    try:
        A.upload_rows(gin, x)
        for g in outs:
            g.fill(np.full(width, np.nan, dtype=odt))
            run(gin.ptr, case.pitch, g.ptr)
            assert g.guards_intact(), "%s: the execute wrote outside its output" % label
        assert gin.guards_intact(), "%s: the execute wrote next to its input" % label
        assert A.input_unchanged(gin, x), "%s: the execute changed its input" % label
        y = outs[0].rows_at(0, rows, odt, width)
        e, k = A.row_errors(y, X, scale="rms" if kind == STFT else "rms_or_bin")
        unit = A.U[dt] * max(1.0, np.log2(case.n))
        print("%s: worst e / (u log2 n) = %.3f (row %d, bin %d)" % (label, float(np.max(e)) / unit, int(np.argmax(e)), int(k[int(np.argmax(e))])))
        if report:
            A._note(FAMILY[kind], dt, case.n, None, e)
        A.assert_within(e, k, bound(kind, dt, case.n), label)
        b = A.same_bits(outs[0], outs[1], odt, width)
        assert b is None, "%s: two executes of one plan differ at row %d" % (label, b)
        return y
    finally:
        gin.free()
        for g in outs:
            g.free()
