"""The cases at which the inverse STFT plan (csrc/fft_plans_ext.h IFramesPlan: one-sided rows back to real signals by weighted
overlap-add) is checked sample by sample against float64, on the GPU (tests/test_gpu_iframes.py) and in the CPU emulation
(tests/test_emulated_iframes.py), with the inputs, the float64 reference and the checker both files share.  Test infrastructure only.

Every shape is the smallest that reaches its hazard (n = 64: a half-length core of 32, tiles of 64 (fp32) / 32 (fp64) frames).  The
input is random complex spectra -- not the STFT of anything, imaginary parts in bins 0 and n/2 included -- unless a case says so.

Reference (numpy, float64): the rows cast to complex128 FIRST, the imaginary parts of bins 0 and n/2 zeroed, np.fft.irfft(., n), the
window in float64 (window64(): frames_ladder.window_values' formulas; a USER window: the plan's own values), a plain loop over the frames that adds
g * v_w into the signal and g^2 into the envelope, then a division where env > 1e-10 max g^2 and 0 elsewhere.

Bound per sample -- derived, not measured:

    |y - y_ref|[t] <= K u log2(n) inv_env[t] sum_w |g[t - w hop]| rms(v_w)  +  (cover(t) + 3) u |y_ref[t]|

The first term is the transform's: frame w carries an error of at most K u log2(n) rms(v_w) per sample (K = 8, the project's bound
for the r2c / c2r and frames paths), weighted by |g| and divided by the envelope like the sample itself.  The second is the
overlap-add's: cover(t) products and additions (accumulated in double, so this is generous), the rounding of the window values and of
1 / env to the plan's precision, and the final rounding.  Where the envelope vanishes both terms are 0: the sample must be exactly 0.
Every sample of every signal is checked.

Worst e / (u log2 n), e = |y - y_ref| / (inv_env sum_w |g| rms(v_w)), measured over this ladder (profiles/iframes_accuracy_report.json):
                 iframes fp32 / fp64     iframes_fallback fp32 / fp64
    MI355X       not measured yet
    emulation    1.65 / 1.97             1.38 / 1.70
All are <= 4, so K stays 8 (tests/accuracy.py's rule: K at least twice the worst measured value).

Round trip istft(stft(x)) against x: the forward leg is the real frames plan, whose rows are within rframes_ladder's 8 u log2(n) of
the row's RMS; the inverse transform is unitary up to its 1 / sqrt(n), so that error reaches the frame's samples as at most
8 u log2(n) rms(v_w) and is charged like the inverse's own: the first term with K = 8 + 8.
"""
import numpy as np

import accuracy as A
import frames_ladder as L
from frames_ladder import BLACKMAN, HAMMING, HANN, RECT, USER, WINDOW_NAMES  # noqa: F401

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BOTH = (F32, F64)
BOUND_K = 8
ROUND_TRIP_K = 8 + 8  # this ladder's K plus rframes_ladder.BOUND_K[STFT]
ENV_EPS = 1e-10  # scipy.signal.istft's constant


class Case:
    """n, hop, nw frames per signal, n_signals; pad: signal_pitch - out_len; offset: reals between a 16-byte boundary and the output."""

    def __init__(self, name, n, hop, nw, n_signals, window=HAMMING, pad=0, offset=0, dtypes=BOTH, why=""):
        self.name, self.n, self.hop, self.nw, self.n_signals = name, n, hop, nw, n_signals
        self.window, self.pad, self.offset, self.dtypes, self.why = window, pad, offset, dtypes, why
        self.out_len = (nw - 1) * hop + n
        self.pitch = self.out_len + pad
        self.bins = n // 2 + 1

    def __repr__(self):
        return self.name


SMALL = [
    Case("a", 64, 16, 30, 5, why="150 frames: tiles straddle signals, the last tile is ragged"),
    Case("a-hop15", 64, 15, 30, 5, why="the cover count varies along the signal, uneven frame starts"),
    Case("a-hop18", 64, 18, 30, 5, why="the cover count varies along the signal, uneven frame starts"),
    Case("b-nooverlap", 64, 64, 30, 5, why="hop = n: one frame per sample"),
    Case("b-hop1", 64, 1, 30, 5, why="hop = 1: 64 terms per sample"),
    Case("c-oneframe", 64, 16, 1, 37, why="one frame per signal, 37 signals"),
    Case("h-rect", 256, 64, 2, 3, window=RECT, why="window kind; no unrecoverable sample"),
    Case("h-hann", 256, 64, 2, 3, window=HANN, why="window kind; the two end samples are unrecoverable"),
    Case("h-hamming", 256, 64, 2, 3, window=HAMMING, why="window kind"),
    Case("h-blackman", 256, 64, 2, 3, window=BLACKMAN, why="window kind"),
    Case("h-user", 256, 64, 2, 3, window=USER, why="a random, asymmetric window: a reversed or pair-swapped window fails"),
    Case("p-pitch", 64, 16, 30, 5, pad=5, offset=1, why="signal_pitch = out_len + 5, the output one real behind a 16-byte boundary"),
    Case("n4", 4, 2, 5, 3, why="n = 4: L = 2, the fallback"),
]
CASE_A = SMALL[0]
IMPULSES = Case("impulses", 64, 64, 64, 1, window=RECT, why="row w = exp(-2 pi i w k / n): frame w is a unit impulse at its sample w")
ROUND_TRIPS = [Case("rt-64", 64, 16, 30, 5, why="istft(stft(x)), hop = n/4"), Case("rt-256", 256, 64, 6, 3, why="istft(stft(x)), hop = n/4")]
# on the device: the largest frames of the one-launch path, and the fallback
GPU_F = [Case("f-fp32", 8192, 4096, 3, 5, dtypes=(F32,), why="the largest fused frame, fp32"),
         Case("f-fp64", 4096, 2048, 3, 5, dtypes=(F64,), why="the largest fused frame, fp64")]
GPU_G = [Case("g", 16384, 8192, 3, 3, why="the fallback: merge, multi-pass core, overlap-add")]
# in the emulation: the one-launch path at n = 512, and the fallback under the LDS budgets that give the half-length core two passes
# (n = 512: a core of 256 under 4096 bytes) and three (n = 8192: a core of 4096 under 4096 bytes) -- as rframes_ladder.EMU_G
EMU_F = [Case("f", 512, 256, 3, 5, why="the one-launch path at n = 512")]
EMU_G = [(Case("g-2pass", 512, 256, 3, 3, why="fallback, two passes"), 4096, 2),
         (Case("g-3pass", 8192, 4096, 3, 3, why="fallback, three passes"), 4096, 3)]


def complex_dtype(dtype):
    return L.C64 if np.dtype(dtype) == F32 else L.C128


def user_window(case, dtype):
    """The n values handed to the plan for a USER window (None otherwise), in the plan's precision."""
    return np.ascontiguousarray(L.window_values(USER, case.n).astype(np.dtype(dtype))) if case.window == USER else None


def window64(case, dtype):
    """The window in float64: frames_ladder.window_values' formulas, evaluated in extended precision and rounded once.  Evaluated in
    float64 they cancel near the ends (0.5 (1 - cos a) keeps 41 of 53 bits at a = 2 pi / 255, Blackman fewer), and the overlap-add
    divides by these values where one frame covers a sample: the reference's own error would exceed the fp64 bound there."""
    if case.window == USER:
        return user_window(case, dtype).astype(np.float64)
    n = case.n
    a = np.longdouble("6.283185307179586476925286766559005768") * np.arange(n, dtype=np.longdouble) / np.longdouble(n - 1)
    half, one = np.longdouble("0.5"), np.longdouble(1)
    if case.window == RECT:
        w = np.ones(n, dtype=np.longdouble)
    elif case.window == HANN:
        w = half * (one - np.cos(a))
    elif case.window == HAMMING:
        w = np.longdouble("0.54") - np.longdouble("0.46") * np.cos(a)
    else:
        w = np.longdouble("0.42") - half * np.cos(a) + np.longdouble("0.08") * np.cos(2 * a)
    return w.astype(np.float64)


def make_spectra(case, dtype, seed=11):
    """[n_signals][nw][n/2 + 1] complex normal values, the imaginary parts of bins 0 and n/2 too."""
    cdt = complex_dtype(dtype)
    real = np.float32 if cdt == L.C64 else np.float64
    shape = (case.n_signals, case.nw, case.bins)
    return np.random.default_rng((seed, case.n, case.hop)).standard_normal(shape + (2,)).astype(real).view(cdt).reshape(shape)


def impulse_spectra(case, dtype):
    """IMPULSES: row w = exp(-2 pi i w k / n), k <= n/2; and the signal expected of it: frame w is a unit impulse at its sample w."""
    n = case.n
    w = np.arange(case.nw)
    X = np.exp(-2j * np.pi * (np.outer(w, np.arange(case.bins)) % n) / n).astype(complex_dtype(dtype)).reshape(1, case.nw, case.bins)
    y = np.zeros((1, case.out_len))
    y[0, w * case.hop + w] = 1.0
    return X, y


def reference(case, X, dtype, K=BOUND_K):
    """(y_ref [S][out_len] float64, limit [S][out_len], scale [S][out_len], unrecoverable samples per signal).
    limit: the bound of the module docstring; scale = inv_env sum_w |g| rms(v_w), the unit of its first term."""
    n, hop, nw, S = case.n, case.hop, case.nw, case.n_signals
    Z = np.array(X, dtype=np.complex128).reshape(S, nw, case.bins)
    Z[:, :, 0] = Z[:, :, 0].real
    Z[:, :, n // 2] = Z[:, :, n // 2].real
    v = np.fft.irfft(Z, n, axis=-1)
    return overlap_add(case, v, dtype, K)


def overlap_add(case, v, dtype, K=BOUND_K):
    """reference() from the float64 frames v [S][nw][n]."""
    n, hop, nw, S = case.n, case.hop, case.nw, case.n_signals
    g = window64(case, dtype)
    rms = np.sqrt(np.mean(v * v, axis=-1))  # [S][nw]
    num = np.zeros((S, case.out_len))
    mag = np.zeros((S, case.out_len))
    env = np.zeros(case.out_len)
    cover = np.zeros(case.out_len)
    for w in range(nw):
        sl = slice(w * hop, w * hop + n)
        num[:, sl] += g * v[:, w, :]
        mag[:, sl] += np.abs(g) * rms[:, w, None]
        env[sl] += g * g
        cover[sl] += 1
    good = env > ENV_EPS * np.max(g * g)
    inv_env = np.where(good, 1.0 / np.where(good, env, 1.0), 0.0)
    y = num * inv_env
    scale = mag * inv_env
    u = A.U[np.dtype(dtype)]
    limit = K * u * max(1.0, np.log2(n)) * scale + (cover + 3) * u * np.abs(y)
    return y, limit, scale, int(np.sum(~good))


NAN_BITS = {F32: np.uint32(0x7FC5A5A5), F64: np.uint64(0x7FF85A5A5A5A5A5A)}  # the NaN pattern the output is pre-filled with


def nan_fill(count, dtype):
    dt = np.dtype(dtype)
    return np.full(count, NAN_BITS[dt]).view(dt)


class Output:
    """The output of one execute: `offset` reals behind a 16-byte boundary, n_signals * pitch reals, all pre-filled with a NaN
    pattern, between two guards."""

    def __init__(self, case, dtype):
        self.case, self.dt = case, np.dtype(dtype)
        self.count = case.offset + case.n_signals * case.pitch
        nbytes = -(-self.count * self.dt.itemsize // 4) * 4
        self.g = A.Guarded(1, nbytes, align16=True)
        self.g.upload(nan_fill(self.count, self.dt).reshape(1, -1))
        self.ptr = self.g.ptr + case.offset * self.dt.itemsize

    def read(self):
        """(y [S][out_len], everything else as one array of bit patterns)"""
        c = self.case
        flat = self.g.rows_at(0, 1, self.dt, self.count)[0]
        body = flat[c.offset:].reshape(c.n_signals, c.pitch)
        rest = np.concatenate([flat[:c.offset], body[:, c.out_len:].reshape(-1)])
        return body[:, :c.out_len].copy(), rest.view(NAN_BITS[self.dt].dtype)

    def free(self):
        self.g.free()


def sample_check(y, y_ref, limit, scale, case, dtype, label, family=None):
    """Every sample of every signal within its limit (a NaN fails); prints e / (u log2 n) before it asserts."""
    dt = np.dtype(dtype)
    d = np.abs(y.astype(np.float64) - y_ref)
    d = np.where(np.isnan(d), np.inf, d)
    unit = A.U[dt] * max(1.0, np.log2(case.n))
    e = np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d == 0, 0.0, np.inf))
    s, t = np.unravel_index(int(np.argmax(e)), e.shape)
    print("%s: worst e / (u log2 n) = %.3f (signal %d, sample %d)" % (label, float(e[s, t]) / unit, s, t))
    if family:
        A._note(family, dt, case.n, None, e)
    bad = np.argwhere(~(d <= limit))
    if bad.size:
        s, t = bad[0]
        raise A.AccuracyError("%s: %d of %d samples over their bound; first: signal %d sample %d is %r, expected %r, bound %.3g (%.1f x)"
                              % (label, len(bad), d.size, s, t, y[s, t], y_ref[s, t], limit[s, t], d[s, t] / max(limit[s, t], 1e-300)))


def check(run, case, dtype, X=None, expected=None, K=BOUND_K, label="", family=None):
    """run(X_ptr, y_ptr, signal_pitch): one execute of an inverse frames plan for `case`, finished when it returns.
    The rows live in a Guarded of their own; the output is an Output (NaN pattern, guards).  Checked: every sample of every signal
    within its bound (so none keeps the NaN pattern); a sample whose envelope vanishes is exactly 0; the padding between signals, the
    reals before the output and the guards hold their pattern bit for bit; the input byte for byte; a second execute of the same
    plan bit-identical to the first.  expected: (y_ref, limit, scale, unrecoverable) instead of reference(case, X).
    Returns (y, unrecoverable samples per signal of the reference)."""
    dt = np.dtype(dtype)
    cdt = complex_dtype(dt)
    X = make_spectra(case, dt) if X is None else X
    y_ref, limit, scale, lost = reference(case, X, dt, K) if expected is None else expected
    label = label or "%s %s" % (case, "fp32" if dt == F32 else "fp64")
    rows = X.reshape(case.n_signals * case.nw, case.bins)
    gin = A.Guarded(rows.shape[0], case.bins * cdt.itemsize, align16=True)
    outs = [Output(case, dt) for _ in range(2)]
    try:
        A.upload_rows(gin, rows)
        res = []
        for o in outs:
            run(gin.ptr, o.ptr, 0 if (case.pad == 0 and case.offset == 0) else case.pitch)
            assert o.g.guards_intact(), "%s: the execute wrote outside its output" % label
            y, rest = o.read()
            assert np.all(rest == NAN_BITS[dt]), "%s: the execute wrote between the signals or before the output" % label
            res.append(y)
        assert gin.guards_intact(), "%s: the execute wrote next to its input" % label
        assert A.input_unchanged(gin, rows), "%s: the execute changed its input" % label
        y = res[0]
        sample_check(y, y_ref, limit, scale, case, dt, label, family)
        assert np.array_equal(res[0].view(np.uint8), res[1].view(np.uint8)), "%s: two executes of one plan differ" % label
        return y, lost
    finally:
        gin.free()
        for o in outs:
            o.free()


def run_once(run, case, dtype, X):
    """One execute on fresh guarded buffers, no accuracy check: the signals [S][out_len] (bit-level comparisons between runs)."""
    dt = np.dtype(dtype)
    rows = np.ascontiguousarray(X.reshape(case.n_signals * case.nw, case.bins))
    gin = A.Guarded(rows.shape[0], case.bins * rows.dtype.itemsize, align16=True)
    o = Output(case, dt)
    try:
        A.upload_rows(gin, rows)
        run(gin.ptr, o.ptr, case.pitch)
        assert o.g.guards_intact() and gin.guards_intact()
        y, rest = o.read()
        assert np.all(rest == NAN_BITS[dt])
        return y
    finally:
        gin.free()
        o.free()


def check_edge_bins_ignored(run, case, dtype):
    """Nonzero imaginary parts in bins 0 and n/2: the result equals, bit for bit, the run with them zeroed."""
    X = make_spectra(case, dtype)
    assert np.all(X[:, :, 0].imag != 0) and np.all(X[:, :, -1].imag != 0)
    Z = X.copy()
    Z[:, :, 0] = Z[:, :, 0].real
    Z[:, :, -1] = Z[:, :, -1].real
    a, b = run_once(run, case, dtype, X), run_once(run, case, dtype, Z)
    assert np.all(np.isfinite(a))
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: the imaginary part of bin 0 or n/2 reached the result" % case


def check_nan_frame(run, case, dtype, s=2, w=7):
    """One frame's row all NaN: exactly the samples that frame covers are NaN in its signal, every other signal is bit-identical to
    the clean run (and so is the rest of its own)."""
    X = make_spectra(case, dtype)
    P = X.copy()
    P[s, w, :] = np.nan + 1j * np.nan
    a, b = run_once(run, case, dtype, X), run_once(run, case, dtype, P)
    assert np.all(np.isfinite(a))
    hit = np.zeros(a.shape, dtype=bool)
    hit[s, w * case.hop:w * case.hop + case.n] = True
    assert np.all(np.isnan(b[hit])), "%s: a sample the NaN frame covers is finite" % case
    assert np.array_equal(a[~hit].view(np.uint8), b[~hit].view(np.uint8)), "%s: a NaN frame changed samples it does not cover" % case


def round_trip_input(case, dtype, seed=23):
    return np.random.default_rng((seed, case.n)).standard_normal((case.n_signals, case.out_len)).astype(np.dtype(dtype))


def round_trip_expected(case, x, dtype):
    """The `expected` of check() for istft(stft(x)): x itself, the bound from the float64 windowed frames of x with ROUND_TRIP_K."""
    from numpy.lib.stride_tricks import as_strided
    xs = np.ascontiguousarray(x.astype(np.float64))
    fr = as_strided(xs, shape=(case.n_signals, case.nw, case.n), strides=(case.out_len * 8, case.hop * 8, 8), writeable=False)
    y, limit, scale, lost = overlap_add(case, fr * window64(case, dtype), dtype, ROUND_TRIP_K)
    assert lost == 0 and np.max(np.abs(y - xs)) < 1e-12  # the reference's own round trip
    return xs, limit, scale, lost
