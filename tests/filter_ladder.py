"""The cases at which overlap-save FIR filtering (csrc/fft_plans_ext.h FilterPlan; tile_fft_kernel HOOK bits 8 and 9, filter_gather_kernel,
filter_scatter_kernel) is checked against direct convolution, on the GPU (tests/test_gpu_filter.py) and in the CPU emulation
(tests/test_emulated_filter.py), with the inputs, the reference and the checkers both files share.  Test infrastructure only.

A backend is a function
    run_plan(h, signal_len, n_signals, n, mode, dtype, x_ptr, x_pitch, y_ptr, y_pitch, no_fusion=False, no_chain=False, lds_budget=0,
             x2_ptr=None, y2_ptr=None) -> (rc, path, n_used)
that builds ONE plan, executes x into y (then x2 into y2 with the same plan), waits, and destroys the plan: rc 0 / -1 plan refused /
-2 execute refused; path = fft_gpu_plan_info_hip().fused (3: the one-launch kernel; 2, 1, 0: the fallback).

Reference: direct convolution, more exact than the thing under test -- float64 np.convolve for fp32; for fp64 np.convolve in
np.longdouble on real and imaginary parts separately (64 mantissa bits, checked at import: without them the fp64 inputs are small
integers, for which float64 convolution is exact).
Error: max |y - ref| over a signal / RMS of ref over that signal, in units of u log2 n (n = the block length); random complex taps, so
no output signal has a vanishing RMS.
Bound: K = 10, by accuracy.py's rule: at least twice the worst value measured in the emulation and on the device.  Worst measured, in
u log2 n (profiles/filter_accuracy_report.json): emulation 1.74 (fp32) / 1.69 (fp64) on the one-launch path, 4.61 (fp32) / 1.69 (fp64)
on the fallback; MI355X 1.48 / 1.83 on both paths.  The 4.61 is the frames_exact case of tests/test_emulated_filter.py: the maximum
over 10^5 output samples of one signal at n = 4, where log2 n = 2 makes the unit small; every other case stays below 2.6.
"""
import numpy as np

import accuracy as A

C64, C128 = np.dtype(np.complex64), np.dtype(np.complex128)
BOTH = (C64, C128)
FULL, CAUSAL, CENTRED = range(3)
MODES = (FULL, CAUSAL, CENTRED)
MODE_NAMES = {FULL: "full", CAUSAL: "causal", CENTRED: "same"}
BOUND_K = 10
NMAX = {C64: 4096, C128: 2048}   # the largest block length of the one-launch path
GUARD = 64                       # elements of sentinel before and behind every buffer
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
# the fp64 reference must be more exact than float64: 64 mantissa bits, or integer inputs (integer_inputs) on which float64 is exact
assert LONGDOUBLE_OK or np.finfo(np.longdouble).nmant == 52


class Case:
    """n: block length (0: the plan chooses), M taps, S signals of slen samples; xpad / ypad: pitch - row length; off: both base
    pointers are moved by this many elements (1: fp32 pointers are only 8-byte aligned); fused: the one-launch path is expected."""

    def __init__(self, name, n, M, slen, S=1, xpad=0, ypad=0, off=0, dtypes=BOTH, fused=True, n_used=None, why=""):
        self.name, self.n, self.M, self.slen, self.S, self.xpad, self.ypad, self.off = name, n, M, slen, S, xpad, ypad, off
        self.dtypes, self.fused, self.n_used, self.why = dtypes, fused, n_used or n, why

    def __repr__(self):
        return self.name

    def out_len(self, mode):
        return self.slen + self.M - 1 if mode == FULL else self.slen

    def out_off(self, mode):
        return (self.M - 1) // 2 if mode == CENTRED else 0


# B = n - (M - 1).  Every shape is the smallest that reaches its hazard.
SMALL = [
    Case("n4-M1", 4, 1, 9, why="M = 1: nothing is dropped, B = n; 9 = 2 B + 1"),
    Case("n4-M2", 4, 2, 7, 3, why="B = 3, 7 = 2 B + 1, three signals"),
    Case("n4-M3", 4, 3, 6, why="M = n/2 + 1, B = 2, 6 = 3 B"),
    Case("n8-Mn", 8, 8, 20, 3, why="M = n: B = 1, one output sample per block"),
    Case("n8-M5", 8, 5, 13, why="M = n/2 + 1"),
    Case("n8-len1", 8, 4, 1, why="M = n/2; a signal of one sample"),
    Case("n64-M1", 64, 1, 130, why="M = 1 at n = 64: the store starts at l = 0"),
    Case("n64-M2", 64, 2, 63 * 3, why="signal_len = 3 B exactly; the store starts at l = 1 (misaligned in fp32)"),
    Case("n64-M3-odd", 64, 3, 62 * 3 + 1, 3, xpad=1, ypad=1, why="M - 1 = 2 = V (fp32); 3 B + 1; odd pitches, NaN gaps"),
    Case("n64-M3-kBm1", 64, 3, 62 * 3 - 1, why="3 B - 1"),
    Case("n64-M32", 64, 32, 33 * 37 - 1, 5, why="5 signals x 37 / 38 blocks: tiles straddle signals, ragged last tile; M = n/2"),
    Case("n64-M33-off", 64, 33, 32 * 4 + 1, 3, xpad=3, ypad=5, off=1, why="M = n/2 + 1; base pointers offset by one element, odd pitches"),
    Case("n64-short", 64, 5, 17, 3, why="signal_len < B: one block (FULL: its tail reads only zeros)"),
    Case("n64-tail", 64, 17, 48 * 2 + 40, 1, why="the last block reads past the end of the signal; FULL adds a tail block"),
    Case("n256-M17", 256, 17, 1000, 3, xpad=2, ypad=2, why="even pitches with NaN gaps: 16-byte accesses next to the gaps"),
    Case("n256-M128", 256, 128, 129 * 3 - 1, why="M = n/2 at n = 256"),
    Case("n1024-M255", 1024, 255, 3000, off=1, why="n = 1024; base pointers offset by one element"),
    Case("n0-M31", 0, 31, 1000, 2, n_used=256, why="n = 0: max(256, next_pow2(124)) = 256"),
]
LARGEST = [Case("n4096-fp32", 4096, 255, 10000, 2, dtypes=(C64,), why="the largest one-launch block length, fp32"),
           Case("n2048-fp64", 2048, 255, 6000, 2, dtypes=(C128,), why="the largest one-launch block length, fp64")]
ABOVE = [Case("n8192-fp32", 8192, 255, 20000, dtypes=(C64,), fused=False, why="above the largest: the fallback"),
         Case("n4096-fp64", 4096, 255, 10000, dtypes=(C128,), fused=False, why="above the largest: the fallback"),
         Case("long-fp32", 0, 2049, 5000, dtypes=(C64,), fused=False, n_used=16384, why="n_taps = nmax/2 + 1: next_pow2(4 M) on the fallback"),
         Case("long-fp64", 0, 1025, 5000, dtypes=(C128,), fused=False, n_used=8192, why="n_taps = nmax/2 + 1: next_pow2(4 M) on the fallback")]
CASE_STRADDLE = next(c for c in SMALL if c.name == "n64-M32")


def integer_inputs(dtype):
    return np.dtype(dtype) == C128 and not LONGDOUBLE_OK


def taps(case, dtype, seed=11):
    rng = np.random.default_rng(seed + case.M)
    h = rng.standard_normal(case.M) + 1j * rng.standard_normal(case.M)
    if integer_inputs(dtype):
        h = np.round(h.real * 4) + 1j * np.round(h.imag * 4) + (1 + 1j)
    return h.astype(dtype)


def signals(case, dtype, seed=7):
    """[S][slen] complex normal values (small integers where the fp64 reference has no longer format to be exact in)."""
    x = A.block_normal_rows(case.slen, 0, case.S, dtype, seed).copy()
    if integer_inputs(dtype):
        x = (np.round(x.real * 8) + 1j * np.round(x.imag * 8)).astype(dtype)
    return x


def full_convolution(x, h, dtype):
    """[S][slen + M - 1]: float64 for fp32 inputs, np.longdouble parts for fp64 inputs."""
    if np.dtype(dtype) == C64 or not LONGDOUBLE_OK:
        x, h = x.astype(np.complex128), h.astype(np.complex128)
        return np.stack([np.convolve(r, h) for r in x])
    L = np.longdouble
    hr, hi = h.real.astype(L), h.imag.astype(L)
    out = []
    for r in x:
        xr, xi = r.real.astype(L), r.imag.astype(L)
        re, im = np.convolve(xr, hr) - np.convolve(xi, hi), np.convolve(xr, hi) + np.convolve(xi, hr)
        out.append(re.astype(np.clongdouble) + 1j * im.astype(np.clongdouble))
    return np.stack(out)


def reference(case, x, h, mode, dtype):
    f = full_convolution(x, h, dtype)
    o = case.out_off(mode)
    return f[:, o:o + case.out_len(mode)]


def errors(y, ref):
    """max |y - ref| / RMS(ref) per signal, as float64."""
    d = np.max(np.abs(y.astype(ref.dtype) - ref), axis=1).astype(np.float64)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=1)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = d / rms
    e[np.isnan(e)] = np.inf
    return e


def unit(dtype, n):
    return A.U[np.dtype(dtype)] * max(1.0, np.log2(n))


class Flat:
    """S rows of `length` elements, `pitch` apart, in one allocation of A.memory(): GUARD elements of sentinel in front, `off` more
    before row 0, GUARD behind the last row.  Everything that is not a row holds A.SENTINEL words (NaN as a float of either width)."""

    def __init__(self, S, length, pitch, dtype, off=0):
        self.S, self.length, self.pitch, self.dt, self.off = S, length, pitch, np.dtype(dtype), off
        self.first = GUARD + off
        self.total = self.first + (S - 1) * pitch + length + GUARD
        self.base, self.handle = A.memory().alloc(self.total * self.dt.itemsize)
        assert self.base % 16 == 0
        self.ptr = self.base + self.first * self.dt.itemsize
        self.image = None

    def put(self, rows=None):
        """Upload: sentinel everywhere, `rows` ([S][length]) in the rows (None: the rows hold sentinel as well)."""
        img = np.full(self.total * self.dt.itemsize // 4, A.SENTINEL, dtype=np.uint32).view(self.dt)
        if rows is not None:
            for s in range(self.S):
                img[self.first + s * self.pitch:self.first + s * self.pitch + self.length] = rows[s]
        self.image = img.copy()
        A.h2d(self.base, img)

    def get(self):
        """(rows [S][length], True if every element outside the rows still holds what put() wrote, bit for bit)"""
        img = A.d2h(self.base, (self.total,), self.dt)
        mask = np.ones(self.total, dtype=bool)
        rows = np.empty((self.S, self.length), dtype=self.dt)
        for s in range(self.S):
            a = self.first + s * self.pitch
            rows[s] = img[a:a + self.length]
            mask[a:a + self.length] = False
        w = self.dt.itemsize // 4
        same = np.array_equal(img.view(np.uint32).reshape(-1, w)[mask], self.image.view(np.uint32).reshape(-1, w)[mask])
        return rows, same

    def free(self):
        A.memory().free(self.handle)


def run_once(run_plan, case, mode, dtype, x, h, x2=None, **opts):
    """One plan on guarded, NaN-gapped buffers.  Returns (y, y2 or None, path, n_used); asserts rc, guards, gaps and the input."""
    dt = np.dtype(dtype)
    ol = case.out_len(mode)
    fx = Flat(case.S, case.slen, case.slen + case.xpad, dt, case.off)
    fy = Flat(case.S, ol, ol + case.ypad, dt, case.off)
    fx2 = Flat(case.S, case.slen, case.slen + case.xpad, dt, case.off) if x2 is not None else None
    fy2 = Flat(case.S, ol, ol + case.ypad, dt, case.off) if x2 is not None else None
    try:
        fx.put(x)
        fy.put(None)
        if x2 is not None:
            fx2.put(x2)
            fy2.put(None)
        rc, path, n_used = run_plan(h, case.slen, case.S, case.n, mode, dt, fx.ptr, case.slen + case.xpad if case.xpad else 0, fy.ptr,
                                    ol + case.ypad if case.ypad else 0, x2_ptr=fx2.ptr if fx2 else None, y2_ptr=fy2.ptr if fy2 else None, **opts)
        assert rc == 0, (case, mode, rc)
        y, ok = fy.get()
        assert ok, "%s %s: the execute wrote outside the out_len samples of its signals" % (case, MODE_NAMES[mode])
        xin, ok = fx.get()
        assert ok and np.array_equal(xin.view(np.uint8), np.ascontiguousarray(x).view(np.uint8)), "%s: the execute changed its input" % case
        y2 = None
        if x2 is not None:
            y2, ok = fy2.get()
            assert ok
        return y, y2, path, n_used
    finally:
        for f in (fx, fy, fx2, fy2):
            if f is not None:
                f.free()


def check(run_plan, case, mode, dtype, label="", report=True, expect_path=None, **opts):
    """One plan for `case` in `mode`: every signal within BOUND_K u log2 n of the reference, nothing written outside the signals, the
    NaN gaps of the input never read (a block that read one fails its signal), the path as expected.  Prints before it asserts."""
    dt = np.dtype(dtype)
    x, h = signals(case, dt), taps(case, dt)
    ref = reference(case, x, h, mode, dt)
    y, _, path, n_used = run_once(run_plan, case, mode, dt, x, h, **opts)
    label = label or "%s %s %s" % (case, MODE_NAMES[mode], "fp32" if dt == C64 else "fp64")
    assert n_used == case.n_used, (label, n_used)
    e = errors(y, ref) / unit(dt, n_used)
    print("%s: path %d, worst e / (u log2 n) = %.3f (signal %d)" % (label, path, float(np.max(e)), int(np.argmax(e))))
    if report:
        A._note("filter_fused" if path == 3 else "filter_fallback", dt, n_used, None, np.max(e), unit=1.0)
    if expect_path is None:
        assert (path == 3) == case.fused, (label, path)
    else:
        assert path in expect_path, (label, path)
    assert float(np.max(e)) <= BOUND_K, "%s: %.3f u log2 n > %d" % (label, float(np.max(e)), BOUND_K)
    return y, path


def check_paths_agree(run_plan, case, mode, dtype):
    """The one-launch path against FFT_GPU_OPT_NO_FUSION: each within the bound of the reference (check), the fallback reporting 0."""
    y3, p3 = check(run_plan, case, mode, dtype)
    y0, p0 = check(run_plan, case, mode, dtype, label="%s %s no_fusion" % (case, MODE_NAMES[mode]), expect_path=(0,), no_fusion=True)
    assert p3 == 3 and p0 == 0


def check_impulses(run_plan, dtype, n=64, M=9):
    """A unit impulse at the last sample of a block's advance and at the first of the next, every mode: the output is the taps, shifted,
    compared tap by tap (error / RMS of the taps within the bound), exact zeros elsewhere being part of the same comparison."""
    dt = np.dtype(dtype)
    B = n - (M - 1)
    case = Case("impulse", n, M, 3 * B + 5, 2)
    h = taps(case, dt)
    for mode in MODES:
        for t in (B - 1, B, 2 * B - 1, 2 * B):
            x = np.zeros((case.S, case.slen), dtype=dt)
            x[0, t] = 1.0
            x[1, case.slen - 1] = 1.0
            ref = reference(case, x, h, mode, dt)
            y, _, path, _ = run_once(run_plan, case, mode, dt, x, h)
            e = errors(y, ref) / unit(dt, n)
            print("impulse at %d, %s: %.3f" % (t, MODE_NAMES[mode], float(np.max(e))))
            assert path == 3 and float(np.max(e)) <= BOUND_K, (mode, t, e)


def check_linear_operator(run_plan, dtype, **opts):
    """A NaN / Inf signal leaves every other signal bit-identical; zeros give exact zeros; scaling x by a power of two scales y exactly."""
    dt = np.dtype(dtype)
    case = Case("operator", 64, 17, 48 * 5 + 7, 3, xpad=1, ypad=1)
    x, h = signals(case, dt), taps(case, dt)
    for mode in MODES:
        y, _, _, _ = run_once(run_plan, case, mode, dt, x, h, **opts)
        for poison in (np.nan, np.inf):
            xp = x.copy()
            xp[1, :] = poison
            yp, _, _, _ = run_once(run_plan, case, mode, dt, xp, h, **opts)
            for s in (0, 2):
                assert np.array_equal(yp[s].view(np.uint8), y[s].view(np.uint8)), "signal %d changed next to a poisoned one (%s)" % (s, MODE_NAMES[mode])
            assert not np.all(np.isfinite(yp[1]))
        yz, _, _, _ = run_once(run_plan, case, mode, dt, np.zeros_like(x), h, **opts)
        assert np.all(yz == 0), "zeros in, something else out (%s)" % MODE_NAMES[mode]
        for k in (3, -5):
            ys, _, _, _ = run_once(run_plan, case, mode, dt, (x * dt.type(2.0 ** k)).astype(dt), h, **opts)
            assert np.array_equal(ys, y * dt.type(2.0 ** k)), "scaling by 2^%d is not exact (%s)" % (k, MODE_NAMES[mode])


def check_two_executes(run_plan, dtype, **opts):
    """Two executes of one plan with different data: the second result is that of a fresh plan on the second data, bit for bit."""
    dt = np.dtype(dtype)
    case = CASE_STRADDLE
    h = taps(case, dt)
    xa, xb = signals(case, dt, seed=7), signals(case, dt, seed=8)
    _, y2, _, _ = run_once(run_plan, case, FULL, dt, xa, h, x2=xb, **opts)
    yb, _, _, _ = run_once(run_plan, case, FULL, dt, xb, h, **opts)
    assert np.array_equal(y2.view(np.uint8), yb.view(np.uint8)), "the second execute differs from a fresh plan's"
    e = errors(y2, reference(case, xb, h, FULL, dt)) / unit(dt, case.n)
    assert float(np.max(e)) <= BOUND_K
