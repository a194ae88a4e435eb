"""The cases at which the 2D convolution / spectrum-filtering plan (csrc/fft_plans_ext.h Conv2DPlan; csrc/fft_kernels_conv2d.h
tile_fft_colround_kernel, conv2d_pad_kernel, conv2d_crop_kernel) is checked against direct 2D convolution, on the GPU
(tests/test_gpu_conv2d.py) and in the CPU emulation (tests/test_emulated_conv2d.py), with the inputs, the reference and the checkers both
files share.  Test infrastructure only.

A backend is a function
    run_plan(k, rows, cols, n_matrices, mode, dtype, x_ptr, x_pitch, y_ptr, y_pitch, no_fusion=False, lds_budget=0, min_seg=0,
             x2_ptr=None, y2_ptr=None) -> (rc, info)
that builds ONE plan, executes x into y (then x2 into y2 with the same plan), waits, and destroys the plan: rc 0 / -1 plan refused /
-2 execute refused; info = dict(fused, n_passes, P, Q, out_rows, out_cols, tile_cols) from fft_gpu_plan_info_hip and the getters
(tile_cols: the emulation only, else 0).  lds_budget and min_seg exist in the emulation only (the NARROW cases).

Reference: direct 2D convolution in float64 numpy, a sum over the kernel's taps of shifted images (circular: rolled images); SPECTRUM:
float64 numpy.fft.ifft2(fft2(x) * H).
Error: filter_ladder's metric with n := P Q -- max |y - ref| over a matrix / RMS of ref over that matrix, in units of u log2(P Q).
Bound: K = 10, the filter plan's: the same forward / product / inverse chain, composed over both dimensions.  Worst measured, in u log2(P Q)
(profiles/conv2d_accuracy_report.json): emulation 1.28 (fp32) / 1.95 (fp64) on the fused path, 1.22 / 2.29 on the fallback; MI355X
1.28 / 2.29 and 1.23 / 2.67 -- all below half the bound.
"""
import numpy as np

import accuracy as A
import filter_ladder as FL

C64, C128 = FL.C64, FL.C128
BOTH = FL.BOTH
FULL, SAME, VALID, CIRCULAR, SPECTRUM = range(5)
LINEAR = (FULL, SAME, VALID)
MODE_NAMES = {FULL: "full", SAME: "same", VALID: "valid", CIRCULAR: "circular", SPECTRUM: "spectrum"}
BOUND_K = FL.BOUND_K
V = {C64: 2, C128: 1}   # complex values per 16-byte lane access


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


class Case:
    """rows x cols images, a krows x kcols kernel, M matrices; xpad / ypad: pitch - matrix size; fused: True / False the path the plan
    must report, a dict per dtype, or None (only the consistency of what it reports is checked)."""

    def __init__(self, name, rows, cols, krows, kcols, mode=FULL, M=3, xpad=3, ypad=5, fused=True, lds_budget=0, min_seg=0, tile_cols=None, why=""):
        self.name, self.rows, self.cols, self.krows, self.kcols, self.mode, self.M = name, rows, cols, krows, kcols, mode, M
        self.xpad, self.ypad, self.fused, self.lds_budget, self.min_seg, self.tile_cols, self.why = xpad, ypad, fused, lds_budget, min_seg, tile_cols, why

    def __repr__(self):
        return "%s-%s" % (self.name, MODE_NAMES[self.mode])

    def padded(self):
        if self.mode in (CIRCULAR, SPECTRUM):
            return self.rows, self.cols
        return next_pow2(self.rows + self.krows - 1), next_pow2(self.cols + self.kcols - 1)

    def out_shape(self):
        if self.mode == FULL:
            return self.rows + self.krows - 1, self.cols + self.kcols - 1
        if self.mode == VALID:
            return self.rows - self.krows + 1, self.cols - self.kcols + 1
        return self.rows, self.cols

    def expect_fused(self, dtype):
        f = self.fused
        return f[np.dtype(dtype)] if isinstance(f, dict) else f

    def with_(self, **kw):
        c = Case(self.name, self.rows, self.cols, self.krows, self.kcols, self.mode, self.M, self.xpad, self.ypad, self.fused, self.lds_budget,
                 self.min_seg, self.tile_cols, self.why)
        for a, b in kw.items():
            setattr(c, a, b)
        return c


def modes(case, which):
    return [case.with_(mode=m) for m in which]


# Every shape is the smallest that reaches its mechanism.  Fused needs P >= 8 (E = 8 values per thread) and tile rows of >= 64 bytes:
# Q >= 8 (fp32) / Q >= 4 (fp64).
SMALL = (
    modes(Case("p8-5x6-3x3", 5, 6, 3, 3, why="P = 8, Q = 8: the smallest E = 8 column tile, no LDS exchange in the stages"), LINEAR)
    + [Case("p4-2x3-2x2", 2, 3, 2, 2, fused=False, why="P = 4: below the smallest tile, must report the fallback"),
       Case("q4-12x2-3x2", 12, 2, 3, 2, fused={C64: False, C128: True}, why="Q = 4: 32-byte rows in fp32 (fallback), 64-byte rows in fp64 (one narrow tile)"),
       Case("q1-9x1-4x1", 9, 1, 4, 1, fused=False, why="Q = 1: no row transform at all"),
       Case("wide-5x200-3x31", 5, 200, 3, 31, why="P = 8, Q = 256: short columns, long rows"),
       Case("tall-200x5-31x3", 200, 5, 31, 3, why="P = 256, Q = 8: long columns (LDS exchanges), short rows"),
       Case("rin1-1x6-8x3", 1, 6, 8, 3, why="rows_in = 1, rows_out = P = 8"),
       Case("rinPm1-7x6-1x3", 7, 6, 1, 3, why="rows_in = rows_out = P - 1 = 7; krows = 1"),
       Case("rinP-8x8-3x3", 8, 8, 3, 3, mode=CIRCULAR, why="rows_in = rows_out = P (CIRCULAR)"),
       Case("rout1-5x6-5x3", 5, 6, 5, 3, mode=VALID, why="VALID with krows = rows: rows_out = 1 at P = 16"),
       Case("kcols1-5x6-4x1", 5, 6, 4, 1, why="kcols = 1"),
       Case("krows1-5x6-1x4", 5, 6, 1, 4, why="krows = 1"),
       Case("circ-8x16-3x5", 8, 16, 3, 5, mode=CIRCULAR, why="CIRCULAR, the kernel wraps in both directions"),
       Case("circ-16x8-16x1", 16, 8, 16, 1, mode=CIRCULAR, why="CIRCULAR, krows = rows")]
    + modes(Case("big-kernel-3x3-6x5", 3, 3, 6, 5, why="a kernel larger than the image"), (FULL, SAME))
    + [Case("same-9x9-%dx%d" % kk, 9, 9, kk[0], kk[1], mode=SAME, why="even and odd kernel sizes: SAME's offset (k - 1) / 2") for kk in ((4, 4), (3, 3), (4, 3), (3, 4))]
    + modes(Case("odd-pitch-15x9-2x8", 15, 9, 2, 8, xpad=1, ypad=1, why="P = Q = 16; odd pitches: rows that are only 8-byte aligned in fp32"), LINEAR)
)
IDENTITY = modes(Case("identity-5x6-1x1", 5, 6, 1, 1, why="1 x 1 kernel: identity"), LINEAR) + [Case("identity-8x8-1x1", 8, 8, 1, 1, mode=CIRCULAR)]
# the emulation only: the LDS budget and the row-segment criterion narrow the column tile to C = V and C = 2 V columns, 16 and 8 tiles per
# matrix at Q = 32; P = 64 so that the tile, not the row plan, is what the budget binds (tile bytes = 64 C sizeof + tables)
NARROW = [Case("narrow-50x27-3x3-C%dV" % m, 50, 27, 3, 3, mode=SAME, min_seg=16, lds_budget={C64: (2000, 3000), C128: (2500, 3500)}, tile_cols=m,
               why="C = %d V columns per tile" % m) for m in (1, 2)]


def images(case, dtype, seed=7):
    """[M][rows][cols] complex normal values"""
    return A.block_normal_rows(case.rows * case.cols, 0, case.M, dtype, seed).copy().reshape(case.M, case.rows, case.cols)


def kernel(case, dtype, seed=11):
    rng = np.random.default_rng(seed + 31 * case.krows + case.kcols)
    k = rng.standard_normal((case.krows, case.kcols)) + 1j * rng.standard_normal((case.krows, case.kcols))
    return k.astype(dtype)


def full_convolution(x, k):
    """[M][rows + krows - 1][cols + kcols - 1] in float64: a sum over the kernel's taps of shifted images"""
    x, k = x.astype(np.complex128), k.astype(np.complex128)
    M, r, c = x.shape
    kr, kc = k.shape
    out = np.zeros((M, r + kr - 1, c + kc - 1), dtype=np.complex128)
    for i in range(kr):
        for j in range(kc):
            out[:, i:i + r, j:j + c] += k[i, j] * x
    return out


def reference(case, x, k):
    if case.mode == SPECTRUM:
        return np.fft.ifft2(np.fft.fft2(x.astype(np.complex128)) * k.astype(np.complex128))
    if case.mode == CIRCULAR:
        x64, k64 = x.astype(np.complex128), k.astype(np.complex128)
        out = np.zeros_like(x64)
        for i in range(case.krows):
            for j in range(case.kcols):
                out += k64[i, j] * np.roll(x64, (i, j), axis=(1, 2))
        return out
    f = full_convolution(x, k)
    orows, ocols = case.out_shape()
    sr = (case.krows - 1) // 2 if case.mode == SAME else case.krows - 1 if case.mode == VALID else 0
    sc = (case.kcols - 1) // 2 if case.mode == SAME else case.kcols - 1 if case.mode == VALID else 0
    return f[:, sr:sr + orows, sc:sc + ocols]


def errors(y, ref):
    """max |y - ref| / RMS(ref) per matrix"""
    M = ref.shape[0]
    return FL.errors(y.reshape(M, -1), ref.reshape(M, -1))


def unit(dtype, P, Q):
    return A.U[np.dtype(dtype)] * max(1.0, np.log2(P * Q))


def run_once(run_plan, case, dtype, x, k, x2=None, no_fusion=False, contiguous=False):
    """One plan on guarded, NaN-gapped buffers.  Returns (y [M][out_rows][out_cols], y2 or None, info); asserts rc, guards, gaps, the input."""
    dt = np.dtype(dtype)
    orows, ocols = case.out_shape()
    nx, ny = case.rows * case.cols, orows * ocols
    xpad, ypad = (0, 0) if contiguous else (case.xpad, case.ypad)
    fx = FL.Flat(case.M, nx, nx + xpad, dt)
    fy = FL.Flat(case.M, ny, ny + ypad, dt)
    fx2 = FL.Flat(case.M, nx, nx + xpad, dt) if x2 is not None else None
    fy2 = FL.Flat(case.M, ny, ny + ypad, dt) if x2 is not None else None
    lds = case.lds_budget
    if isinstance(lds, dict):
        lds = lds[dt][case.tile_cols - 1]
    try:
        fx.put(x.reshape(case.M, nx))
        fy.put(None)
        if x2 is not None:
            fx2.put(x2.reshape(case.M, nx))
            fy2.put(None)
        rc, info = run_plan(k, case.rows, case.cols, case.M, case.mode, dt, fx.ptr, nx + xpad if xpad else 0, fy.ptr, ny + ypad if ypad else 0,
                            no_fusion=no_fusion, lds_budget=lds, min_seg=case.min_seg, x2_ptr=fx2.ptr if fx2 else None, y2_ptr=fy2.ptr if fy2 else None)
        assert rc == 0, (case, rc)
        assert (info["P"], info["Q"]) == case.padded() and (info["out_rows"], info["out_cols"]) == (orows, ocols), (case, info)
        assert (info["fused"], info["n_passes"]) in ((1, 3), (0, 5)), info
        y, ok = fy.get()
        assert ok, "%s: the execute wrote outside the out_rows x out_cols values of its matrices" % case
        xin, ok = fx.get()
        assert ok and np.array_equal(xin.view(np.uint8), np.ascontiguousarray(x.reshape(case.M, nx)).view(np.uint8)), "%s: the execute changed its input" % case
        y2 = None
        if x2 is not None:
            y2, ok = fy2.get()
            assert ok
            y2 = y2.reshape(case.M, orows, ocols)
        return y.reshape(case.M, orows, ocols), y2, info
    finally:
        for f in (fx, fy, fx2, fy2):
            if f is not None:
                f.free()


def check(run_plan, case, dtype, label="", no_fusion=False, contiguous=False, x=None, k=None, report=True):
    """One plan for `case`: every matrix within BOUND_K u log2(P Q) of the reference, nothing written outside the matrices, the NaN gaps
    of the input never read, the path as the case says.  Prints before it asserts."""
    dt = np.dtype(dtype)
    x = images(case, dt) if x is None else x
    k = kernel(case, dt) if k is None else k
    ref = reference(case, x, k)
    y, _, info = run_once(run_plan, case, dt, x, k, no_fusion=no_fusion, contiguous=contiguous)
    P, Q = case.padded()
    label = label or "%s %s%s%s" % (case, "fp32" if dt == C64 else "fp64", " no_fusion" if no_fusion else "", " contiguous" if contiguous else "")
    e = errors(y, ref) / unit(dt, P, Q)
    print("%s: fused %d, %d round trips, worst e / (u log2 PQ) = %.3f (matrix %d)" % (label, info["fused"], info["n_passes"], float(np.max(e)), int(np.argmax(e))))
    if report:
        A._note("conv2d_fused" if info["fused"] else "conv2d_fallback", dt, P * Q, None, np.max(e), unit=1.0)
    want = False if no_fusion else case.expect_fused(dt)
    if want is not None:
        assert info["fused"] == (1 if want else 0), (label, info)
    if case.tile_cols and not no_fusion:
        assert info["tile_cols"] == case.tile_cols * V[dt], (label, info)
    assert float(np.max(e)) <= BOUND_K, "%s: %.3f u log2 PQ > %d" % (label, float(np.max(e)), BOUND_K)
    return y, info


def check_paths_agree(run_plan, case, dtype):
    """The plan's own path and FFT_GPU_OPT_NO_FUSION on the same data, three pitched matrices; then one contiguous matrix."""
    check(run_plan, case, dtype)
    check(run_plan, case, dtype, no_fusion=True)
    one = case.with_(M=1)
    check(run_plan, one, dtype, contiguous=True)


def check_identity(run_plan, case, dtype):
    """k = [[1]]: the output is the image, within the bound; every mode has the image's shape"""
    dt = np.dtype(dtype)
    for no_fusion in (False, True):
        y, _ = check(run_plan, case, dt, k=np.ones((1, 1), dtype=dt), no_fusion=no_fusion)
        assert y.shape == (case.M, case.rows, case.cols)


def check_impulses(run_plan, dtype, no_fusion=False):
    """A unit impulse at each corner and at the centre of a 5 x 6 image, one per matrix: the output is the kernel at that offset, compared
    tap by tap through the reference (error / RMS of the taps within the bound)."""
    dt = np.dtype(dtype)
    for mode in LINEAR:
        case = Case("impulse", 5, 6, 3, 3, mode=mode, M=5)
        k = kernel(case, dt)
        x = np.zeros((5, 5, 6), dtype=dt)
        for m, (i, j) in enumerate(((0, 0), (0, 5), (4, 0), (4, 5), (2, 3))):
            x[m, i, j] = 1.0
        ref = reference(case, x, k)
        if mode == FULL:
            assert np.array_equal(ref[3, 4:7, 5:8], k.astype(np.complex128)) and np.count_nonzero(ref[3]) == 9  # the reference itself: taps in place
        y, _, info = run_once(run_plan, case, dt, x, k, no_fusion=no_fusion)
        e = errors(y, ref) / unit(dt, 8, 8)
        print("impulses, %s: %s" % (MODE_NAMES[mode], np.round(e, 3)))
        assert info["fused"] == (0 if no_fusion else 1) and float(np.max(e)) <= BOUND_K, (mode, e)


def check_linear_operator(run_plan, dtype, no_fusion=False):
    """A NaN / Inf matrix leaves every other matrix bit-identical; zeros give exact zeros; scaling x by a power of two scales y exactly;
    conv(a x1 + x2) = a conv(x1) + conv(x2) within the three results' own error bounds."""
    dt = np.dtype(dtype)
    for case in (Case("operator", 5, 6, 3, 3, mode=FULL), Case("operator", 5, 6, 3, 3, mode=SAME, xpad=1, ypad=1), Case("operator", 6, 5, 2, 3, mode=VALID),
                 Case("operator", 8, 8, 3, 3, mode=CIRCULAR)):
        x, k = images(case, dt), kernel(case, dt)
        y, _, info = run_once(run_plan, case, dt, x, k, no_fusion=no_fusion)
        assert info["fused"] == (0 if no_fusion else 1)
        for poison in (np.nan, np.inf):
            xp = x.copy()
            xp[1] = poison
            yp, _, _ = run_once(run_plan, case, dt, xp, k, no_fusion=no_fusion)
            for m in (0, 2):
                assert np.array_equal(yp[m].view(np.uint8), y[m].view(np.uint8)), "matrix %d changed next to a poisoned one (%s)" % (m, case)
            assert not np.all(np.isfinite(yp[1]))
        yz, _, _ = run_once(run_plan, case, dt, np.zeros_like(x), k, no_fusion=no_fusion)
        assert np.all(yz == 0), "zeros in, something else out (%s)" % case
        for s in (3, -5):
            ys, _, _ = run_once(run_plan, case, dt, (x * dt.type(2.0 ** s)).astype(dt), k, no_fusion=no_fusion)
            assert np.array_equal(ys, y * dt.type(2.0 ** s)), "scaling by 2^%d is not exact (%s)" % (s, case)
        # linearity: each of the three results is within K u log2(PQ) RMS(its reference) of its exact value, so their combination is within
        # the sum of the three bounds
        a = dt.type(0.75 - 1.5j)
        x2 = images(case, dt, seed=8)
        xs = (a * x + x2).astype(dt)
        y2, _, _ = run_once(run_plan, case, dt, x2, k, no_fusion=no_fusion)
        y12, _, _ = run_once(run_plan, case, dt, xs, k, no_fusion=no_fusion)
        P, Q = case.padded()
        rms = lambda r: np.sqrt(np.mean(np.abs(r.reshape(case.M, -1)) ** 2, axis=1))
        tol = BOUND_K * unit(dt, P, Q) * (rms(reference(case, xs, k)) + abs(a) * rms(reference(case, x, k)) + rms(reference(case, x2, k)))
        d = np.max(np.abs(y12.astype(np.complex128) - (np.complex128(a) * y.astype(np.complex128) + y2.astype(np.complex128))).reshape(case.M, -1), axis=1)
        print("linearity %s: %s of the bound" % (case, np.round(d / tol, 4)))
        assert np.all(d <= tol), (case, d, tol)


def check_two_executes(run_plan, dtype, no_fusion=False):
    """Two executes of one plan with different data: the second result is that of a fresh plan on the second data, bit for bit."""
    dt = np.dtype(dtype)
    case = Case("two", 15, 9, 2, 8, mode=SAME)
    k = kernel(case, dt)
    xa, xb = images(case, dt, seed=7), images(case, dt, seed=8)
    _, y2, _ = run_once(run_plan, case, dt, xa, k, x2=xb, no_fusion=no_fusion)
    yb, _, _ = run_once(run_plan, case, dt, xb, k, no_fusion=no_fusion)
    assert np.array_equal(y2.view(np.uint8), yb.view(np.uint8)), "the second execute differs from a fresh plan's"
    assert float(np.max(errors(y2, reference(case, xb, k)) / unit(dt, 16, 16))) <= BOUND_K


def check_largest_fused(run_plan, dtype):
    """The largest P the planner fuses, read from the plans themselves (CIRCULAR P x 8 images, P = 8, 16, ...): every P up to it reports the
    column round, the next power of two the fallback; both are checked against the reference."""
    dt = np.dtype(dtype)
    fused = {}
    for lp in range(3, 13):
        P = 1 << lp
        case = Case("P%d" % P, P, 8, 1, 1, mode=CIRCULAR, M=1, fused=None)
        _, _, info = run_once(run_plan, case, dt, images(case, dt), kernel(case, dt), contiguous=True)
        fused[P] = info["fused"]
        if not info["fused"]:
            break
    largest = max(P for P, f in fused.items() if f)
    print("largest fused P, %s: %d (%s)" % (dt.name, largest, fused))
    assert all(f for P, f in fused.items() if P <= largest) and fused.get(2 * largest) == 0, fused
    check(run_plan, Case("largest-P%d" % largest, largest, 8, 5, 3, mode=CIRCULAR, M=3, fused=True), dt)
    check(run_plan, Case("largest-P%d" % largest, largest, 8, 5, 3, mode=CIRCULAR, M=3, fused=True), dt, no_fusion=True)
    check(run_plan, Case("above-P%d" % (2 * largest), 2 * largest, 8, 5, 3, mode=CIRCULAR, M=1, fused=False), dt)
    return largest


def gaussian_mask_centred(rows, cols, sigma):
    """exp(-r^2 / (2 sigma^2)), r the distance from [rows/2][cols/2]: the reference's Gaussian mask in its centred (fft_shift_2d) layout"""
    i, j = np.meshgrid(np.arange(rows) - rows / 2.0, np.arange(cols) - cols / 2.0, indexing="ij")
    return np.exp(-(i * i + j * j) / (2.0 * sigma * sigma))


def check_spectrum(run_plan, dtype):
    """H = 1 returns x; the Gaussian mask (sigma = 4, 32 x 32, unshifted) against ifft2(fft2(x) H); both paths"""
    dt = np.dtype(dtype)
    case = Case("spectrum-32x32", 32, 32, 32, 32, mode=SPECTRUM)
    x = images(case, dt)
    for no_fusion in (False, True):
        y, _ = check(run_plan, case, dt, k=np.ones((32, 32), dtype=dt), no_fusion=no_fusion, label="spectrum identity %s %d" % (dt.name, no_fusion))
        e = errors(y, x.astype(np.complex128)) / unit(dt, 32, 32)
        assert float(np.max(e)) <= BOUND_K
        H = np.fft.ifftshift(gaussian_mask_centred(32, 32, 4.0)).astype(dt)
        check(run_plan, case, dt, k=H, no_fusion=no_fusion, label="spectrum gaussian %s %d" % (dt.name, no_fusion))
