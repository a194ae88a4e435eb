"""The cases at which the real 2D transform plan (csrc/fft_plans_ext.h Real2DPlan; csrc/fft_kernels_real2d.h tile_fft_colpass_kernel,
real2d_copy_kernel) is checked against numpy, on the GPU (tests/test_gpu_real2d.py) and in the CPU emulation
(tests/test_emulated_real2d.py), with the inputs, the reference and the checkers both files share.  Test infrastructure only.

A backend is a function
    run_plan(rows, cols, n_matrices, inverse, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False, lds_budget=0, min_seg=0) -> (rc, info)
that builds ONE plan (dtype: the REAL dtype), executes, waits and destroys the plan: rc 0 / -1 plan refused / -2 execute refused;
info = dict(fused, n_passes, bins, tile_cols) (tile_cols: the emulation only, else 0).  lds_budget and min_seg exist in the emulation
only (the NARROW cases).

Reference: numpy.fft.rfft2 / numpy.fft.irfft2(X, s=(rows, cols)) in float64.
Error: per matrix max |y - ref| / RMS(ref), in units of u log2(rows cols) (u = 2^-24 / 2^-53; a single pixel counts log2 as 1).
Bound: K = 8, the one the ext and frames ladders use for one transform.  Worst measured (profiles/real2d_accuracy_report.json): emulation
1.14 (fp32) / 1.25 (fp64) fused, 1.64 / 1.85 fallback; MI355X 0.94 / 1.09 fused, 3.53 / 1.85 fallback -- none above half the bound.
"""
import numpy as np

import accuracy as A
import filter_ladder as FL

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BOTH = (F32, F64)
CDT = {F32: np.dtype(np.complex64), F64: np.dtype(np.complex128)}
V = {F32: 2, F64: 1}          # complex values per 16-byte lane access
LONGEST = {F32: 8192, F64: 4096}  # the longest rows whose half fits one hooked pass
BOUND_K = 8


class Case:
    """M images of rows x cols; ipad / opad: pitch - matrix size on the input / output side; fused: True / False the path the plan must
    report, a dict per dtype, or None (only what it reports is recorded)."""

    def __init__(self, name, rows, cols, M=3, ipad=0, opad=0, fused=True, lds_budget=0, min_seg=0, tile_cols=None, why=""):
        self.name, self.rows, self.cols, self.M, self.ipad, self.opad = name, rows, cols, M, ipad, opad
        self.fused, self.lds_budget, self.min_seg, self.tile_cols, self.why = fused, lds_budget, min_seg, tile_cols, why

    def __repr__(self):
        return self.name

    @property
    def bins(self):
        return self.cols // 2 + 1

    def expect_fused(self, dtype):
        f = self.fused
        return f[np.dtype(dtype)] if isinstance(f, dict) else f

    def with_(self, **kw):
        c = Case(self.name, self.rows, self.cols, self.M, self.ipad, self.opad, self.fused, self.lds_budget, self.min_seg, self.tile_cols, self.why)
        for a, b in kw.items():
            setattr(c, a, b)
        return c


# Fused needs rows >= 8 (E = 8 values per thread), cols a power of two >= 8 and tile rows of >= 64 bytes: cols/2 >= 8 (fp32) / 4 (fp64).
FUSED = [
    Case("8x16", 8, 16, why="the smallest fused shape in both precisions; P = 8: the stages need no LDS exchange"),
    Case("8x8", 8, 8, fused={F32: False, F64: True}, why="L = 4: 32-byte tile rows in fp32 (fallback), 64-byte rows in fp64"),
    Case("256x16", 256, 16, why="LDS exchanges in the column stages"),
    Case("8x512", 8, 512, why="many tiles per matrix, one live column in the last"),
    Case("8x16-odd-pitches", 8, 16, ipad=3, opad=5, why="odd pitches: the second real matrix is only 4-byte, the second spectral matrix only 8-byte aligned in fp32"),
    Case("16x32-pitches", 16, 32, ipad=4, opad=4, why="pitches that keep every matrix 16-byte aligned"),
]
FALLBACK = (
    [Case("%dx16" % r, r, 16, fused=False, why="rows = %d: below the smallest column tile" % r) for r in (1, 2, 4)]
    + [Case("8x%d" % c, 8, c, fused=False, why="cols = %d" % c) for c in (1, 2, 4)]
    + [Case("8x9", 8, 9, fused=False, why="odd cols: the row plan's promoted path"),
       Case("12x12", 12, 12, fused=False), Case("8x12", 8, 12, fused=False), Case("12x16", 12, 16, fused=False),
       Case("1x1", 1, 1, fused=False, why="a single pixel"),
       Case("5x9-odd-pitches", 5, 9, ipad=1, opad=1, fused=False, why="odd pitches on the fallback")]
)
# the emulation only: the LDS budget and the row-segment criterion narrow the column tile to C = V and C = 2 V columns at P = 64, cols = 64
NARROW = [Case("narrow-64x64-C%dV" % m, 64, 64, min_seg=16, lds_budget={F32: (2000, 3000), F64: (2500, 3500)}, tile_cols=m, why="C = %d V columns per tile" % m)
          for m in (1, 2)]


def images(case, dtype, seed=7):
    """[M][rows][cols] real normal values"""
    rng = np.random.default_rng((seed, case.rows, case.cols))
    return rng.standard_normal((case.M, case.rows, case.cols)).astype(dtype)


def spectra(case, dtype, seed=9):
    """[M][rows][bins] complex normal values: NOT Hermitian-consistent"""
    rng = np.random.default_rng((seed, case.rows, case.cols))
    s = (case.M, case.rows, case.bins)
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(CDT[np.dtype(dtype)])


def reference(case, a, inverse):
    if inverse:
        return np.fft.irfft2(a.astype(np.complex128), s=(case.rows, case.cols))
    return np.fft.rfft2(a.astype(np.float64))


def errors(y, ref):
    """max |y - ref| / RMS(ref) per matrix"""
    M = ref.shape[0]
    return FL.errors(y.reshape(M, -1), ref.reshape(M, -1))


def unit(dtype, case):
    return A.U[np.dtype(dtype)] * max(1.0, np.log2(case.rows * case.cols))


def run_once(run_plan, case, dtype, a, inverse, no_fusion=False):
    """One plan on guarded, NaN-gapped buffers.  Returns (result [M][rows][bins or cols], info); asserts rc, guards, gaps and the input."""
    dt = np.dtype(dtype)
    idt, odt = (CDT[dt], dt) if inverse else (dt, CDT[dt])
    nr, ns = case.rows * case.cols, case.rows * case.bins
    ni, no = (ns, nr) if inverse else (nr, ns)
    fi = FL.Flat(case.M, ni, ni + case.ipad, idt)
    fo = FL.Flat(case.M, no, no + case.opad, odt)
    lds = case.lds_budget
    if isinstance(lds, dict):
        lds = lds[dt][case.tile_cols - 1]
    try:
        flat = np.ascontiguousarray(a.reshape(case.M, ni))
        fi.put(flat)
        fo.put(None)
        rc, info = run_plan(case.rows, case.cols, case.M, inverse, dt, fi.ptr, ni + case.ipad if case.ipad else 0, fo.ptr, no + case.opad if case.opad else 0,
                            no_fusion=no_fusion, lds_budget=lds, min_seg=case.min_seg)
        assert rc == 0, (case, rc)
        assert info["bins"] == case.bins, (case, info)
        assert (info["fused"], info["n_passes"]) in ((1, 2), (0, 4 if case.rows > 1 else 1)), info
        y, ok = fo.get()
        assert ok, "%s: the execute wrote outside its matrices" % case
        back, ok = fi.get()
        assert ok and np.array_equal(back.view(np.uint8), flat.view(np.uint8)), "%s: the execute changed its input" % case
        return y.reshape((case.M, case.rows, case.cols if inverse else case.bins)), info
    finally:
        fi.free()
        fo.free()


def check(run_plan, case, dtype, inverse=False, no_fusion=False, a=None, label="", report=True):
    """One plan for `case`: every value of every matrix within BOUND_K u log2(rows cols) of numpy's, nothing written outside the matrices,
    the input untouched, the path as the case says.  Prints before it asserts."""
    dt = np.dtype(dtype)
    if a is None:
        a = spectra(case, dt) if inverse else images(case, dt)
    ref = reference(case, a, inverse)
    y, info = run_once(run_plan, case, dt, a, inverse, no_fusion=no_fusion)
    label = label or "%s %s %s%s" % (case, "irfft2" if inverse else "rfft2", dt.name, " no_fusion" if no_fusion else "")
    e = errors(y, ref) / unit(dt, case)
    print("%s: fused %d, passes %d, worst e / (u log2 rows cols) = %.3f (matrix %d)" % (label, info["fused"], info["n_passes"], float(np.max(e)), int(np.argmax(e))))
    if report:
        A._note("real2d_fused" if info["fused"] else "real2d_fallback", dt, case.rows * case.cols, None, np.max(e), unit=1.0)
    want = False if no_fusion else case.expect_fused(dt)
    if want is not None:
        assert info["fused"] == (1 if want else 0), (label, info)
    if case.tile_cols and not no_fusion:
        assert info["tile_cols"] == case.tile_cols * V[dt], (label, info)
    assert float(np.max(e)) <= BOUND_K, "%s: %.3f u log2(rows cols) > %d" % (label, float(np.max(e)), BOUND_K)
    return y, info


def check_case(run_plan, case, dtype):
    """Both directions (the inverse on spectra that are not Hermitian), the plan's own path and NO_FUSION, and the round trip."""
    dt = np.dtype(dtype)
    x = images(case, dt)
    for no_fusion in (False, True):
        X, _ = check(run_plan, case, dt, False, no_fusion, a=x)
        check(run_plan, case, dt, True, no_fusion)
        # the round trip through the device's own spectrum: irfft2(rfft2(x)) against x, two transforms -> twice the bound
        back, _ = run_once(run_plan, case.with_(ipad=case.opad, opad=case.ipad), dt, X, True, no_fusion=no_fusion)
        e = errors(back, x.astype(np.float64)) / unit(dt, case)
        print("%s %s%s: irfft2(rfft2(x)) - x = %.3f u log2(rows cols)" % (case, dt.name, " no_fusion" if no_fusion else "", float(np.max(e))))
        assert float(np.max(e)) <= 2 * BOUND_K, (case, e)


def check_ignored_imaginary_parts(run_plan, case, dtype, no_fusion=False):
    """Large imaginary parts in columns 0 and cols/2 of a non-Hermitian spectrum: the result is numpy's, which transforms those columns
    as they are and drops the imaginary parts of the ROW bins 0 and cols/2 only after the column transforms."""
    dt = np.dtype(dtype)
    X = spectra(case, dt)
    X[:, :, 0] += 1j * CDT[dt].type(1e3)
    X[:, :, -1] -= 1j * CDT[dt].type(3e3)
    ref = reference(case, X, True)
    y, info = run_once(run_plan, case, dt, X, True, no_fusion=no_fusion)
    # the error of the column transforms scales with what they transform (the large imaginary parts included), not with what is left
    # after the c2r has dropped them: the unit is the RMS of the column-transformed spectrum, per matrix
    col = np.fft.ifft(X.astype(np.complex128), axis=1)
    scale = np.sqrt(np.mean(np.abs(col) ** 2, axis=(1, 2)))
    d = np.max(np.abs(y.astype(np.float64) - ref).reshape(case.M, -1), axis=1)
    e = d / scale / unit(dt, case)
    print("%s %s%s: large Im in columns 0 and cols/2: %.3f" % (case, dt.name, " no_fusion" if no_fusion else "", float(np.max(e))))
    assert info["fused"] == (0 if no_fusion else 1 if case.expect_fused(dt) else 0)
    assert float(np.max(e)) <= BOUND_K, e


def check_impulses(run_plan, dtype, no_fusion=False):
    """A unit impulse at each corner and at one interior pixel of an 8 x 16 image, one per matrix, against the closed form
    X[k][c] = exp(-2 pi i (k i / rows + c j / cols))."""
    dt = np.dtype(dtype)
    where = ((0, 0), (0, 15), (7, 0), (7, 15), (3, 5))
    case = Case("impulse-8x16", 8, 16, M=len(where))
    x = np.zeros((case.M, 8, 16), dtype=dt)
    k, c = np.meshgrid(np.arange(8), np.arange(9), indexing="ij")
    ref = np.empty((case.M, 8, 9), dtype=np.complex128)
    for m, (i, j) in enumerate(where):
        x[m, i, j] = 1.0
        ref[m] = np.exp(-2j * np.pi * ((k * i % 8) / 8.0 + (c * j % 16) / 16.0))
    y, info = run_once(run_plan, case, dt, x, False, no_fusion=no_fusion)
    e = errors(y, ref) / unit(dt, case)
    print("impulses %s%s: %s" % (dt.name, " no_fusion" if no_fusion else "", np.round(e, 3)))
    assert info["fused"] == (0 if no_fusion else 1) and float(np.max(e)) <= BOUND_K, e
    assert np.array_equal(y[0], np.ones((8, 9), dtype=CDT[dt])), "an impulse at the origin: every bin is exactly 1"


def check_linear_operator(run_plan, dtype, inverse, no_fusion=False):
    """Zeros give exact zeros; scaling by a power of two is exact; a NaN / Inf matrix leaves its neighbours bit-identical."""
    dt = np.dtype(dtype)
    for case in (Case("operator-8x16", 8, 16, ipad=1, opad=1), Case("operator-16x32", 16, 32)):
        a = spectra(case, dt) if inverse else images(case, dt)
        y, info = run_once(run_plan, case, dt, a, inverse, no_fusion=no_fusion)
        assert info["fused"] == (0 if no_fusion else 1)
        for poison in (np.nan, np.inf):
            ap = a.copy()
            ap[1] = poison
            yp, _ = run_once(run_plan, case, dt, ap, inverse, no_fusion=no_fusion)
            for m in (0, 2):
                assert np.array_equal(yp[m].view(np.uint8), y[m].view(np.uint8)), "matrix %d changed next to a poisoned one (%s)" % (m, case)
            assert not np.all(np.isfinite(yp[1]))
        yz, _ = run_once(run_plan, case, dt, np.zeros_like(a), inverse, no_fusion=no_fusion)
        assert np.all(yz == 0), "zeros in, something else out (%s)" % case
        for s in (3, -5):
            ys, _ = run_once(run_plan, case, dt, a * a.dtype.type(2.0 ** s), inverse, no_fusion=no_fusion)
            assert np.array_equal(ys, y * y.dtype.type(2.0 ** s)), "scaling by 2^%d is not exact (%s)" % (s, case)


def check_largest_fused(run_plan, dtype):
    """The largest P the plan fuses, read from the plans themselves (P x 16 images, P = 8, 16, ...): every P up to it reports the fused
    path, twice that the fallback; both are checked in both directions."""
    dt = np.dtype(dtype)
    fused = {}
    for lp in range(3, 14):
        P = 1 << lp
        case = Case("P%d" % P, P, 16, M=1, fused=None)
        _, info = run_once(run_plan, case, dt, images(case, dt), False)
        fused[P] = info["fused"]
        if not info["fused"]:
            break
    largest = max(P for P, f in fused.items() if f)
    print("largest fused P, %s: %d (%s)" % (dt.name, largest, fused))
    assert all(f for P, f in fused.items() if P <= largest) and fused.get(2 * largest) == 0, fused
    for inverse in (False, True):
        check(run_plan, Case("largest-%dx16" % largest, largest, 16, fused=True), dt, inverse)
        check(run_plan, Case("largest-%dx16" % largest, largest, 16, fused=True), dt, inverse, no_fusion=True)
        check(run_plan, Case("above-%dx16" % (2 * largest), 2 * largest, 16, M=1, fused=False), dt, inverse)
    return largest


def check_longest_rows(run_plan, dtype):
    """8 x LONGEST (M = 1): the longest fused rows; 8 x twice that: the fallback."""
    dt = np.dtype(dtype)
    n = LONGEST[dt]
    for inverse in (False, True):
        check(run_plan, Case("8x%d" % n, 8, n, M=1, fused=True), dt, inverse)
        check(run_plan, Case("8x%d" % (2 * n), 8, 2 * n, M=1, fused=False), dt, inverse)
