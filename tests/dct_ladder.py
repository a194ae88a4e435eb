"""The cases at which the cosine / sine transform plans (csrc/fft_plans_ext.h DctPlan, Dct2DPlan; csrc/fft_kernels_dct.h) are checked
against float64 numpy, on the GPU (tests/test_gpu_dct.py) and in the CPU emulation (tests/test_emulated_dct.py), with the inputs, the
reference and the checkers both files share.  Test infrastructure only.

A backend is a pair of functions
    run_plan(n, batch, type, norm, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False) -> (rc, fused)
    run_plan2d(rows, cols, M, type, norm, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False) -> (rc, fused)
that build ONE plan, execute, wait and destroy the plan: rc 0 / -1 plan refused / -2 execute refused; fused 1 / 0.

Reference: float64 numpy only (scipy may be absent): the direct cosine / sine matrix of the definition for N <= 64, above that the 2N
even extension through numpy.fft.  Norms as scipy.fft's: NONE unscaled, INVERSE times 1 / (2N), ORTHO norm="ortho".
Error: per row max |y - ref| / RMS(ref), in units of u log2 N (u = 2^-24 / 2^-53; N = 1 counts log2 as 1); 2D: per image, log2(rows cols).
Bound: K = 8, the one the ext, frames and real2d ladders use for one transform.  Worst measured (profiles/dct_accuracy_report.json):
emulation 1.73 (fp32) / 1.69 (fp64) fused, 2.82 / 2.21 fallback; MI355X 1.87 / 2.52 fused, 4.03 (N = 8192 under NO_FUSION) / 2.42
fallback -- the fp32 fallback's worst is just above half the bound.
"""
import numpy as np

import accuracy as A
import filter_ladder as FL

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BOTH = (F32, F64)
DCT2, DCT3, DST2, DST3 = 0, 1, 2, 3
TYPES = (DCT2, DCT3, DST2, DST3)
TYPE_NAMES = {DCT2: "dct2", DCT3: "dct3", DST2: "dst2", DST3: "dst3"}
NONE, INVERSE, ORTHO = 0, 1, 2
NORMS = (NONE, INVERSE, ORTHO)
NORM_NAMES = {NONE: "none", INVERSE: "inverse", ORTHO: "ortho"}
LONGEST = {F32: 8192, F64: 4096}  # the longest rows whose half fits one hooked pass
SMALLEST = {F32: 16, F64: 8}      # the shortest fused rows: 64 bytes
BOUND_K = 8


class Case:
    """batch rows of n reals; ipad / opad: pitch - n on the input / output side; fused: True / False the path the plan must report, or a
    dict per dtype; norms: the norms the case runs at."""

    def __init__(self, name, n, batch=3, ipad=0, opad=0, fused=True, norms=(NONE,), inplace=False, dtypes=BOTH, why=""):
        self.name, self.n, self.batch, self.ipad, self.opad, self.fused, self.norms = name, n, batch, ipad, opad, fused, norms
        self.inplace, self.dtypes, self.why = inplace, dtypes, why

    def __repr__(self):
        return self.name

    def expect_fused(self, dtype):
        f = self.fused
        return f[np.dtype(dtype)] if isinstance(f, dict) else f


FUSED = [
    Case("n16", 16, norms=NORMS, why="the smallest fused length in fp32"),
    Case("n8", 8, fused={F32: False, F64: True}, norms=NORMS, why="32-byte rows in fp32: the fallback; the smallest fused length in fp64"),
    Case("n32", 32, norms=NORMS, why="the pair k, L - k crosses threads"),
    Case("n64", 64, why="the pair k, L - k crosses threads"),
    Case("n1024", 1024, batch=3),
    Case("n8192-longest", 8192, batch=2, dtypes=(F32,), why="the longest fused rows, fp32"),
    Case("n4096-longest", 4096, batch=2, dtypes=(F64,), why="the longest fused rows, fp64"),
    Case("n64-batch1", 64, batch=1, why="one live row, the rest of the tile is padding"),
    Case("n16-batch129", 16, batch=129, why="one tile's worth of rows plus one: the emulation's fp64 tile at N = 16 is 128 rows"),
    Case("n16-batch257", 16, batch=257, why="... its fp32 tile 256 rows"),
    Case("n16-batch1025", 16, batch=1025, why="... and no tile of the rows kernel holds more than 1024 rows (1024 threads): one row in the last tile"),
    Case("n64-odd-pitches", 64, ipad=3, opad=5, why="rows only element-aligned: component accesses"),
    Case("n64-aligned-pitches", 64, ipad=4, opad=8, why="pitches that keep every row 16-byte aligned"),
    Case("n64-inplace", 64, inplace=True, why="d_in == d_out"),
    Case("n64-inplace-pitch", 64, ipad=3, opad=3, inplace=True, why="d_in == d_out at an odd pitch"),
]
FALLBACK = (
    [Case("n%d" % n, n, fused=False, norms=NORMS if n == 12 else (NONE,), why="N = %d" % n) for n in (1, 2, 3, 4, 9, 12, 1000)]
    + [Case("n16384-above", 16384, batch=2, fused=False, dtypes=(F32,), why="twice the longest fused length, fp32"),
       Case("n8192-above", 8192, batch=2, fused=False, dtypes=(F64,), why="twice the longest fused length, fp64"),
       Case("n9-odd-pitches", 9, ipad=1, opad=2, fused=False),
       Case("n12-inplace", 12, inplace=True, fused=False)]
)


class Case2D:
    def __init__(self, name, rows, cols, M=3, ipad=0, opad=0):
        self.name, self.rows, self.cols, self.M, self.ipad, self.opad = name, rows, cols, M, ipad, opad

    def __repr__(self):
        return self.name


CASES_2D = [Case2D("8x16", 8, 16), Case2D("16x8", 16, 8), Case2D("5x9", 5, 9), Case2D("1x1", 1, 1), Case2D("64x64-padded", 64, 64, M=3, ipad=5, opad=3)]


# ---- the reference
def _matrix(n, type):
    """[n_out][n_in] long double: the definition's sums (unnormalised).  The integer in the angle is reduced mod 4n first, so that the
    angle stays below 2 pi and the matrix is good to the long double's rounding: the reference's own error stays far below u."""
    k = np.arange(n)[:, None]
    m = np.arange(n)[None, :]
    step = np.arctan(np.longdouble(1)) * 4 / (2 * np.longdouble(n))  # pi / 2n in long double

    def ang(q):
        return (q % (4 * n)).astype(np.longdouble) * step

    if type == DCT2:
        return 2 * np.cos(ang(k * (2 * m + 1)))
    if type == DST2:
        return 2 * np.sin(ang((k + 1) * (2 * m + 1)))
    # type III: rows = n (output sample), columns = k (input coefficient)
    nn, kk = k, m
    if type == DCT3:
        M = 2 * np.cos(ang(kk * (2 * nn + 1)))
        M[:, 0] = 1
        return M
    M = 2 * np.sin(ang((2 * nn + 1) * (kk + 1)))
    M[:, n - 1] = (-1.0) ** np.arange(n)
    return M


def _dct2_ext(x):
    """unnormalised DCT-II of float64 rows through the 2N even extension"""
    n = x.shape[-1]
    Y = np.fft.fft(np.concatenate([x, x[..., ::-1]], axis=-1), axis=-1)[..., :n]
    return np.real(Y * np.exp(-1j * np.pi * np.arange(n) / (2.0 * n)))


def _dct3_ext(X):
    """unnormalised DCT-III of float64 rows: y[n] = Re sum_{k < 2N} c_k e^(i pi k / 2N) e^(2 pi i k n / 2N), c_0 = X[0], c_k = 2 X[k], 0 beyond N"""
    n = X.shape[-1]
    c = np.zeros(X.shape[:-1] + (2 * n,), dtype=np.complex128)
    c[..., :n] = 2.0 * X * np.exp(1j * np.pi * np.arange(n) / (2.0 * n))
    c[..., 0] = X[..., 0]
    return np.real(np.fft.ifft(c, axis=-1)[..., :n]) * (2 * n)


def _unnormalised(x, type):
    n = x.shape[-1]
    if n <= 64:
        return (x.astype(np.longdouble) @ _matrix(n, type).T).astype(np.float64)
    sign = (-1.0) ** np.arange(n)
    if type == DCT2:
        return _dct2_ext(x)
    if type == DST2:
        return _dct2_ext(x * sign)[..., ::-1]
    if type == DCT3:
        return _dct3_ext(x)
    return _dct3_ext(x[..., ::-1]) * sign


def reference(x, type, norm):
    """float64 transform of the rows of x (last axis), scipy's conventions"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    if norm == NONE:
        return _unnormalised(x, type)
    if norm == INVERSE:
        return _unnormalised(x, type) / (2.0 * n)
    odd = 0 if type in (DCT2, DCT3) else n - 1
    if type in (DCT2, DST2):
        y = _unnormalised(x, type) / np.sqrt(2.0 * n)
        y[..., odd] /= np.sqrt(2.0)
        return y
    xs = x / np.sqrt(2.0 * n)
    xs[..., odd] *= np.sqrt(2.0)
    return _unnormalised(xs, type)


def reference2d(x, type, norm):
    return np.swapaxes(reference(np.swapaxes(reference(x, type, norm), -1, -2), type, norm), -1, -2)


def rows_of(case, dtype, seed=11):
    rng = np.random.default_rng((seed, case.n, case.batch))
    return rng.standard_normal((case.batch, case.n)).astype(dtype)


def unit(dtype, n):
    return A.U[np.dtype(dtype)] * max(1.0, np.log2(n))


errors = FL.errors


# ---- one plan on guarded buffers
def run_once(run_plan, case, dtype, type, norm, x, no_fusion=False):
    """One plan on guarded, NaN-gapped buffers.  Returns (result [batch][n], fused); asserts rc, guards, gaps and, out of place, the input."""
    dt = np.dtype(dtype)
    n, B = case.n, case.batch
    fi = FL.Flat(B, n, n + case.ipad, dt)
    fo = fi if case.inplace else FL.Flat(B, n, n + case.opad, dt)
    try:
        flat = np.ascontiguousarray(x.reshape(B, n)).astype(dt)
        if not case.inplace:
            fo.put(None)
        fi.put(flat)
        rc, fused = run_plan(n, B, type, norm, dt, fi.ptr, n + case.ipad if case.ipad else 0, fo.ptr, (n + case.opad if case.opad else 0) if not case.inplace
                             else (n + case.ipad if case.ipad else 0), no_fusion=no_fusion)
        assert rc == 0, (case, rc)
        y, ok = fo.get()
        assert ok, "%s: the execute wrote outside its rows" % case
        if not case.inplace:
            back, ok = fi.get()
            assert ok and np.array_equal(back.view(np.uint8), flat.view(np.uint8)), "%s: the execute changed its input" % case
        return y, fused
    finally:
        fi.free()
        if fo is not fi:
            fo.free()


def check(run_plan, case, dtype, type, norm=NONE, no_fusion=False, x=None, report=True):
    """Every row within BOUND_K u log2 N of the float64 reference, nothing written outside the rows, the input untouched, the path as the
    case says.  Prints before it asserts."""
    dt = np.dtype(dtype)
    if x is None:
        x = rows_of(case, dt)
    ref = reference(x, type, norm)
    y, fused = run_once(run_plan, case, dt, type, norm, x, no_fusion=no_fusion)
    e = errors(y, ref) / unit(dt, case.n)
    label = "%s %s/%s %s%s" % (case, TYPE_NAMES[type], NORM_NAMES[norm], dt.name, " no_fusion" if no_fusion else "")
    print("%s: fused %d, worst e / (u log2 N) = %.3f (row %d)" % (label, fused, float(np.max(e)), int(np.argmax(e))))
    if report:
        A._note("dct_fused" if fused else "dct_fallback", dt, case.n, None, np.max(e), unit=1.0)
    assert fused == (0 if no_fusion else 1 if case.expect_fused(dt) else 0), (label, fused)
    assert float(np.max(e)) <= BOUND_K, "%s: %.3f u log2 N > %d" % (label, float(np.max(e)), BOUND_K)
    return y


def check_case(run_plan, case, dtype, type):
    """The case's norms on the plan's own path and under NO_FUSION; the two agree to rounding (twice the bound)."""
    dt = np.dtype(dtype)
    x = rows_of(case, dt)
    for norm in case.norms:
        y = check(run_plan, case, dt, type, norm, x=x)
        if case.expect_fused(dt):
            yf = check(run_plan, case, dt, type, norm, no_fusion=True, x=x)
            e = errors(y, yf.astype(np.float64)) / unit(dt, case.n)
            assert float(np.max(e)) <= 2 * BOUND_K, (case, e)


def check_2d(run_plan2d, case, dtype, type, norm=NONE, no_fusion=False):
    dt = np.dtype(dtype)
    rng = np.random.default_rng((5, case.rows, case.cols))
    x = rng.standard_normal((case.M, case.rows, case.cols)).astype(dt)
    ref = reference2d(x, type, norm).reshape(case.M, -1)
    nr = case.rows * case.cols
    fi = FL.Flat(case.M, nr, nr + case.ipad, dt)
    fo = FL.Flat(case.M, nr, nr + case.opad, dt)
    try:
        flat = np.ascontiguousarray(x.reshape(case.M, nr))
        fi.put(flat)
        fo.put(None)
        rc, fused = run_plan2d(case.rows, case.cols, case.M, type, norm, dt, fi.ptr, nr + case.ipad if case.ipad else 0, fo.ptr,
                               nr + case.opad if case.opad else 0, no_fusion=no_fusion)
        assert rc == 0, (case, rc)
        y, ok = fo.get()
        assert ok, "%s: the execute wrote outside its matrices" % case
        back, ok = fi.get()
        assert ok and np.array_equal(back.view(np.uint8), flat.view(np.uint8)), "%s: the execute changed its input" % case
    finally:
        fi.free()
        fo.free()
    e = errors(y, ref) / unit(dt, nr)
    print("%s 2D %s/%s %s%s: fused %d, worst e / (u log2 rows cols) = %.3f" % (case, TYPE_NAMES[type], NORM_NAMES[norm], dt.name, " no_fusion" if no_fusion else "",
                                                                             fused, float(np.max(e))))
    A._note("dct2d_fused" if fused else "dct2d_fallback", dt, nr, None, np.max(e), unit=1.0)
    both = all(v >= SMALLEST[dt] and v & (v - 1) == 0 for v in (case.rows, case.cols))
    assert fused == (1 if both and not no_fusion else 0), (case, fused)
    assert float(np.max(e)) <= BOUND_K, (case, e)


# ---- as a linear operator
def closed_form_column(n, type, at):
    """the transform of a unit impulse at `at`: column `at` of the definition's matrix, written out"""
    k = np.arange(n)
    step = np.arctan(np.longdouble(1)) * 4 / (2 * np.longdouble(n))  # pi / 2n; the integer in the angle is reduced mod 4n first

    def ang(q):
        return (q % (4 * n)).astype(np.longdouble) * step

    if type == DCT2:
        c = 2 * np.cos(ang(k * (2 * at + 1)))
    elif type == DST2:
        c = 2 * np.sin(ang((k + 1) * (2 * at + 1)))
    elif type == DCT3:
        c = np.ones(n) if at == 0 else 2 * np.cos(ang(at * (2 * k + 1)))
    else:
        c = (-1.0) ** k if at == n - 1 else 2 * np.sin(ang((2 * k + 1) * (at + 1)))
    return np.asarray(c, dtype=np.float64)


def check_impulses(run_plan, dtype, type, n=64, no_fusion=False):
    """A unit impulse at 0, at N - 1 and at one interior odd position, one per row, against the closed-form column; then a constant row."""
    dt = np.dtype(dtype)
    where = (0, n - 1, 5 if n > 5 else 1)
    case = Case("impulse-n%d" % n, n, batch=len(where) + 1)
    x = np.zeros((case.batch, n), dtype=dt)
    ref = np.empty((case.batch, n))
    for b, at in enumerate(where):
        x[b, at] = 1.0
        ref[b] = closed_form_column(n, type, at)
    x[-1] = 1.0
    ref[-1] = reference(x[-1:], type, NONE)[0]
    y, fused = run_once(run_plan, case, dt, type, NONE, x, no_fusion=no_fusion)
    d = np.max(np.abs(y.astype(np.float64) - ref), axis=1)
    e = d / np.sqrt(np.mean(ref ** 2, axis=1)) / unit(dt, n)
    print("impulses %s %s n = %d%s: %s" % (TYPE_NAMES[type], dt.name, n, " no_fusion" if no_fusion else "", np.round(e, 3)))
    assert float(np.max(e)) <= BOUND_K, e


def check_linear_operator(run_plan, dtype, type, n=64, no_fusion=False):
    """Zeros give exact zeros; scaling by 2 is exact; a NaN row leaves its neighbours bit-identical."""
    dt = np.dtype(dtype)
    case = Case("operator-n%d" % n, n, batch=3, ipad=1, opad=1)
    x = rows_of(case, dt)
    y, _ = run_once(run_plan, case, dt, type, ORTHO, x, no_fusion=no_fusion)
    xp = x.copy()
    xp[1] = np.nan
    yp, _ = run_once(run_plan, case, dt, type, ORTHO, xp, no_fusion=no_fusion)
    for b in (0, 2):
        assert np.array_equal(yp[b].view(np.uint8), y[b].view(np.uint8)), "row %d changed next to a NaN row" % b
    assert np.all(np.isnan(yp[1]))
    yz, _ = run_once(run_plan, case, dt, type, ORTHO, np.zeros_like(x), no_fusion=no_fusion)
    assert np.all(yz == 0), "zeros in, something else out"
    y2, _ = run_once(run_plan, case, dt, type, ORTHO, x * dt.type(2), no_fusion=no_fusion)
    assert np.array_equal(y2, y * dt.type(2)), "scaling by 2 is not exact"


def check_identities(run_plan, dtype, sine, n=64, no_fusion=False):
    """type III / INVERSE of type II / NONE is the identity (twice the bound); ORTHO preserves sum x^2 (to the bound, relative)."""
    dt = np.dtype(dtype)
    t2, t3 = (DST2, DST3) if sine else (DCT2, DCT3)
    case = Case("identity-n%d" % n, n, batch=3)
    x = rows_of(case, dt)
    X, _ = run_once(run_plan, case, dt, t2, NONE, x, no_fusion=no_fusion)
    back, _ = run_once(run_plan, case, dt, t3, INVERSE, X, no_fusion=no_fusion)
    e = errors(back, x.astype(np.float64)) / unit(dt, n)
    print("%s n = %d %s: III/INVERSE(II/NONE(x)) - x = %.3f u log2 N" % ("dst" if sine else "dct", n, dt.name, float(np.max(e))))
    assert float(np.max(e)) <= 2 * BOUND_K, e
    for t in (t2, t3):
        Y, _ = run_once(run_plan, case, dt, t, ORTHO, x, no_fusion=no_fusion)
        sx, sy = np.sum(x.astype(np.float64) ** 2, axis=1), np.sum(Y.astype(np.float64) ** 2, axis=1)
        e = np.abs(sy - sx) / sx / unit(dt, n)
        print("%s ortho n = %d %s: |sum y^2 - sum x^2| / sum x^2 = %s u log2 N" % (TYPE_NAMES[t], n, dt.name, np.round(e, 3)))
        assert float(np.max(e)) <= BOUND_K, e
