"""Every transform path as a linear operator: the cases, inputs and closed-form references that tests/test_emulated_operator.py (CPU
emulation) and tests/test_gpu_operator.py (device) share.  Test infrastructure only.

A. The DFT matrix, column by column.  Row i of a batch is the unit impulse at sample js[i]; its transform is column js[i] of the
   matrix, exp(-+2 pi i ((j k) mod n) / n) (inverse: / n), every bin of magnitude 1 (1 / n).  On a random row an error d in one
   matrix element reaches the result as d / sqrt(n) of the row's RMS; on the impulse the per-bin error IS the twiddle error.  The
   reference is the closed form (unit()), never an FFT: the product j k is reduced mod n in int64, the angle is reduced to
   [-pi/4, pi/4] around the nearest multiple of pi/2 and the quadrant applied exactly, so the float64 value is good to ~2 u.  For
   fp64 results closed_form_checked() compares the first rows with the same form in long double (pi = 4 atan(1)) and asserts the
   float64 one within a quarter of the bound.  Metric and bound are accuracy.py's: row_errors(), K u log2(n) of the path's family
   (accuracy.IMPULSE_K pins a family of its own where one is needed; none is).

B. check_neighbours / C. check_scaling, check_zeros (accuracy.py): exact conditions, at one size per path family.

MEASURED: the worst e / (u log2 n) (chirp-z: log2 m) over the impulse cases of tests/test_gpu_operator.py on the MI355X, fp32 / fp64,
as merged into profiles/operator_accuracy_report.json (keys "impulse:<family>") by a run with FFT_ACCURACY_REPORT.  accuracy.check_rows
prints each case's figure before it asserts.
"""
import numpy as np

import accuracy as A

A.BOUND_K.setdefault("mixed_radix", 8)  # the mixed-radix plan's K (tests/test_gpu_mixed_radix.py)

C64, C128 = np.dtype(np.complex64), np.dtype(np.complex128)
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BOTH = (C64, C128)

# family: (K of the impulse bound, worst e / (u log2 n) measured on the MI355X over tests/test_gpu_operator.py, fp32 / fp64, and the n of
# the worst case); every family is below K / 2, so none is marked "over K / 2 (open)" and accuracy.IMPULSE_K stays empty
MEASURED = {
    "multipass":     (8, "0.56 (4096) / 0.58 (4096)"),       # single pass, two and three passes up to 2^21
    "radix2_global": (8, "0.41 (1024) / 0.45 (1024)"),
    "radix2_shfl":   (8, "0.41 (1024) / 0.45 (1024)"),
    "wide_row":      (9, "2.26 (8192) / 0.34 (8192)"),
    "team_quad":     (8, "1.97 (2^20) / 1.30 (2^16)"),
    "team_defer":    (8, "  -         / 1.23 (2^18)"),       # no fp32 size runs it
    "mixed_radix":   (8, "0.81 (3375) / 0.86 (3375)"),
    "bluestein":     (32, "1.44 (1009) / 1.30 (1009)"),      # in units of u log2 m
    "r2c":           (8, "1.59 (1009) / 1.28 (1006)"),
    "c2r":           (8, "1.67 (1006) / 1.67 (1006)"),
    "2d":            (8, "0.76 (12 x 32) / 0.81 (30 x 90)"),
}

ALL_IMPULSES = 4096   # every j up to this n, sampled positions above
RANDOM_BELOW = 1 << 21  # the 8 random positions are dropped from this n on


def prime_factors(n):
    out = []
    for p in (2, 3, 5, 7):
        while n % p == 0:
            out.append(p)
            n //= p
    return out + ([n] if n > 1 else [])


def positions(n, factors=(), every=ALL_IMPULSES, seed=1):
    """The impulse positions of a transform of length n: every j for n <= 4096; else 0, 1, n - 1, n / 2; 2^t, 2^t - 1 and n - 2^t
    for every 2^t < n (each bit of j selects one table level); the partial products of `factors` (a mixed-radix plan's factor
    schedule) and each of them minus 1; 8 seeded random positions below n = 2^21."""
    if n <= every:
        return np.arange(n, dtype=np.int64)
    js = {0, 1, n - 1, n // 2}
    t = 1
    while t < n:
        js |= {t, t - 1, n - t}
        t *= 2
    p = 1
    for f in factors:
        p *= f
        if 1 < p < n:
            js |= {p, p - 1}
    if n < RANDOM_BELOW:
        js |= {int(j) for j in np.random.default_rng((seed, n)).integers(0, n, 8)}
    return np.array(sorted(j for j in js if 0 <= j < n), dtype=np.int64)


def unit(r, n, real=np.float64):
    """exp(+2 pi i r / n) for integer r in [0, n), in the precision `real` (float64 or longdouble)."""
    r = np.asarray(r, dtype=np.int64)
    s = (8 * r + n) // (2 * n)          # the nearest multiple of pi/2
    t = 4 * r - s * n                   # angle = s pi/2 + pi t / (2 n), |t| <= n/2
    a = (4 * np.arctan(real(1))) * t.astype(real) / real(2 * n)
    c, sn = np.cos(a), np.sin(a)
    q = s & 3
    re = np.where(q == 0, c, np.where(q == 1, -sn, np.where(q == 2, -c, sn)))
    im = np.where(q == 0, sn, np.where(q == 1, c, np.where(q == 2, -sn, -c)))
    return re + 1j * im


def column(n, js, direction, bins=None, real=np.float64):
    """Columns js of the DFT matrix of length n, [len(js)][bins] (default n): forward exp(-2 pi i j k / n), inverse exp(+...) / n."""
    js = np.asarray(js, dtype=np.int64).reshape(-1, 1)
    k = np.arange(bins or n, dtype=np.int64).reshape(1, -1)
    w = unit((js * k) % n, n, real)
    return np.conj(w) if direction < 0 else w / real(n)


def impulses(n, js, dtype):
    x = np.zeros((len(js), n), dtype=dtype)
    x[np.arange(len(js)), js] = 1
    return x


def where(xs):
    """The impulse position of every row (the references take it from the input rows, so they serve any slice of a batch)."""
    return np.argmax(np.abs(np.asarray(xs)), axis=-1)


def ref_1d(n, direction, real=np.float64):
    return lambda xs: column(n, where(xs), direction, real=real)


def ref_r2c(n, real=np.float64):
    return lambda xs: column(n, where(xs), -1, bins=n // 2 + 1, real=real)


def ref_c2r(n, real=np.float64):
    """One-hot Hermitian half spectra (value 1 at bin j <= n/2): 2 cos(2 pi j k / n) / n; bins 0 and n/2 are not doubled."""
    def ref(Xs):
        j = where(Xs)
        c = column(n, j, 1, real=real).real
        single = (j == 0) | (2 * j == n)
        return np.where(single[:, None], c, 2 * c)
    return ref


def ref_2d(rows, cols, direction, real=np.float64):
    def ref(xs):
        r, c = np.divmod(where(xs), cols)
        return (column(rows, r, direction, real=real)[:, :, None] * column(cols, c, direction, real=real)[:, None, :]).reshape(len(r), -1)
    return ref


def positions_2d(rows, cols):
    """Flat positions r * cols + c: every (r, c) if rows * cols <= 4096, else positions(rows) x positions(cols)."""
    if rows * cols <= ALL_IMPULSES:
        return np.arange(rows * cols, dtype=np.int64)
    return (positions(rows, every=64)[:, None] * cols + positions(cols, every=64)[None, :]).reshape(-1)


def positions_half(n, factors=()):
    """Positions of a one-hot half spectrum: those of positions(n) that are bins 0 ... n/2."""
    js = positions(n, factors)
    return js[js <= n // 2]


def closed_form_checked(ref64, ref_long, x, family, dtype, n, m=None, rows=3, label=""):
    """fp64 results: the float64 closed form of the first rows of x against the long-double one, within a quarter of the bound
    (what check_rows(long_rows=) shows for FFT references; that branch is skipped when ref= is given)."""
    if np.dtype(dtype) not in (C128, F64):
        return
    xs = x[:rows] if x.shape[0] <= 2 * rows else np.concatenate([x[:rows], x[x.shape[0] // 2:x.shape[0] // 2 + rows], x[-rows:]])
    e, k = A.row_errors(ref64(xs), ref_long(xs))
    A.assert_within(e, k, A.bound(family, dtype, n, m, "impulse") / 4, "float64 closed form vs long double, %s n=%d" % (label, n))


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
SINGLE_PASS_AUTO = tuple(1 << t for t in range(1, 13))                    # n = 2 ... 4096, every impulse
SINGLE_PASS_EXPLICIT = [(a, n) for a in ("radix2", "radix4", "split_radix", "radix2_global") for n in (64, 1024)] + \
                       [("radix2_shfl", 128), ("radix2_shfl", 1024)]
WIDE_ROW = [(8192, C64), (16384, C64), (8192, C128)]
MIXED_ALL = (6, 30, 210, 1000, 1080, 3375, 4050)                          # every impulse
MIXED_SAMPLED = (4200, 44100, 10 ** 6)                                    # 4200: the smallest two-pass length with a factor 7
CHIRPZ = (7, 1009, 2049, 100003)                                          # 1009: one kernel (fused == 3); 2049: m = 8192
REAL = (1024, 1000, 1009, 1006)                                           # 1000: the mixed core with algo = mixed_radix
TWO_D = [(32, 64, False), (12, 32, False), (30, 90, True)]                # (rows, cols, mixed); 12 x 32: transposed chirp-z columns
# every (log2 n, dtype) the device build has a team kernel for (csrc/fft_team_list.h FFT_QUAD_INSTANCES / FFT_TEAM_INSTANCES), forced as
# tests/test_gpu_every_transform.py forces them (policy team = 2): the planner then runs the quad kernel's default slot variant at
# every fp32 size and fp64 2^14 ... 2^16, and team_defer at fp64 2^17 ... 2^19.  The other slot variants of FFT_QUAD_INSTANCES and the
# fp32 rows of FFT_TEAM_INSTANCES (2^16 ... 2^20) are not reachable through the policy and are not run here.
TEAM = [(20, C64), (19, C64), (18, C64), (17, C64), (16, C64), (15, C64),
        (19, C128), (18, C128), (17, C128), (16, C128), (15, C128), (14, C128)]
# the emulation's multi-pass sizes: (n, lds_budget, passes), as tests/ext_ladder.py forces them
EMU_MULTIPASS = [(256, 4096, 2), (4096, 4096, 3)]
# The emulation runs one host thread per GPU thread (about 2 * 10^5 points a second on the power-of-two engine, 10^6 on the mixed-radix
# one, far less on the one-wavefront and team kernels): every impulse of a power-of-two n costs n^2 points per execute, 90 s at
# n = 4096.  The power-of-two paths run every impulse up to n = 256 and the sampled positions above; the mixed-radix lengths run every
# impulse at every all-impulse length, r2c / c2r at 1024 and 1000.
EMU_ALL_IMPULSES = 256


def chirpz_m(n):
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


def neighbour_batch(c):
    """Two full tiles of c transforms and a ragged one; the poisoned rows: the first and the last transform of a tile, the last of
    the batch (in the ragged tile)."""
    batch = 2 * c + max(1, c // 2) + (1 if c > 1 else 0)
    return batch, sorted({c, 2 * c - 1, batch - 1} if c > 1 else {1, batch - 1})


def normal_scaled(width, batch, dtype, seed):
    """Complex (or real) normal rows for the exact-condition checks."""
    dt = np.dtype(dtype)
    if dt in (F32, F64):
        cdt = C64 if dt == F32 else C128
        return np.ascontiguousarray(A.block_normal_rows((width + 1) // 2, 0, batch, cdt, seed).view(dt)[:, :width])
    return A.block_normal_rows(width, 0, batch, dt, seed)


def exact_conditions(run, x, poison_rows, label, degree=1, w_out=None, dtype_out=None, x2=None, out_rows=None, rows_out=None,
                     poisons=A.POISONS, scaling=True):
    """Parts B and C on one plan: every poison on `poison_rows`, the scaling property and the zero batch."""
    kw = dict(w_out=w_out, dtype_out=dtype_out, x2=x2, rows_out=rows_out, label=label)
    for poison in poisons:
        A.check_neighbours(run, x, poison_rows, poison, out_rows=out_rows, **kw)
        if x2 is not None:
            A.check_neighbours(run, x, poison_rows[:1], poison, poison_second=True, out_rows=out_rows, **kw)
    if scaling:
        A.check_scaling(run, x, degree=degree, **kw)
    A.check_zeros(run, x, **kw)
