"""2D, r2c and c2r plans with their 7-smooth lengths on the mixed-radix engine (FFT_GPU_ALGO_MIXED_RADIX through
fft_gpu_plan_2d_algo_hip / fft_gpu_plan_r2c_1d_algo_hip / fft_gpu_plan_c2r_1d_algo_hip, or AUTO under the smooth policy), on the
GPU, at the cases of tests/mixed_ext_ladder.py.

Every execute goes through accuracy.check_execute_io: guards around input and output, a NaN-filled output, the input unchanged,
every row bin by bin against float64, in place bit-equal to out of place.  Every case asserts its path through plan.info().
The bound is accuracy.py's K * u * log2(n) (2D: log2(rows * cols)), K = 8 as for the project's other Stockham schedules:

    family      K    worst e_b / (u log2 n), fp32 / fp64: on the MI355X (this file, FFT_ACCURACY_REPORT) | in the CPU emulation
    2d_mixed    8    1.39 (1009 x 90) / 1.44 (30 x 64)                | 1.21 (15 x 9) / 1.28 (101 x 90)
    r2c_mixed   8    1.23 (n = 1000) / 1.62 (n = 1000)                | 0.92 (n = 12) / 1.42 (n = 360)
    c2r_mixed   8    2.35 (n = 10) / 2.49 (n = 30)                    | 1.78 (n = 30) / 2.49 (n = 30)

Every family measures below 4 on the device, so K = 8 is at least twice the worst measured value (accuracy.py's rule).
"""
import numpy as np
import pytest

import accuracy as A
import ext_ladder as X
import mixed_ext_ladder as L

for _f in ("2d_mixed", "r2c_mixed", "c2r_mixed"):
    A.BOUND_K.setdefault(_f, 8)

pytestmark = pytest.mark.gpu

_ids = lambda v: None if isinstance(v, (str, dict)) and (isinstance(v, dict) or " " in v) else str(v)  # noqa: E731
INFO_FIELDS = ("n", "batch", "direction", "precision", "algo", "device", "bluestein_m", "n_passes", "chunk_batch", "workspace_bytes",
               "team_tiles", "fused", "team_kernel")


def _info_tuple(info):
    return tuple(getattr(info, f) for f in INFO_FIELDS) + (tuple(info.factors),)


def _run_ptr(plan):
    def run(d_in, _, d_out):
        plan.execute_ptr(d_in, d_out)
        assert plan.sync() == 0
    return run


def _check_rows_engine(info, length, why):
    """algo / bluestein_m of a plan describe the row transforms (2D) or the complex core (real plans)."""
    eng = L.engine(length)
    if eng == L.MIXED:
        assert info.algo == 7 and info.bluestein_m == 0, (why, info.algo, info.bluestein_m)
    elif eng == L.POW2:
        assert info.algo != 7 and info.bluestein_m == 0, (why, info.algo, info.bluestein_m)
    else:
        assert info.algo != 7 and info.bluestein_m > 0, (why, info.algo, info.bluestein_m)


@pytest.mark.parametrize("dtype", [L.C64, L.C128], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rows,cols,nm,path,colk,why", L.GPU_2D, ids=_ids)
def test_2d_every_matrix_every_path(gpu_lib, rows, cols, nm, path, colk, why, dtype):
    """What plan.info() can show of a 2D plan is asserted: the engine of the rows (algo / bluestein_m), the column path (n_passes,
    factors) and the workspace.  The struct has no word for the engine of the transposed-image columns, so on the device a
    mixed-radix colt and a chirp-z one report alike; where cols is a power of two (360 x 64, 1000 x 64, 30 x 64) the info is the
    parent plan's, and the case checks the result only.  The engine of colt is asserted in the emulation
    (tests/test_emulated_mixed_ext.py, info[2] / info[3]), which runs the same planner source; only the two-pass colt (4200 x 6) shows
    here, through its scratch image in workspace_bytes."""
    import fftlib
    x = X.complex_rows(rows * cols, nm, dtype, seed=rows + cols)
    for d in (-1, 1):
        plan = fftlib.ExtPlan.fft2d(rows, cols, nm, d, dtype, algo=fftlib.ALGO_MIXED_RADIX)
        try:
            info = plan.info()
            _check_rows_engine(info, cols, why)
            assert info.n_passes == {L.DIRECT: 1, L.STRIDED: 2, L.TRANSPOSE: 0, L.ROWS: 0}[path], (why, info.n_passes)
            if path == L.DIRECT:
                assert list(info.factors) == [rows, 0, 0, 0], (why, list(info.factors))
            if path == L.TRANSPOSE:
                need = x.nbytes  # the transposed image, and the scratch image of a two-pass mixed-radix core
                if colk == L.MIXED and rows > L.MAX_L:
                    need += rows * x.dtype.itemsize
                assert info.workspace_bytes >= need, (why, info.workspace_bytes)
            A.check_execute_io(_run_ptr(plan), x, rows * cols, dtype, "2d_mixed", X.ref_2d(rows, cols, d), n=rows * cols, inplace=True,
                               label="2D %d x %d x %d dir %+d (%s)" % (rows, cols, nm, d, why))
        finally:
            plan.destroy()


@pytest.mark.parametrize("dtype", [L.F32, L.F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n,batch,policy,eng,passes,why", L.GPU_REAL, ids=_ids)
def test_r2c_c2r_every_row(gpu_lib, n, batch, policy, eng, passes, why, dtype):
    """r2c: every row against rfft of the float64 input.  c2r: every row against irfft of the r2c result and (small cases) of random
    Hermitian half spectra.  In place through one buffer of batch * (n/2 + 1) complex values."""
    import fftlib
    cdt = L.C64 if dtype == L.F32 else L.C128
    hb = n // 2 + 1
    core = n // 2 if n % 2 == 0 else n
    x = X.real_rows(n, batch, dtype, seed=n)
    try:
        if policy:
            fftlib.set_policy(**policy)
        fwd = fftlib.ExtPlan.r2c(n, batch, dtype, algo=fftlib.ALGO_MIXED_RADIX)
        inv = fftlib.ExtPlan.c2r(n, batch, dtype, algo=fftlib.ALGO_MIXED_RADIX)
    finally:
        fftlib.set_policy(team=1, min_batch=0, chunk_mb=0)
    try:
        for plan in (fwd, inv):
            info = plan.info()
            assert L.engine(core) == eng, why
            _check_rows_engine(info, core, why)
            assert info.fused == 0, why  # the split / merge runs as a kernel of its own
            if eng == L.MIXED:
                f = list(info.factors)
                assert info.n_passes == passes, (why, info.n_passes)
                assert (f[0] == core) if passes == 1 else (f[0] * f[1] == core and max(f[:2]) <= L.MAX_L), (why, f)
                if passes == 2:
                    assert info.workspace_bytes >= core * cdt.itemsize, why
                if "chunk_mb" in policy:
                    assert info.chunk_batch == max(1, (policy["chunk_mb"] << 20) // (core * cdt.itemsize)) < batch, (why, info.chunk_batch)
        fam = ("r2c_mixed", "c2r_mixed") if eng == L.MIXED else ("r2c", "c2r")
        label = "n=%d batch=%d %s (%s)" % (n, batch, dtype, why)
        S = {}

        def run_r2c(d_in, _, d_out):
            fwd.execute_ptr(d_in, d_out)
            assert fwd.sync() == 0
            if d_in != d_out:
                S["dev"] = A.d2h(d_out, (batch, hb), cdt)

        A.check_execute_io(run_r2c, x, hb, cdt, fam[0], X.ref_r2c, n=n, inplace=True, label="r2c " + label)
        if n in (12, 30):  # the pairs k = 0 and 2k = h of the split
            assert np.all(S["dev"][:, 0].imag == 0) and np.all(S["dev"][:, -1].imag == 0)
            ref = np.fft.rfft(x.astype(np.float64), axis=1)
            for k in (0, n // 2) + ((n // 4,) if n % 4 == 0 else ()):
                assert np.max(np.abs(S["dev"][:, k] - ref[:, k])) <= A.bound(fam[0], cdt, n) * np.sqrt(np.mean(np.abs(ref) ** 2)), (why, k)
        spectra = [S["dev"]]
        if S["dev"].nbytes <= 16 << 20:
            spectra.append(X.half_spectra(n, batch, cdt, seed=n + 1))
        for H in spectra:
            A.check_execute_io(_run_ptr(inv), H, n, dtype, fam[1], X.ref_c2r(n), n=n, inplace=True, label="c2r " + label)
    finally:
        fwd.destroy()
        inv.destroy()


def test_algo_entry_points_reject_other_algorithms(gpu_lib):
    lib = gpu_lib
    for algo in (1, 2, 3, 4, 5, 6, 8, -1):
        assert lib.fft_gpu_plan_2d_algo_hip(6, 10, 1, -1, 1, algo) is None, algo
        assert lib.fft_gpu_plan_2d_algo(6, 10, 1, -1, 1, algo) is None, algo
        assert lib.fft_gpu_plan_r2c_1d_algo_hip(12, 1, 1, algo) is None, algo
        assert lib.fft_gpu_plan_c2r_1d_algo_hip(12, 1, 1, algo) is None, algo
    for algo in (0, 7):
        for h in (lib.fft_gpu_plan_2d_algo_hip(6, 10, 1, -1, 1, algo), lib.fft_gpu_plan_2d_algo(6, 10, 1, -1, 1, algo),
                  lib.fft_gpu_plan_r2c_1d_algo_hip(12, 1, 1, algo), lib.fft_gpu_plan_c2r_1d_algo_hip(12, 1, 1, algo)):
            assert h
            lib.fft_gpu_destroy_plan(h)


def test_policy_decides_what_auto_builds(gpu_lib):
    """Policy 0 and AUTO: the plan the entry points without an algorithm build, field by field, chirp-z.  Policy 1: algorithm 7."""
    import fftlib
    lib = gpu_lib

    def makers():
        return (("2D 1080 x 1920", lambda a: fftlib.ExtPlan.fft2d(1080, 1920, 1, -1, L.C64, algo=a),
                 lambda: fftlib.ExtPlan(lib.fft_gpu_plan_2d_ex_hip(1080, 1920, 1, -1, fftlib.PREC_F32))),
                ("r2c 1000", lambda a: fftlib.ExtPlan.r2c(1000, 4, L.F32, algo=a),
                 lambda: fftlib.ExtPlan(lib.fft_gpu_plan_r2c_1d_hip(1000, 4, fftlib.PREC_F32))),
                ("r2c 44100", lambda a: fftlib.ExtPlan.r2c(44100, 2, L.F32, algo=a),
                 lambda: fftlib.ExtPlan(lib.fft_gpu_plan_r2c_1d_hip(44100, 2, fftlib.PREC_F32))))

    assert fftlib.set_smooth_policy(-1) == 0
    try:
        for what, with_algo, plain in makers():
            a, b = with_algo(fftlib.ALGO_AUTO), plain()
            try:
                assert _info_tuple(a.info()) == _info_tuple(b.info()), what
                assert a.info().bluestein_m != 0 and a.info().algo != 7, what
            finally:
                a.destroy()
                b.destroy()
        assert fftlib.set_smooth_policy(1) == 1
        for what, with_algo, plain in makers():
            for p in (with_algo(fftlib.ALGO_AUTO), plain()):
                try:
                    assert p.info().algo == 7 and p.info().bluestein_m == 0, what
                finally:
                    p.destroy()
        x = X.real_rows(1000, 4, L.F32, seed=2)  # and the plan AUTO builds under the policy computes the transform
        S = fftlib.rfft(x)
        e, k = A.row_errors(S, X.ref_r2c(x))
        A.assert_within(e, k, A.bound("r2c_mixed", L.C64, 1000), "rfft under the smooth policy")
    finally:
        assert fftlib.set_smooth_policy(0) == 0
    p = fftlib.ExtPlan.r2c(1000, 1, L.F32)
    try:
        assert p.info().bluestein_m != 0 and p.info().algo != 7
    finally:
        p.destroy()


@pytest.mark.parametrize("dtype", [L.F32, L.F64], ids=["fp32", "fp64"])
def test_helpers_agree_with_numpy(gpu_lib, dtype):
    import fftlib
    cdt = L.C64 if dtype == L.F32 else L.C128
    for n in (1000, 945):
        x = X.real_rows(n, 3, dtype, seed=n)
        S = fftlib.rfft(x, algo=fftlib.ALGO_MIXED_RADIX)
        e, k = A.row_errors(S, np.fft.rfft(x.astype(np.float64), axis=1))
        A.assert_within(e, k, A.bound("r2c_mixed", cdt, n), "rfft n=%d" % n)
        back = fftlib.irfft(S, n, algo=fftlib.ALGO_MIXED_RADIX)
        e, k = A.row_errors(back, np.fft.irfft(S.astype(np.complex128), n, axis=1))
        A.assert_within(e, k, A.bound("c2r_mixed", dtype, n), "irfft n=%d" % n)
    m = X.complex_rows(360 * 100, 2, cdt, seed=9).reshape(2, 360, 100)
    for d in (-1, 1):
        y = fftlib.fft2d(m, d, algo=fftlib.ALGO_MIXED_RADIX)
        ref = np.fft.fft2(m.astype(np.complex128)) if d < 0 else np.fft.ifft2(m.astype(np.complex128))
        e, k = A.row_errors(y.reshape(2, -1), ref.reshape(2, -1))
        A.assert_within(e, k, A.bound("2d_mixed", cdt, 360 * 100), "fft2d 360 x 100 dir %+d" % d)
