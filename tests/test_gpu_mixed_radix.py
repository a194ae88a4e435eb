"""The mixed-radix plan for 7-smooth lengths (FFT_GPU_ALGO_MIXED_RADIX; csrc/fft_mixed_radix.h, ffteng::MixedRadixPlan) on the GPU.

Every execute goes through accuracy.check_execute_streamed() or check_execute(): a guarded NaN-filled output, an unchanged
input, in-place bits equal to out-of-place bits, and every transform checked bin by bin against the float64 transform of the
input actually given.  The bound is accuracy.py's K * u * log2(n):

    family        K    worst e_b / (u log2 n) measured on the MI355X over this file (FFT_ACCURACY_REPORT)
    mixed_radix   8    fp32 2.83 (n = 15) / fp64 3.44 (n = 15)

K = 8 is the project's K for its Stockham schedules; accuracy.py's rule (K at least twice the worst measured value, never above
the power-of-two cap of 16) holds for it.
"""
import ctypes as C

import numpy as np
import pytest

import accuracy as A
import mixed_radix_ladder as L

A.BOUND_K.setdefault("mixed_radix", 8)

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
FAMILY = "mixed_radix"


def _expect(plan, n, passes):
    def check():
        info = plan.info()
        assert info.algo == 7, ("algo", info.algo)
        assert info.n_passes == passes, ("n_passes", info.n_passes, passes)
        assert info.bluestein_m == 0 and info.team_tiles == 0 and info.team_kernel == 0 and info.fused == 0, \
            (info.bluestein_m, info.team_tiles, info.team_kernel, info.fused)
        f = list(info.factors)
        if passes == 1:
            assert f[0] == n, f
        else:
            assert f[0] * f[1] == n and max(f[0], f[1]) <= 4096, f
    return check


def _run(n, batch, dtype, d, passes, seed=None):
    import fftlib
    dt = np.dtype(dtype)
    plan = fftlib.Plan(n, batch, d, dt, fftlib.ALGO_MIXED_RADIX)
    try:
        A.check_execute_streamed(plan, n, batch, dt, seed=(seed if seed is not None else 7 * n + batch % 991), family=FAMILY,
                                 expect=_expect(plan, n, passes), label="mixed_radix %s n=%d batch=%d dir=%+d" % (dt.name, n, batch, d),
                                 long_rows=1 if dt == C128 else 0)
        return plan.info()
    finally:
        plan.destroy()


# ---- 1. every single-pass size
@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("d", [-1, 1], ids=["fwd", "inv"])
def test_every_single_pass_size(gpu_lib, dtype, d):
    assert len(L.SINGLE_PASS) == 235
    for n in L.SINGLE_PASS:
        for batch in (1, 5):
            _run(n, batch, dtype, d, 1)


# ---- 2. the tile-shape ladder
@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("n", L.LADDER_SIZES)
def test_tile_shape_ladder(gpu_lib, n, dtype):
    for batch in L.ladder(n, dtype):
        for d in (-1, 1):
            _run(n, batch, dtype, d, 1)


# ---- 3. two passes
@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("n", L.TWO_PASS)
def test_two_pass(gpu_lib, n, dtype):
    for batch in (1, 3):
        for d in (-1, 1):
            _run(n, batch, dtype, d, 2)


def test_two_pass_in_launch_groups(gpu_lib):
    """n = 10^6 fp32 is 8 MB per transform: with 16 MiB per launch group five transforms take three groups."""
    import fftlib
    fftlib.set_policy(chunk_mb=16)
    info = _run(10 ** 6, 5, C64, -1, 2)
    assert info.chunk_batch == 2, info.chunk_batch
    info = _run(10 ** 6, 5, C64, 1, 2)
    assert info.chunk_batch == 2, info.chunk_batch


# ---- 4. one launch whose element offsets pass 2^31
def test_one_launch_past_2_31_elements(gpu_lib):
    n, dtype = 3000, C64
    batch = (1 << 31) // n + 5
    assert n * batch > (1 << 31)
    tot, av = C.c_size_t(), C.c_size_t()
    gpu_lib.fft_gpu_get_memory_info_hip(C.byref(tot), C.byref(av))
    need = 2 * (batch + 2) * n * 8 + (1 << 30)
    if av.value < need:
        pytest.skip("needs %.1f GiB of free device memory, %.1f GiB free" % (need / 2 ** 30, av.value / 2 ** 30))
    info = _run(n, batch, dtype, -1, 1, seed=31)
    assert info.chunk_batch == batch


# ---- 5. the new plan and chirp-z agree
@pytest.mark.parametrize("n", [1000, 44100, 10 ** 6])
@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
def test_agrees_with_chirp_z(gpu_lib, n, dtype):
    import fftlib
    x = A.normal_rows(n, 0, 2, dtype, seed=n)
    y = fftlib.fft(x, -1, algo=fftlib.ALGO_MIXED_RADIX, inplace=False)
    z = fftlib.fft(x, -1, algo=fftlib.ALGO_AUTO, inplace=False)
    m = 1 << int(np.ceil(np.log2(2 * n - 1)))
    e, k = A.row_errors(y, z.astype(np.complex128))
    A.assert_within(e, k, A.bound(FAMILY, dtype, n) + A.bound("bluestein", dtype, n, m), "mixed radix vs chirp-z n=%d" % n)


# ---- 6. fallbacks
@pytest.mark.parametrize("n", [1009, 4100])
def test_other_lengths_fall_back_to_chirp_z(gpu_lib, n):
    import fftlib
    m = 1 << int(np.ceil(np.log2(2 * n - 1)))
    for dtype in L.DTYPES:
        for d in (-1, 1):
            plan = fftlib.Plan(n, 3, d, dtype, fftlib.ALGO_MIXED_RADIX)
            try:
                assert plan.info().bluestein_m == m, plan.info().bluestein_m
                A.check_execute(plan, A.normal_rows(n, 0, 3, dtype, seed=n), "bluestein", m=m, label="fallback n=%d" % n)
            finally:
                plan.destroy()


def test_a_power_of_two_gets_autos_plan(gpu_lib):
    import fftlib
    for dtype in L.DTYPES:
        a = fftlib.Plan(1024, 4, -1, dtype, fftlib.ALGO_MIXED_RADIX)
        b = fftlib.Plan(1024, 4, -1, dtype, fftlib.ALGO_AUTO)
        try:
            ia, ib = a.info(), b.info()
            assert (ia.algo, ia.bluestein_m, ia.n_passes, list(ia.factors), ia.team_tiles) == \
                   (ib.algo, ib.bluestein_m, ib.n_passes, list(ib.factors), ib.team_tiles)
            A.check_execute(a, A.normal_rows(1024, 0, 4, dtype, seed=10), "multipass", label="pow2 with algo 7")
        finally:
            a.destroy()
            b.destroy()
    assert gpu_lib.fft_gpu_plan_1d_ex_hip(1000, 1, -1, 1, 8) is None


# ---- 7. policy
def test_smooth_policy(gpu_lib):
    import fftlib
    lib = gpu_lib
    assert fftlib.set_smooth_policy(-1) == 0
    lib.fft_auto_cleanup()  # fft_auto() keeps its plans: none made under the other policy may serve here, or later
    try:
        assert fftlib.set_smooth_policy(1) == 1 and fftlib.set_smooth_policy(-1) == 1
        plan = fftlib.Plan(1000, 4, -1, C64)
        try:
            info = plan.info()
            assert info.algo == 7 and info.bluestein_m == 0 and info.n_passes == 1, (info.algo, info.bluestein_m)
            A.check_execute(plan, A.normal_rows(1000, 0, 4, C64, seed=5), FAMILY, label="AUTO under the smooth policy")
        finally:
            plan.destroy()
        p7 = fftlib.Plan(1009, 1, -1, C64)  # not 7-smooth: chirp-z whatever the policy
        assert p7.info().bluestein_m == 2048
        p7.destroy()
        for n in (1000, 44100):
            x = A.normal_rows(n, 0, 1, C128, seed=n)[0]
            ref = A.fft_ref(x[None, :], -1)
            y = np.full(n, np.nan, dtype=C128)
            assert lib.fft_auto(x.ctypes.data, y.ctypes.data, n, -1) == 0
            e, k = A.row_errors(y[None, :], ref)
            A.assert_within(e, k, A.bound(FAMILY, C128, n), "fft_auto under the smooth policy n=%d" % n)
            y[:] = np.nan
            plan = lib.fft_plan_dft_1d(n, x.ctypes.data, y.ctypes.data, -1, 1)  # FFT_MEASURE
            assert plan
            assert lib.fft_plan_measured_algo(plan) in (0, 7), lib.fft_plan_measured_algo(plan)
            lib.fft_execute(plan)
            lib.fft_destroy_plan(plan)
            e, k = A.row_errors(y[None, :], ref)
            # (whichever candidate won: chirp-z has the wider bound)
            m = 1 << int(np.ceil(np.log2(2 * n - 1)))
            A.assert_within(e, k, A.bound("bluestein", C128, n, m), "fft_plan_dft_1d FFT_MEASURE n=%d" % n)
    finally:
        lib.fft_auto_cleanup()
        assert fftlib.set_smooth_policy(0) == 0
    plan = fftlib.Plan(1000, 1, -1, C64)
    try:
        assert plan.info().bluestein_m == 2048 and plan.info().algo != 7
    finally:
        plan.destroy()


# ---- 8. the host-array entry
def test_host_array_entry_round_trip(gpu_lib):
    lib = gpu_lib
    for n in (6, 10, 12, 15, 20, 24, 30, 35, 40, 42, 48, 60, 72, 84, 90, 100, 120, 144):
        x = A.normal_rows(n, 0, 1, C128, seed=n)[0]
        y = x.copy()
        assert lib.fft_mixed_radix_gpu(y.ctypes.data, n, -1) == 0
        e, k = A.row_errors(y[None, :], A.fft_ref(x[None, :], -1))
        A.assert_within(e, k, A.bound(FAMILY, C128, n), "fft_mixed_radix_gpu forward n=%d" % n)
        assert lib.fft_mixed_radix_gpu(y.ctypes.data, n, 1) == 0  # scaled by 1/n
        e, k = A.row_errors(y[None, :], x[None, :])
        A.assert_within(e, k, 2 * A.bound(FAMILY, C128, n), "fft_mixed_radix_gpu forward then inverse n=%d" % n)
