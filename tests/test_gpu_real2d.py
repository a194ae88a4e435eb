"""The real 2D transform plans (fft_gpu_plan_r2c_2d_hip / fft_gpu_plan_c2r_2d_hip) on the device, at the cases of tests/real2d_ladder.py:
every value of every matrix against numpy's rfft2 / irfft2 in float64, outputs between sentinel guards and gaps that must stay
bit-identical, NaN in every input gap; each case asserts through plan.info() which path ran, and runs FFT_GPU_OPT_NO_FUSION on the same
data.  Then the refusals, the host and the numpy front ends."""
import numpy as np
import pytest

import real2d_ladder as L

pytestmark = pytest.mark.gpu


def run_plan(rows, cols, n_matrices, inverse, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False, lds_budget=0, min_seg=0):
    import fftlib
    lib = fftlib.init()
    prec = fftlib.PREC_F32 if np.dtype(dtype) == L.F32 else fftlib.PREC_F64
    handle = (lib.fft_gpu_plan_c2r_2d_hip if inverse else lib.fft_gpu_plan_r2c_2d)(rows, cols, n_matrices, prec)
    if not handle:
        return -1, None
    plan = fftlib.ExtPlan(handle)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        pi = plan.info()
        info = dict(fused=pi.fused, n_passes=pi.n_passes, bins=lib.fft_gpu_real2d_bins_hip(handle), tile_cols=0)
        assert pi.n == cols and pi.batch == n_matrices and list(pi.factors)[:3] == [cols, rows, 0] and pi.direction == (1 if inverse else -1)
        assert lib.fft_gpu_real2d_bins(handle) == cols // 2 + 1
        if (lib.fft_gpu_execute_real2d if inverse else lib.fft_gpu_execute_real2d_hip)(handle, in_ptr, in_pitch, out_ptr, out_pitch) != 0:
            return -2, info
        assert plan.sync() == 0
        return 0, info
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.FUSED + L.FALLBACK, ids=repr)
def test_cases(gpu_lib, case, dt):
    """every shape of the ladder: both directions, the plan's path and FFT_GPU_OPT_NO_FUSION, the round trip"""
    L.check_case(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_largest_fused_and_twice_that(gpu_lib, dt):
    L.check_largest_fused(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_longest_rows(gpu_lib, dt):
    L.check_longest_rows(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_many_tiles_many_matrices(gpu_lib, dt):
    """256 x 512, 5 matrices: workgroups walk several tiles, tiles of different matrices in one workgroup"""
    case = L.Case("256x512", 256, 512, M=5, ipad=2, opad=3)
    for inverse in (False, True):
        L.check(run_plan, case, dt, inverse)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_ignored_imaginary_parts(gpu_lib, dt, no_fusion):
    L.check_ignored_imaginary_parts(run_plan, L.Case("8x16", 8, 16), dt, no_fusion)
    L.check_ignored_imaginary_parts(run_plan, L.Case("12x12", 12, 12, fused=False), dt, no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_impulses(gpu_lib, dt, no_fusion):
    L.check_impulses(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("inverse", (False, True), ids=["forward", "inverse"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_linear_operator(gpu_lib, dt, inverse, no_fusion):
    L.check_linear_operator(run_plan, dt, inverse, no_fusion=no_fusion)


def test_refusals(gpu_lib):
    """every NULL / -1 condition; nothing is launched"""
    import fftlib
    lib = gpu_lib
    P = fftlib.PREC_F32
    for args in ((0, 16, 1), (8, 0, 1), (8, 16, 0), (-8, 16, 1), (1 << 16, 1 << 15, 1)):
        for f in (lib.fft_gpu_plan_r2c_2d_hip, lib.fft_gpu_plan_c2r_2d_hip, lib.fft_gpu_plan_r2c_2d, lib.fft_gpu_plan_c2r_2d):
            assert f(*args, P) is None, args
    fwd = fftlib.ExtPlan.real2d(8, 16, 2, False, np.float32)
    inv = fftlib.ExtPlan.real2d(8, 16, 2, True, np.float32)
    assert fwd.bins == 9 and inv.bins == 9
    x = np.arange(2 * 140 + 2 * 2 * 80, dtype=np.float32)
    buf = fftlib.DeviceBuffer(x.nbytes)
    try:
        buf.upload(x)
        xp, Xp = buf.ptr, buf.ptr + 4 * 280
        f = lib.fft_gpu_execute_real2d_hip
        assert f(fwd.handle, xp, 127, Xp, 80) == -1 and f(fwd.handle, xp, 140, Xp, 71) == -1   # a pitch smaller than the matrix
        assert f(inv.handle, Xp, 71, xp, 140) == -1 and f(inv.handle, Xp, 80, xp, 127) == -1
        assert f(fwd.handle, xp, 140, xp, 80) == -1                                             # d_out == d_in
        assert f(fwd.handle, xp, 140, xp + 4 * 267, 80) == -1                                   # d_out starts on the last input value
        assert f(inv.handle, Xp, 80, Xp + 8, 140) == -1
        assert f(fwd.handle, None, 0, Xp, 0) == -1 and f(fwd.handle, xp, 0, None, 0) == -1 and f(None, xp, 0, Xp, 0) == -1
        assert lib.fft_gpu_execute_ptr_hip(fwd.handle, xp, Xp) == -1 and lib.fft_gpu_execute_ptr(inv.handle, Xp, xp) == -1  # not the real 2D execute
        one = fftlib.ExtPlan.r2c(16, 16, np.float32)
        assert f(one.handle, xp, 0, Xp, 0) == -1 and lib.fft_gpu_execute_real2d(one.handle, xp, 0, Xp, 0) == -1           # a 1D plan
        assert lib.fft_gpu_real2d_bins_hip(one.handle) == -1 and lib.fft_gpu_real2d_bins(None) == -1
        one.destroy()
        assert fwd.sync() == 0 and inv.sync() == 0
        assert np.array_equal(buf.download(x.shape, x.dtype).view(np.uint8), x.view(np.uint8))
    finally:
        buf.free()
        fwd.destroy()
        inv.destroy()


def test_host_front_ends(gpu_lib):
    """fft_rfft2_gpu / fft_irfft2_gpu on host pointers against numpy, and their refusals"""
    for rows, cols in ((16, 32), (12, 9)):
        case = L.Case("host", rows, cols, M=1)
        x = L.images(case, L.F64)[0]
        X = np.zeros((rows, case.bins), dtype=np.complex128)
        assert gpu_lib.fft_rfft2_gpu(x.ctypes.data, rows, cols, X.ctypes.data) == 0
        e = float(L.errors(X[None], L.reference(case, x[None], False))[0]) / L.unit(L.F64, case)
        back = np.zeros((rows, cols), dtype=np.float64)
        assert gpu_lib.fft_irfft2_gpu(X.ctypes.data, rows, cols, back.ctypes.data) == 0
        e2 = float(L.errors(back[None], x[None])[0]) / L.unit(L.F64, case)
        print("fft_rfft2_gpu %dx%d: %.3f, round trip %.3f u log2(rows cols)" % (rows, cols, e, e2))
        assert e <= L.BOUND_K and e2 <= 2 * L.BOUND_K
    assert gpu_lib.fft_rfft2_gpu(None, 16, 32, X.ctypes.data) == -1 and gpu_lib.fft_rfft2_gpu(x.ctypes.data, 0, 32, X.ctypes.data) == -1
    assert gpu_lib.fft_irfft2_gpu(X.ctypes.data, 16, 32, None) == -1 and gpu_lib.fft_irfft2_gpu(X.ctypes.data, 16, -1, back.ctypes.data) == -1


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_numpy_front_end(gpu_lib, dt):
    """fftlib.rfft2 / irfft2 on [..., rows, cols] arrays against numpy"""
    import fftlib
    rng = np.random.default_rng(3)
    for shape in ((2, 3, 16, 32), (12, 9), (1, 8, 16)):
        x = rng.standard_normal(shape).astype(dt)
        case = L.Case("numpy", shape[-2], shape[-1], M=int(np.prod(shape[:-2], dtype=np.int64)))
        X = fftlib.rfft2(x)
        assert X.dtype == L.CDT[np.dtype(dt)] and X.shape == shape[:-1] + (shape[-1] // 2 + 1,)
        ref = np.fft.rfft2(x.astype(np.float64))
        assert float(np.max(L.errors(X.reshape((case.M,) + X.shape[-2:]), ref.reshape((case.M,) + X.shape[-2:])) / L.unit(dt, case))) <= L.BOUND_K
        back = fftlib.irfft2(X, shape[-1])
        assert back.dtype == np.dtype(dt) and back.shape == shape
        assert float(np.max(L.errors(back.reshape(case.M, -1), x.astype(np.float64).reshape(case.M, -1)) / L.unit(dt, case))) <= 2 * L.BOUND_K
    with pytest.raises(ValueError):
        fftlib.rfft2(np.zeros(8))
    with pytest.raises(ValueError):
        fftlib.irfft2(np.zeros((8, 9), dtype=np.complex64), 18)
