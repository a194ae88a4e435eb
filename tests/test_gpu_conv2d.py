"""The 2D convolution / spectrum-filtering plan (fft_gpu_plan_conv2d_hip) on the device, at the cases of tests/conv2d_ladder.py: every
matrix against direct 2D convolution in float64, outputs between sentinel guards and gaps that must stay bit-identical, NaN in every
input gap; each case asserts through plan.info() which path ran, and runs FFT_GPU_OPT_NO_FUSION on the same data.  Then the host and
numpy front ends."""
import numpy as np
import pytest

import conv2d_ladder as L
from test_conv2d_no_device import row_pointers

pytestmark = pytest.mark.gpu


def run_plan(k, rows, cols, n_matrices, mode, dtype, x_ptr, x_pitch, y_ptr, y_pitch, no_fusion=False, lds_budget=0, min_seg=0, x2_ptr=None, y2_ptr=None):
    import fftlib
    lib = fftlib.init()
    k = np.ascontiguousarray(k)
    handle = lib.fft_gpu_plan_conv2d_hip(rows, cols, k.shape[0], k.shape[1], k.ctypes.data if k.size else None, n_matrices, mode, fftlib._prec_of(np.dtype(dtype)))
    if not handle:
        return -1, None
    plan = fftlib.ExtPlan(handle)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        pi = plan.info()
        info = dict(fused=pi.fused, n_passes=pi.n_passes, P=lib.fft_gpu_conv2d_padded_rows_hip(handle), Q=lib.fft_gpu_conv2d_padded_cols(handle),
                    out_rows=lib.fft_gpu_conv2d_out_rows_hip(handle), out_cols=lib.fft_gpu_conv2d_out_cols(handle), tile_cols=0)
        assert pi.n == info["Q"] and pi.batch == n_matrices and list(pi.factors)[:3] == [info["Q"], info["P"], info["Q"]]
        assert lib.fft_gpu_conv2d_padded_rows(handle) == info["P"] and lib.fft_gpu_conv2d_out_rows(handle) == info["out_rows"]
        if lib.fft_gpu_execute_conv2d_hip(handle, x_ptr, x_pitch, y_ptr, y_pitch) != 0:
            return -2, info
        if y2_ptr is not None and lib.fft_gpu_execute_conv2d(handle, x2_ptr or x_ptr, x_pitch, y2_ptr, y_pitch) != 0:
            return -2, info
        assert plan.sync() == 0
        return 0, info
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.SMALL, ids=repr)
def test_small_cases(gpu_lib, case, dt):
    """every shape of the ladder: the plan's path and FFT_GPU_OPT_NO_FUSION on three pitched matrices, then one contiguous matrix"""
    L.check_paths_agree(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.IDENTITY, ids=repr)
def test_identity_kernel(gpu_lib, case, dt):
    L.check_identity(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_largest_fused_and_one_above(gpu_lib, dt):
    L.check_largest_fused(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_many_tiles_per_matrix(gpu_lib, dt):
    """512 x 512 images, a 7 x 9 kernel, SAME: P = Q = 1024, 128 (fp32) / 256 (fp64) column tiles per matrix, multi-tile workgroups"""
    case = L.Case("same-512x512-7x9", 512, 512, 7, 9, mode=L.SAME, M=3, xpad=2, ypad=2)
    L.check(run_plan, case, dt)
    L.check(run_plan, case, dt, no_fusion=True)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_impulses(gpu_lib, dt, no_fusion):
    L.check_impulses(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_linear_operator(gpu_lib, dt, no_fusion):
    L.check_linear_operator(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_two_executes(gpu_lib, dt, no_fusion):
    L.check_two_executes(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_spectrum_mode(gpu_lib, dt):
    L.check_spectrum(run_plan, dt)


def test_refusals(gpu_lib):
    """every NULL / -1 condition; nothing is launched"""
    import fftlib
    lib = gpu_lib
    k = np.ones((3, 3), dtype=np.complex64)
    kp = k.ctypes.data
    P = fftlib.PREC_F32
    for args in ((0, 6, 3, 3, kp, 1, 0), (5, 0, 3, 3, kp, 1, 0), (5, 6, 0, 3, kp, 1, 0), (5, 6, 3, 3, None, 1, 0), (5, 6, 3, 3, kp, 0, 0), (5, 6, 3, 3, kp, 1, 5),
                 (2, 6, 3, 3, kp, 1, 2), (5, 6, 3, 3, kp, 1, 3), (4, 2, 3, 3, kp, 1, 3), (4, 8, 3, 3, kp, 1, 4), (1 << 16, 1 << 15, 1, 1, kp, 1, 0)):
        assert lib.fft_gpu_plan_conv2d_hip(*args, P) is None, args
        assert lib.fft_gpu_plan_conv2d(*args, P) is None, args
    plan = fftlib.ExtPlan.conv2d(k, 5, 6, 2, "full", np.complex64)
    assert (plan.out_rows, plan.out_cols, plan.padded) == (7, 8, (8, 8))
    x = np.arange(2 * 40 + 2 * 80, dtype=np.float32).astype(np.complex64)
    buf = fftlib.DeviceBuffer(x.nbytes)
    try:
        buf.upload(x)
        xp, yp = buf.ptr, buf.ptr + 8 * 80
        f = lib.fft_gpu_execute_conv2d_hip
        assert f(plan.handle, xp, 29, yp, 80) == -1 and f(plan.handle, xp, 40, yp, 55) == -1   # a pitch smaller than the matrix
        assert f(plan.handle, xp, 40, xp, 80) == -1                                             # d_y == d_x
        assert f(plan.handle, xp, 40, xp + 8 * 69, 80) == -1                                    # d_y starts on the last input value
        assert f(plan.handle, None, 0, yp, 0) == -1 and f(plan.handle, xp, 0, None, 0) == -1
        assert lib.fft_gpu_execute_ptr(plan.handle, xp, yp) == -1                               # not the conv2d execute
        assert plan.sync() == 0
        assert np.array_equal(buf.download(x.shape, x.dtype).view(np.uint8), x.view(np.uint8))
        assert lib.fft_gpu_conv2d_out_rows_hip(None) == -1 and lib.fft_gpu_conv2d_padded_cols_hip(None) == -1
    finally:
        buf.free()
        plan.destroy()
    other = fftlib.ExtPlan.fused("conv", 64, 1, np.ones(5, dtype=np.complex64), np.complex64)
    assert lib.fft_gpu_conv2d_out_rows_hip(other.handle) == -1 and lib.fft_gpu_conv2d_padded_rows(other.handle) == -1
    other.destroy()


def test_host_convolution_2d_front_end(gpu_lib):
    """fft_convolution_2d_gpu through row pointers (the reference's signature) against the direct sum"""
    case = L.Case("host", 37, 21, 5, 8, M=1)
    x, k = L.images(case, L.C128)[0], L.kernel(case, L.C128)
    y = np.zeros((41, 28), dtype=np.complex128)
    assert gpu_lib.fft_convolution_2d_gpu(row_pointers(x), 37, 21, row_pointers(k), 5, 8, row_pointers(y)) == 0
    e = float(L.errors(y[None], L.reference(case, x[None], k))[0]) / L.unit(L.C128, 64, 32)
    print("fft_convolution_2d_gpu: %.3f u log2 PQ" % e)
    assert e <= L.BOUND_K
    assert gpu_lib.fft_convolution_2d_gpu(None, 37, 21, row_pointers(k), 5, 8, row_pointers(y)) == -1
    assert gpu_lib.fft_convolution_2d_gpu(row_pointers(x), 0, 21, row_pointers(k), 5, 8, row_pointers(y)) == -1


def test_host_filter_2d_front_end(gpu_lib):
    """fft_filter_2d_gpu with the centred Gaussian mask gives what the plan gives with the unshifted mask, and ifft2(fft2(x) H)"""
    import fftlib
    case = L.Case("host-spectrum", 32, 32, 32, 32, mode=L.SPECTRUM, M=1)
    x = L.images(case, L.C128)[0]
    Hc = L.gaussian_mask_centred(32, 32, 4.0).astype(np.complex128)
    out = np.zeros((32, 32), dtype=np.complex128)
    assert gpu_lib.fft_filter_2d_gpu(x.ctypes.data, 32, 32, Hc.ctypes.data, out.ctypes.data) == 0
    H = np.fft.ifftshift(Hc)
    direct = fftlib.filter2d(x, H)
    assert np.array_equal(out.view(np.uint8), direct.view(np.uint8)), "the centred front end and the unshifted plan differ"
    e = float(L.errors(out[None], L.reference(case, x[None], H))[0]) / L.unit(L.C128, 32, 32)
    print("fft_filter_2d_gpu: %.3f u log2 PQ" % e)
    assert e <= L.BOUND_K
    assert gpu_lib.fft_filter_2d_gpu(x.ctypes.data, 24, 32, Hc.ctypes.data, out.ctypes.data) == -1  # no power of two
    assert gpu_lib.fft_filter_2d_gpu(None, 32, 32, Hc.ctypes.data, out.ctypes.data) == -1


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_numpy_front_end(gpu_lib, dt):
    """fftlib.conv2d in its four modes against the float64 reference; a reused plan; the real convenience"""
    import fftlib
    for mode, shape in ((L.FULL, (37, 21)), (L.SAME, (37, 21)), (L.VALID, (37, 21)), (L.CIRCULAR, (32, 16))):
        case = L.Case("numpy", shape[0], shape[1], 5, 8, mode=mode, M=2)
        x, k = L.images(case, dt), L.kernel(case, dt)
        y = fftlib.conv2d(x, k, L.MODE_NAMES[mode])
        assert y.dtype == dt and y.shape == (2,) + case.out_shape()
        P, Q = case.padded()
        e = L.errors(y, L.reference(case, x, k)) / L.unit(dt, P, Q)
        assert float(np.max(e)) <= L.BOUND_K, (mode, e)
        assert fftlib.conv2d(x[0], k, L.MODE_NAMES[mode]).shape == case.out_shape()
    case = L.Case("numpy", 37, 21, 5, 8, mode=L.SAME, M=2)
    x, k = L.images(case, dt), L.kernel(case, dt)
    plan = fftlib.ExtPlan.conv2d(k, 37, 21, 2, "same", dt)
    try:
        assert (plan.out_rows, plan.out_cols, plan.padded) == (37, 21, (64, 32))
        y = fftlib.conv2d(x, None, plan=plan)
        assert float(np.max(L.errors(y, L.reference(case, x, k)) / L.unit(dt, 64, 32))) <= L.BOUND_K
    finally:
        plan.destroy()
    xr, kr = np.ascontiguousarray(x.real), np.ascontiguousarray(k.real)
    yr = fftlib.conv2d(xr, kr, "same")
    assert yr.dtype == xr.dtype
    ref = L.reference(case, xr.astype(np.complex128), kr.astype(np.complex128))
    assert float(np.max(L.errors(yr.astype(np.complex128), ref) / L.unit(dt, 64, 32))) <= L.BOUND_K
