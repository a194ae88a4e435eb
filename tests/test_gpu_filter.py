"""Overlap-save FIR filtering (fft_gpu_plan_filter_hip) on the device, at the cases of tests/filter_ladder.py: every signal against
direct convolution, outputs between sentinel guards and gaps that must stay bit-identical, NaN in every input gap; each case asserts
through plan.info() which path ran.  Then the host and numpy front ends, and the FIR design against recorded outputs of the
reference's design_fir_filter (tests/golden/reference_filter_vectors.npz, made by tests/golden/make_golden_filter.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_ladder as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_plan(h, signal_len, n_signals, n, mode, dtype, x_ptr, x_pitch, y_ptr, y_pitch, no_fusion=False, no_chain=False, lds_budget=0,
             x2_ptr=None, y2_ptr=None):
    import fftlib
    lib = fftlib.init()
    h = np.ascontiguousarray(h)
    handle = lib.fft_gpu_plan_filter_hip(h.size, h.ctypes.data if h.size else None, signal_len, n_signals, n, mode, fftlib._prec_of(np.dtype(dtype)))
    if not handle:
        return -1, -1, -1
    plan = fftlib.ExtPlan(handle)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        if no_chain:
            plan.set_option(fftlib.OPT_NO_CHAIN, 1)
        info = plan.info()
        assert info.n == lib.fft_gpu_filter_block_hip(handle) == lib.fft_gpu_filter_block(handle)
        assert lib.fft_gpu_filter_out_len_hip(handle) == lib.fft_gpu_filter_out_len(handle) == (signal_len + h.size - 1 if mode == L.FULL else signal_len)
        if lib.fft_gpu_execute_filter_hip(handle, x_ptr, x_pitch, y_ptr, y_pitch) != 0:
            return -2, info.fused, info.n
        if y2_ptr is not None and lib.fft_gpu_execute_filter(handle, x2_ptr or x_ptr, x_pitch, y2_ptr, y_pitch) != 0:
            return -2, info.fused, info.n
        assert plan.sync() == 0
        return 0, info.fused, info.n
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.SMALL, ids=repr)
def test_small_cases(gpu_lib, case, dt):
    """every block length, tap count, signal length and layout of the ladder, all three modes, fused against FFT_GPU_OPT_NO_FUSION"""
    for mode in L.MODES:
        L.check_paths_agree(run_plan, case, mode, dt)


@pytest.mark.parametrize("case", L.LARGEST, ids=repr)
def test_largest(gpu_lib, case):
    """n = 4096 fp32 / 2048 fp64: one launch, against the gather / middle / scatter fallback (FFT_GPU_OPT_NO_FUSION) on the same data"""
    for mode in L.MODES:
        L.check_paths_agree(run_plan, case, mode, case.dtypes[0])


@pytest.mark.parametrize("case", L.ABOVE, ids=repr)
def test_above_the_largest(gpu_lib, case):
    """one n above the largest and one long filter report the fallback"""
    for mode in L.MODES:
        L.check(run_plan, case, mode, case.dtypes[0])


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_no_chain_takes_the_fallback(gpu_lib, dt):
    L.check(run_plan, L.CASE_STRADDLE, L.FULL, dt, label="no_chain", expect_path=(1,), no_chain=True)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_impulses(gpu_lib, dt):
    L.check_impulses(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_linear_operator(gpu_lib, dt, no_fusion):
    L.check_linear_operator(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_two_executes(gpu_lib, dt, no_fusion):
    L.check_two_executes(run_plan, dt, no_fusion=no_fusion)


def test_refusals(gpu_lib):
    """every NULL / -1 condition; nothing is launched"""
    import fftlib
    lib = gpu_lib
    h = np.ones(5, dtype=np.complex64)
    hp = h.ctypes.data
    P = fftlib.PREC_F32
    for args in ((0, hp, 200, 2, 64), (5, None, 200, 2, 64), (5, hp, 0, 2, 64), (5, hp, 200, 0, 64), (5, hp, 200, 2, 48), (5, hp, 200, 2, 4), (5, hp, 200, 2, -8)):
        assert lib.fft_gpu_plan_filter_hip(args[0], args[1], args[2], args[3], args[4], 0, P) is None, args
        assert lib.fft_gpu_plan_filter(args[0], args[1], args[2], args[3], args[4], 0, P) is None, args
    assert lib.fft_gpu_plan_filter_hip(5, hp, 200, 2, 64, 3, P) is None  # no such output mode
    plan = fftlib.ExtPlan.filter(h, 200, 2, "full", 64, np.complex64)
    x = np.arange(2 * 300 + 2 * 400, dtype=np.float32).astype(np.complex64)
    buf = fftlib.DeviceBuffer(x.nbytes)
    try:
        buf.upload(x)
        xp, yp = buf.ptr, buf.ptr + 8 * 600
        f = lib.fft_gpu_execute_filter_hip
        assert f(plan.handle, xp, 199, yp, 400) == -1 and f(plan.handle, xp, 300, yp, 203) == -1  # a pitch smaller than the row
        assert f(plan.handle, xp, 300, xp, 400) == -1                                               # d_y == d_x
        assert f(plan.handle, xp, 300, xp + 8 * 499, 400) == -1                                     # d_y starts on the last input sample
        assert f(plan.handle, xp + 8 * 100, 300, xp, 0) == -1                                       # d_y ends inside d_x
        assert f(plan.handle, None, 0, yp, 0) == -1 and f(plan.handle, xp, 0, None, 0) == -1
        assert lib.fft_gpu_execute_ptr(plan.handle, xp, yp) == -1                                   # not the filter execute
        assert plan.sync() == 0
        assert np.array_equal(buf.download(x.shape, x.dtype).view(np.uint8), x.view(np.uint8))
        assert lib.fft_gpu_filter_out_len_hip(None) == -1 and lib.fft_gpu_filter_block_hip(None) == -1
    finally:
        buf.free()
        plan.destroy()
    other = fftlib.ExtPlan.fused("conv", 64, 1, h, np.complex64)
    assert lib.fft_gpu_filter_out_len_hip(other.handle) == -1 and lib.fft_gpu_filter_block(other.handle) == -1
    other.destroy()


def test_host_fir_filter_front_end(gpu_lib):
    """fft_fir_filter_gpu against fft_convolution_gpu and against the direct sum, nx no single transform's business"""
    import accuracy as A
    nx, nh = 20011, 63
    case = L.Case("host", 256, nh, nx)
    x, h = L.signals(case, L.C128, seed=3), L.taps(case, L.C128)
    y = np.zeros(nx + nh - 1, dtype=np.complex128)
    yc = np.zeros_like(y)
    assert gpu_lib.fft_fir_filter_gpu(x.ctypes.data, nx, h.ctypes.data, nh, y.ctypes.data) == 0
    assert gpu_lib.fft_convolution_gpu(x.ctypes.data, nx, h.ctypes.data, nh, yc.ctypes.data) == 0
    ref = L.reference(case, x, h, L.FULL, L.C128)
    e = float(L.errors(y[None, :], ref)[0]) / L.unit(L.C128, 256)
    ec = float(L.errors(yc[None, :], ref)[0]) / (A.U[L.C128] * 15)
    d = float(np.max(np.abs(y - yc)) / np.sqrt(np.mean(np.abs(ref) ** 2)).astype(np.float64))
    print("fft_fir_filter_gpu: %.3f u log2 256; fft_convolution_gpu: %.3f u log2 2^15; apart: %.3g" % (e, ec, d))
    assert e <= L.BOUND_K and d <= (L.BOUND_K * L.unit(L.C128, 256) + A.BOUND_K["fused_conv"] * A.U[L.C128] * 15)
    assert gpu_lib.fft_fir_filter_gpu(None, nx, h.ctypes.data, nh, y.ctypes.data) == -1
    assert gpu_lib.fft_fir_filter_gpu(x.ctypes.data, 0, h.ctypes.data, nh, y.ctypes.data) == -1


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_numpy_front_end(gpu_lib, dt):
    """fftlib.fir_filter in its three modes against np.convolve / the causal slice; a reused plan; the real convenience"""
    import fftlib
    case = L.Case("numpy", 256, 31, 3001, 2)
    x, h = L.signals(case, dt), L.taps(case, dt)
    for mode in L.MODES:
        y = fftlib.fir_filter(x, h, L.MODE_NAMES[mode], n=256)
        assert y.dtype == dt and y.shape == (2, case.out_len(mode))
        e = L.errors(y, L.reference(case, x, h, mode, dt)) / L.unit(dt, 256)
        assert float(np.max(e)) <= L.BOUND_K, (mode, e)
    assert fftlib.fir_filter(x[0], h, "same").shape == (3001,)
    plan = fftlib.ExtPlan.filter(h, 3001, 2, "causal", 0, dt)
    try:
        assert plan.block == 256 and plan.out_len == 3001
        y = fftlib.fir_filter(x, None, plan=plan)
        assert float(np.max(L.errors(y, L.reference(case, x, h, L.CAUSAL, dt)) / L.unit(dt, 256))) <= L.BOUND_K
    finally:
        plan.destroy()
    xr, hr = np.ascontiguousarray(x.real), np.ascontiguousarray(h.real)
    yr = fftlib.fir_filter(xr, hr, "same")
    assert yr.dtype == xr.dtype
    ref = np.stack([np.convolve(r.astype(np.float64), hr.astype(np.float64), "same") for r in xr])
    assert float(np.max(L.errors(yr.astype(np.complex128), ref.astype(np.complex128)) / L.unit(dt, 256))) <= L.BOUND_K


def test_fir_design_against_the_reference(gpu_lib):
    """fft_design_fir_filter_gpu against what the reference's design_fir_filter computed for the same parameters"""
    import fftlib
    G = np.load(os.path.join(ROOT, "tests", "golden", "reference_filter_vectors.npz"))
    for i, (taps, kind, lo, hi, fs, tw) in enumerate(G["sets"]):
        h = fftlib.design_fir(int(taps), int(kind), lo, hi, fs, tw)
        ref = G["taps_%d" % i]
        r = float(np.linalg.norm(h - ref) / np.linalg.norm(ref))
        print("design_fir set %d: rel %.3g" % (i, r))
        assert r < 1e-14, (i, r)
    assert not gpu_lib.fft_design_fir_filter_gpu(1, 0, 1000.0, 0.0, 8000.0, 0.0)
    assert not gpu_lib.fft_design_fir_filter_gpu(31, 5, 1000.0, 0.0, 8000.0, 0.0)
    assert fftlib.design_fir(31, "lowpass", 1000.0, fs=8000.0).shape == (31,)
