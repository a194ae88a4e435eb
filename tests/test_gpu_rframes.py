"""The frames plans on REAL signals (fft_gpu_plan_frames_real_hip: one-sided STFT, spectrogram, Welch) on the device, at the cases of
tests/rframes_ladder.py: every row against float64, the output NaN-filled between guards, NaN in every input sample no frame covers,
two executes of one plan bit-identical; each case asserts through plan.info() that the path it was written for ran."""
import ctypes as C

import numpy as np
import pytest

import accuracy as A
import frames_ladder as L
import rframes_ladder as R

pytestmark = pytest.mark.gpu

OUT = {R.STFT: "stft", R.POWER: "power", R.WELCH: "welch"}


def _plan(case, kind, dt):
    import fftlib
    w = R.user_window(case, dt)
    return fftlib.ExtPlan.frames(case.n, case.hop, case.signal_len, case.n_signals, R.WINDOW_NAMES[case.window] if w is None else w, OUT[kind], dt)


def _runner(plan):
    def run(x_ptr, pitch, out_ptr):
        plan.execute_frames(x_ptr, out_ptr, pitch, R.FS)
        assert plan.sync() == 0
    return run


def _run_case(case, kind, dt, fused=1, passes=1, no_fusion=False, x=None, expected=None, offset=0):
    import fftlib
    plan = _plan(case, kind, dt)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        info = plan.info()
        assert plan.nw == case.nw and info.n == case.n and info.batch == case.n_signals * case.nw
        assert info.fused == fused, (case, info.fused)
        assert (info.n_passes == passes) if passes > 0 else (info.n_passes >= -passes), (case, info.n_passes)
        if info.n_passes == 1:
            assert info.factors[0] == case.n // 2  # the core is the transform of half the length
        return R.check(_runner(plan), case, kind, dt, x=x, expected=expected, offset=offset)
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.SMALL, ids=repr)
def test_small_cases(gpu_lib, case, dt):
    for kind in case.kinds:
        # (n = 4: a core of length 2 has no hooked kernel, the plan takes its fallback)
        _run_case(case, kind, dt, fused=0 if case.n == 4 else 1)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_input_one_real_off_a_16_byte_boundary(gpu_lib, dt):
    for kind in R.OFFSET_CASE.kinds:
        _run_case(R.OFFSET_CASE, kind, dt, offset=1)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_impulses_against_the_closed_form(gpu_lib, dt):
    """frame w = a unit impulse at sample w: row w is W_n^(w k)"""
    x, X = R.impulse_input(R.IMPULSES, dt)
    _run_case(R.IMPULSES, R.STFT, dt, x=x, expected=X)


@pytest.mark.parametrize("case", R.GPU_F, ids=repr)
def test_largest_fused_frame(gpu_lib, case):
    """n = 8192 fp32 / 4096 fp64: one pass of half the length, fused"""
    for kind in case.kinds:
        _run_case(case, kind, case.dtypes[0], fused=1, passes=1)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.GPU_G, ids=repr)
def test_multi_pass_fallback(gpu_lib, case, dt):
    """n = 16384: pack kernel, a core of at least two passes, split kernel"""
    for kind in case.kinds:
        _run_case(case, kind, dt, fused=0, passes=-2)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_no_fusion_on_case_a(gpu_lib, dt):
    """FFT_GPU_OPT_NO_FUSION on (a): within the bound of float64, and within the bound of the fused rows"""
    for kind in R.CASE_A.kinds:
        a = _run_case(R.CASE_A, kind, dt, fused=0, no_fusion=True)
        b = _run_case(R.CASE_A, kind, dt)
        e, k = A.row_errors(a, b.astype(np.complex128 if kind == R.STFT else np.float64), scale="rms" if kind == R.STFT else "rms_or_bin")
        A.assert_within(e, k, R.bound(kind, dt, R.CASE_A.n), "no_fusion vs fused, %s" % R.KIND_NAMES[kind])


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_rows_equal_the_complex_plan_on_a_zero_imaginary_part(gpu_lib, dt):
    import fftlib
    case = R.CASE_A
    for kind in case.kinds:
        pr = _plan(case, kind, dt)
        pc = fftlib.ExtPlan.frames(case.n, case.hop, case.signal_len, case.n_signals, R.WINDOW_NAMES[case.window], OUT[kind], R.complex_dtype(dt))
        try:
            R.check_consistency(_runner(pr), _runner(pc), case, kind, dt)
        finally:
            pr.destroy()
            pc.destroy()


def test_refusals(gpu_lib):
    """bad arguments return NULL / -1, nothing is launched"""
    import fftlib
    lib = gpu_lib
    for n, hop, slen in ((2, 1, 128), (96, 16, 128), (64, 0, 128), (64, 65, 128), (64, 16, 63)):
        assert lib.fft_gpu_plan_frames_real_hip(n, hop, slen, 2, 1, None, 0, fftlib.PREC_F32) is None, (n, hop, slen)
        assert lib.fft_gpu_plan_frames_real(n, hop, slen, 2, 1, None, 0, fftlib.PREC_F32) is None, (n, hop, slen)
    assert lib.fft_gpu_plan_frames_real_hip(64, 16, 128, 2, 4, None, 0, fftlib.PREC_F32) is None  # USER without values
    plan = fftlib.ExtPlan.frames(64, 16, 128, 2, "hann", "stft", np.float32)
    x = np.random.default_rng(3).standard_normal((2 * 5 * 2, 128)).astype(np.float32)  # room for an (unwanted) result behind the signals
    buf = fftlib.DeviceBuffer(x.nbytes)
    try:
        buf.upload(x)
        assert lib.fft_gpu_execute_frames_hip(plan.handle, buf.ptr, 0, buf.ptr, 1.0) == -1  # d_out == d_x
        assert lib.fft_gpu_execute_frames_hip(plan.handle, buf.ptr, 127, buf.ptr + 4 * 2 * 128, 1.0) == -1  # pitch < signal_len
        assert lib.fft_gpu_execute_ptr_hip(plan.handle, buf.ptr, buf.ptr + 4 * 2 * 128) == -1  # not the frames execute
        assert lib.fft_gpu_execute_ptr(plan.handle, buf.ptr, buf.ptr + 4 * 2 * 128) == -1
        assert plan.sync() == 0
        assert np.array_equal(buf.download(x.shape, x.dtype).view(np.uint8), x.view(np.uint8))
        assert lib.fft_gpu_frames_count_hip(plan.handle) == 5 and lib.fft_gpu_frames_count(plan.handle) == 5
        assert plan.frames_out() == ((2, 5, 33), np.dtype(np.complex64))
    finally:
        buf.free()
        plan.destroy()


def test_host_welch_front_end(gpu_lib):
    """fft_welch_psd_real_gpu against the numpy Welch, window_size = 256, overlap = 128"""
    n, overlap, slen = 256, 128, 256 + 128 * 9 + 77
    case = R.Case("m", n, n - overlap, 1, 10, tail=77)
    assert case.signal_len == slen
    x = np.random.default_rng(21).standard_normal((1, slen))
    ptr = gpu_lib.fft_welch_psd_real_gpu(x.ctypes.data, slen, R.FS, n, overlap)
    assert ptr
    y = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(1, n // 2 + 1)).copy()
    gpu_lib.fft_free(ptr)
    e, k = A.row_errors(y, R.reference(case, x, R.WELCH, np.float64), scale="rms_or_bin")
    print("fft_welch_psd_real_gpu: worst e / (u log2 n) = %.3f" % (float(e[0]) / (A.U[R.F64] * 8)))
    A.assert_within(e, k, R.bound(R.WELCH, np.float64, n), "fft_welch_psd_real_gpu")
    for bad in ((slen, 100, 50), (slen, 256, 256), (slen, 256, -1), (200, 256, 128), (slen, 2, 1)):
        assert not gpu_lib.fft_welch_psd_real_gpu(x.ctypes.data, bad[0], R.FS, bad[1], bad[2]), bad


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_numpy_front_ends(gpu_lib, dt):
    """fftlib.stft / spectrogram / welch on a real [2][1000]: one-sided shapes, the reference's values"""
    import fftlib
    n, hop = 128, 32
    nw = (1000 - (n - hop)) // hop
    case = R.Case("n", n, hop, 2, nw, tail=1000 - (n + (nw - 1) * hop))
    assert case.signal_len == 1000
    x = np.random.default_rng(31).standard_normal((2, 1000)).astype(dt)
    for kind, f in ((R.STFT, lambda: fftlib.stft(x, n, hop)), (R.POWER, lambda: fftlib.spectrogram(x, n, hop, fs=R.FS)),
                    (R.WELCH, lambda: fftlib.welch(x, n, hop, fs=R.FS))):
        y = f()
        rows, width, odt = R.out_shape(case, kind, dt)
        assert y.dtype == odt and y.shape == ((2, nw, n // 2 + 1) if kind != R.WELCH else (2, n // 2 + 1))
        e, k = A.row_errors(y.reshape(rows, width), R.reference(case, x, kind, dt), scale="rms" if kind == R.STFT else "rms_or_bin")
        A.assert_within(e, k, R.bound(kind, dt, n), "fftlib %s, real input" % R.KIND_NAMES[kind])
    w = L.window_values(L.USER, n)
    user = R.Case("n-user", n, hop, 2, nw, tail=case.tail, window=R.USER)
    y = fftlib.welch(x, n, hop, window=w, fs=R.FS)
    e, k = A.row_errors(y, R.reference(user, x, R.WELCH, dt), scale="rms_or_bin")
    A.assert_within(e, k, R.bound(R.WELCH, dt, n), "fftlib welch, real input, user window")
    assert fftlib.stft(x[0], n, hop).shape == (nw, n // 2 + 1)  # one signal in, one signal out
