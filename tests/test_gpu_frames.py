"""The plans on overlapping frames (fft_gpu_plan_frames_hip: STFT, spectrogram, Welch) on the device, at the cases of
tests/frames_ladder.py: every frame against float64, the output NaN-filled between guards, NaN in every input sample no frame covers,
two executes of one plan bit-identical; each case asserts through plan.info() that the path it was written for ran."""
import ctypes as C

import numpy as np
import pytest

import accuracy as A
import frames_ladder as L

pytestmark = pytest.mark.gpu

OUT = {L.STFT: "stft", L.POWER: "power", L.WELCH: "welch"}


def _plan(case, kind, dt):
    import fftlib
    w = L.user_window(case, dt)
    return fftlib.ExtPlan.frames(case.n, case.hop, case.signal_len, case.n_signals, L.WINDOW_NAMES[case.window] if w is None else w, OUT[kind], dt)


def _run_case(case, kind, dt, fused=1, passes=1, no_fusion=False, x=None):
    import fftlib
    plan = _plan(case, kind, dt)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        info = plan.info()
        assert plan.nw == case.nw and info.n == case.n and info.batch == case.n_signals * case.nw
        assert info.fused == fused, (case, info.fused)
        assert (info.n_passes == passes) if passes > 0 else (info.n_passes >= -passes), (case, info.n_passes)

        def run(x_ptr, pitch, out_ptr):
            plan.execute_frames(x_ptr, out_ptr, pitch, L.FS)
            assert plan.sync() == 0

        return L.check(run, case, kind, dt, x=x)
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.SMALL, ids=repr)
def test_small_cases(gpu_lib, case, dt):
    """(a) - (e), (h), (j)"""
    for kind in case.kinds:
        _run_case(case, kind, dt)


@pytest.mark.parametrize("case", L.GPU_F, ids=repr)
def test_largest_single_pass_frame(gpu_lib, case):
    """(f): n = 4096 fp32 / 2048 fp64, one pass, fused"""
    for kind in case.kinds:
        _run_case(case, kind, case.dtypes[0], fused=1, passes=1)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.GPU_G, ids=repr)
def test_multi_pass_fallback(gpu_lib, case, dt):
    """(g): n = 8192 runs the per-signal fallback on a core of at least two passes"""
    for kind in case.kinds:
        _run_case(case, kind, dt, fused=0, passes=-2)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_welch_of_one_frame_is_the_periodogram(gpu_lib, dt):
    """(i): WELCH with nw = 1, hop = n, Hann equals FFT_GPU_FUSED_PSD of the same rows (pinned to the reference's golden vectors by
    tests/test_gpu_ext.py) to within the bound"""
    import fftlib
    case = L.Case("i", 64, 64, 5, 1, kinds=(L.WELCH,))
    x = L.make_input(case, dt)
    y = _run_case(case, L.WELCH, dt, x=x)
    p = fftlib.fused("psd", x[:, :case.n], fs=L.FS)
    e, k = A.row_errors(y, p.astype(np.float64), scale="rms_or_bin")
    A.assert_within(e, k, L.bound(L.WELCH, dt, case.n), "welch(nw = 1) vs FUSED_PSD")


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_no_fusion_on_case_a(gpu_lib, dt):
    """(k): FFT_GPU_OPT_NO_FUSION on (a), within the same bound"""
    for kind in L.CASE_A.kinds:
        _run_case(L.CASE_A, kind, dt, fused=0, no_fusion=True)


def test_refusals(gpu_lib):
    """(l): bad arguments return NULL / -1, nothing is launched"""
    import fftlib
    lib = gpu_lib
    for n, hop, slen in ((64, 0, 128), (64, 65, 128), (100, 16, 128), (64, 16, 63)):
        assert lib.fft_gpu_plan_frames_hip(n, hop, slen, 2, 1, None, 0, fftlib.PREC_F32) is None, (n, hop, slen)
    assert lib.fft_gpu_plan_frames_hip(64, 16, 128, 2, 4, None, 0, fftlib.PREC_F32) is None  # USER without values
    plan = fftlib.ExtPlan.frames(64, 16, 128, 2, "hann", "stft", np.complex64)
    x = A.block_normal_rows(128, 0, 2 * 5, np.complex64, 3)  # room for an (unwanted) in-place result
    buf = fftlib.DeviceBuffer(x.nbytes)
    try:
        buf.upload(x)
        assert lib.fft_gpu_execute_frames_hip(plan.handle, buf.ptr, 0, buf.ptr, 1.0) == -1  # d_out == d_x
        assert lib.fft_gpu_execute_frames_hip(plan.handle, buf.ptr, 127, buf.ptr + 8 * 2 * 128, 1.0) == -1  # pitch < signal_len
        assert lib.fft_gpu_execute_ptr(plan.handle, buf.ptr, buf.ptr + 8 * 2 * 128) == -1  # not the frames execute
        assert plan.sync() == 0
        assert np.array_equal(buf.download(x.shape, x.dtype).view(np.uint8), x.view(np.uint8))
        assert lib.fft_gpu_frames_count_hip(plan.handle) == 5 and lib.fft_gpu_frames_count(plan.handle) == 5
    finally:
        buf.free()
        plan.destroy()


def test_host_welch_front_end(gpu_lib):
    """(m): fft_welch_psd_gpu against the numpy Welch, window_size = 256, overlap = 128"""
    n, overlap, slen = 256, 128, 256 + 128 * 9 + 77
    case = L.Case("m", n, n - overlap, 1, 10, tail=77)
    assert case.signal_len == slen
    x = A.block_normal_rows(slen, 0, 1, np.complex128, 21)
    ptr = gpu_lib.fft_welch_psd_gpu(x.ctypes.data, slen, L.FS, n, overlap)
    assert ptr
    y = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(1, n // 2 + 1)).copy()
    gpu_lib.fft_free(ptr)
    e, k = A.row_errors(y, L.reference(case, x, L.WELCH, np.complex128), scale="rms_or_bin")
    print("fft_welch_psd_gpu: worst e / (u log2 n) = %.3f" % (float(e[0]) / (A.U[L.C128] * 8)))
    A.assert_within(e, k, L.bound(L.WELCH, np.complex128, n), "fft_welch_psd_gpu")
    for bad in ((slen, 100, 50), (slen, 256, 256), (slen, 256, -1), (200, 256, 128)):
        assert not gpu_lib.fft_welch_psd_gpu(x.ctypes.data, bad[0], L.FS, bad[1], bad[2]), bad


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_numpy_front_ends(gpu_lib, dt):
    """(n): fftlib.stft / spectrogram / welch on [2][1000]"""
    import fftlib
    n, hop = 128, 32
    nw = (1000 - (n - hop)) // hop
    case = L.Case("n", n, hop, 2, nw, tail=1000 - (n + (nw - 1) * hop))
    assert case.signal_len == 1000
    x = A.block_normal_rows(1000, 0, 2, dt, 31)
    for kind, f in ((L.STFT, lambda: fftlib.stft(x, n, hop)), (L.POWER, lambda: fftlib.spectrogram(x, n, hop, fs=L.FS)),
                    (L.WELCH, lambda: fftlib.welch(x, n, hop, fs=L.FS))):
        y = f()
        rows, width, odt = L.out_shape(case, kind, dt)
        assert y.dtype == odt and y.size == rows * width and y.shape[0] == 2
        e, k = A.row_errors(y.reshape(rows, width), L.reference(case, x, kind, dt), scale="rms" if kind == L.STFT else "rms_or_bin")
        A.assert_within(e, k, L.bound(kind, dt, n), "fftlib %s" % L.KIND_NAMES[kind])
    w = L.window_values(L.USER, n)
    user = L.Case("n-user", n, hop, 2, nw, tail=case.tail, window=L.USER)
    y = fftlib.welch(x, n, hop, window=w, fs=L.FS)
    e, k = A.row_errors(y, L.reference(user, x, L.WELCH, dt), scale="rms_or_bin")
    A.assert_within(e, k, L.bound(L.WELCH, dt, n), "fftlib welch, user window")
    assert fftlib.stft(x[0], n, hop).shape == (nw, n)  # one signal in, one signal out
