"""The inverse STFT plan (fft_gpu_plan_iframes_real_hip: one-sided rows back to real signals by weighted overlap-add) on the device, at
the cases of tests/iframes_ladder.py: every sample of every signal against float64, the output pre-filled with a NaN pattern between
guards, two executes of one plan bit-identical; each case asserts through plan.info() that the path it was written for ran."""
import numpy as np
import pytest

import iframes_ladder as R

pytestmark = pytest.mark.gpu


def _plan(case, dt):
    import fftlib
    w = R.user_window(case, dt)
    return fftlib.ExtPlan.iframes(case.n, case.hop, case.nw, case.n_signals, R.WINDOW_NAMES[case.window] if w is None else w, dt)


def _runner(plan):
    def run(X_ptr, y_ptr, pitch):
        plan.execute_iframes(X_ptr, y_ptr, pitch)
        assert plan.sync() == 0
    return run


def _run_case(case, dt, fused=1, passes=1, no_fusion=False, X=None, expected=None):
    import fftlib
    plan = _plan(case, dt)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        info = plan.info()
        assert plan.out_len == case.out_len and info.n == case.n and info.batch == case.n_signals * case.nw and info.direction == 1
        assert info.fused == fused, (case, info.fused)
        assert (info.n_passes == passes) if passes > 0 else (info.n_passes >= -passes), (case, info.n_passes)
        if info.n_passes == 1:
            assert info.factors[0] == case.n // 2  # the core is the transform of half the length
        y, lost = R.check(_runner(plan), case, dt, X=X, expected=expected, family="iframes" if fused else "iframes_fallback")
        assert plan.unrecoverable == lost
        return y, plan.unrecoverable
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.SMALL, ids=repr)
def test_small_cases(gpu_lib, case, dt):
    # (n = 4: a core of length 2 has no hooked kernel, the plan takes its fallback)
    y, lost = _run_case(case, dt, fused=0 if case.n == 4 else 1)
    if case.name == "h-hann":
        assert lost == 2 and np.all(y[:, 0] == 0) and np.all(y[:, -1] == 0)
    if case.name == "h-rect":
        assert lost == 0


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_edge_bin_imaginary_parts_are_ignored(gpu_lib, dt, no_fusion):
    import fftlib
    plan = _plan(R.CASE_A, dt)
    try:
        plan.set_option(fftlib.OPT_NO_FUSION, 1 if no_fusion else 0)
        R.check_edge_bins_ignored(_runner(plan), R.CASE_A, dt)
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_a_nan_frame_poisons_exactly_its_samples(gpu_lib, dt, no_fusion):
    import fftlib
    plan = _plan(R.CASE_A, dt)
    try:
        plan.set_option(fftlib.OPT_NO_FUSION, 1 if no_fusion else 0)
        R.check_nan_frame(_runner(plan), R.CASE_A, dt)
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_impulses_against_the_closed_form(gpu_lib, dt):
    X, y = R.impulse_spectra(R.IMPULSES, dt)
    _, limit, scale, lost = R.reference(R.IMPULSES, X, dt)
    _run_case(R.IMPULSES, dt, X=X, expected=(y, limit, scale, lost))


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.ROUND_TRIPS, ids=repr)
def test_round_trip(gpu_lib, case, dt):
    """istft(stft(x)) against x; the forward leg is the real frames plan (fftlib.stft on a real x)"""
    import fftlib
    x = R.round_trip_input(case, dt)
    X = fftlib.stft(x, case.n, case.hop, R.WINDOW_NAMES[case.window])
    assert X.shape == (case.n_signals, case.nw, case.bins) and X.dtype == R.complex_dtype(dt)
    _run_case(case, dt, X=X, expected=R.round_trip_expected(case, x, dt))


@pytest.mark.parametrize("case", R.GPU_F, ids=repr)
def test_largest_fused_frame(gpu_lib, case):
    """n = 8192 fp32 / 4096 fp64: one pass of half the length, fused"""
    _run_case(case, case.dtypes[0], fused=1, passes=1)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.GPU_G, ids=repr)
def test_multi_pass_fallback(gpu_lib, case, dt):
    """n = 16384: merge kernel, a core of at least two passes, overlap-add"""
    _run_case(case, dt, fused=0, passes=-2)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_no_fusion_agrees_with_the_fused_path(gpu_lib, dt):
    """FFT_GPU_OPT_NO_FUSION on (a): within the bound of float64, and within twice the bound of the fused signals"""
    case = R.CASE_A
    a, _ = _run_case(case, dt, fused=0, no_fusion=True)
    b, _ = _run_case(case, dt)
    _, limit, scale, _ = R.reference(case, R.make_spectra(case, dt), dt)
    R.sample_check(a, b.astype(np.float64), 2 * limit, scale, case, dt, "no_fusion vs fused")


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_numpy_front_end(gpu_lib, dt):
    """fftlib.istft on [signals, frames, n//2 + 1] and on one signal's [frames, n//2 + 1]"""
    import fftlib
    case = R.CASE_A
    X = R.make_spectra(case, dt)
    y_ref, limit, scale, _ = R.reference(case, X, dt)
    y = fftlib.istft(X, case.n, case.hop, R.WINDOW_NAMES[case.window])
    assert y.shape == (case.n_signals, case.out_len) and y.dtype == np.dtype(dt)
    R.sample_check(y, y_ref, limit, scale, case, dt, "fftlib.istft")
    one = fftlib.istft(X[1], case.n, case.hop, R.WINDOW_NAMES[case.window])
    assert one.shape == (case.out_len,) and np.array_equal(one.view(np.uint8), y[1].view(np.uint8))


def test_refusals(gpu_lib):
    """bad arguments return NULL / -1, nothing is launched"""
    import fftlib
    lib = gpu_lib
    w = np.ones(64, dtype=np.float32)
    for n, hop, nw, S in ((2, 1, 5, 2), (96, 16, 5, 2), (0, 1, 5, 2), (64, 0, 5, 2), (64, 65, 5, 2), (64, 16, 0, 2), (64, 16, 5, 0),
                          (64, 16, 65536, 65536), (1 << 20, 1 << 19, 1 << 21, 1)):
        assert lib.fft_gpu_plan_iframes_real_hip(n, hop, nw, S, 1, None, fftlib.PREC_F32) is None, (n, hop, nw, S)
        assert lib.fft_gpu_plan_iframes_real(n, hop, nw, S, 1, None, fftlib.PREC_F32) is None, (n, hop, nw, S)
    assert lib.fft_gpu_plan_iframes_real_hip(64, 16, 5, 2, 4, None, fftlib.PREC_F32) is None  # USER without values
    h = lib.fft_gpu_plan_iframes_real(64, 16, 5, 2, 4, w.ctypes.data, fftlib.PREC_F32)  # ... and with them, through the dispatcher
    assert h and lib.fft_gpu_iframes_len(h) == 128 and lib.fft_gpu_iframes_unrecoverable(h) == 0
    lib.fft_gpu_destroy_plan(h)
    plan = fftlib.ExtPlan.iframes(64, 16, 5, 2, "hann", np.float32)
    X = np.random.default_rng(3).standard_normal((2 * 5, 66)).astype(np.float32)  # 10 rows of 33 bins
    y = np.full((2, 130), 7.0, dtype=np.float32)
    bx, by = fftlib.DeviceBuffer(X.nbytes), fftlib.DeviceBuffer(y.nbytes)
    try:
        bx.upload(X)
        by.upload(y)
        assert plan.out_len == 128 and plan.unrecoverable == 2
        assert lib.fft_gpu_iframes_len_hip(plan.handle) == 128 and lib.fft_gpu_iframes_unrecoverable_hip(plan.handle) == 2
        assert lib.fft_gpu_execute_iframes_hip(plan.handle, bx.ptr, bx.ptr, 0) == -1  # d_y == d_X
        assert lib.fft_gpu_execute_iframes_hip(plan.handle, bx.ptr, by.ptr, 127) == -1  # pitch < out_len
        assert lib.fft_gpu_execute_iframes_hip(plan.handle, None, by.ptr, 0) == -1
        assert lib.fft_gpu_execute_iframes_hip(plan.handle, bx.ptr, None, 0) == -1
        assert lib.fft_gpu_execute_iframes(plan.handle, bx.ptr, by.ptr, 127) == -1
        assert lib.fft_gpu_execute_ptr_hip(plan.handle, bx.ptr, by.ptr) == -1  # not the inverse frames execute
        assert lib.fft_gpu_execute_frames_hip(plan.handle, bx.ptr, 0, by.ptr, 1.0) == -1
        assert plan.sync() == 0
        assert np.array_equal(by.download(y.shape, y.dtype), y) and np.array_equal(bx.download(X.shape, X.dtype).view(np.uint8), X.view(np.uint8))
        fwd = fftlib.ExtPlan.frames(64, 16, 128, 2, "hann", "stft", np.float32)
        try:
            assert lib.fft_gpu_iframes_len_hip(fwd.handle) == -1 and lib.fft_gpu_iframes_unrecoverable_hip(fwd.handle) == -1
            assert lib.fft_gpu_execute_iframes_hip(fwd.handle, bx.ptr, by.ptr, 0) == -1
        finally:
            fwd.destroy()
        assert lib.fft_gpu_execute_iframes(plan.handle, bx.ptr, by.ptr, 130) == 0 and plan.sync() == 0  # the dispatcher's execute
        out = by.download(y.shape, y.dtype)
        assert np.all(out[:, 128:] == 7.0) and np.all(np.isfinite(out))
    finally:
        bx.free()
        by.free()
        plan.destroy()
