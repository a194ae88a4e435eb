"""The cross frames plans (fft_gpu_plan_cross_frames_hip / _real_hip: cross-spectral density, coherence, H1 transfer estimate of
signal pairs) on the device, at the cases of tests/cross_ladder.py: every bin of Pxx, Pyy, Pxy, coherence and H1 against float64
numpy, everything between guards, NaN in every sample no frame covers, two executes of one plan bit-identical.  The reference
project's compute_coherence is no oracle (it writes 1.0 into every bin); the oracle is cross_ladder.reference."""
import ctypes as C

import numpy as np
import pytest

import accuracy as A
import cross_ladder as X

pytestmark = pytest.mark.gpu


class Device:
    """cross_ladder's backend on the device: one plan per run."""

    def _window(self, case, dt):
        w = X.user_window(case, dt)
        return X.WINDOW_NAMES[case.window] if w is None else w

    def run(self, case, kind, dt, x_ptr, x_pitch, y_ptr, y_pitch, out_ptrs, no_fusion=False):
        import fftlib
        plan = fftlib.ExtPlan.cross_frames(case.n, case.hop, case.signal_len, case.n_signals, self._window(case, dt), X.KIND_NAMES[kind], dt)
        try:
            if no_fusion:
                plan.set_option(fftlib.OPT_NO_FUSION, 1)
            info = plan.info()
            assert info.n == case.n and info.batch == case.n_signals * case.nw and info.chunk_batch == plan.chunk
            assert plan.cross_out()[0][:2] == (case.n_signals, case.hb)
            for p in out_ptrs:
                plan.execute_cross(x_ptr, y_ptr, p, x_pitch, y_pitch, X.FS)
                assert plan.sync() == 0
            return dict(fused=info.fused, passes=info.n_passes, nw=plan.nw, C=plan.chunk, chunks=-(-plan.nw // plan.chunk))
        finally:
            plan.destroy()

    def welch(self, case, dt, x_ptr, pitch, out_ptr):
        import fftlib
        plan = fftlib.ExtPlan.frames(case.n, case.hop, case.signal_len, case.n_signals, self._window(case, dt), "welch", dt)
        try:
            plan.execute_frames(x_ptr, out_ptr, pitch, X.FS)
            assert plan.sync() == 0
        finally:
            plan.destroy()


DEV = Device()
ALL_DT = pytest.mark.parametrize("dt", X.DTYPES, ids=X.dtype_id)


@pytest.mark.parametrize("case,dt", [(c, dt) for c in X.SMALL for dt in c.dtypes], ids=lambda v: v.name if isinstance(v, X.Case) else X.dtype_id(v))
def test_small_cases(gpu_lib, case, dt):
    info = X.run_case(DEV, case, dt)
    assert info["fused"] == (0 if (case.n == 4 and X.is_real(dt)) else 1), info
    assert info["C"] == 32 and info["chunks"] == {31: 1, 32: 1, 33: 2, 75: 3}.get(case.nw, 1)


@pytest.mark.parametrize("case", X.BIG, ids=repr)
def test_one_step_past_the_one_launch_range(gpu_lib, case):
    """n = 16384 fp32 and fp64, real signals: the inner plan's pack, multi-pass core and split; n = 8192 fp64: its largest one-launch frame"""
    info = X.run_case(DEV, case, case.dtypes[0])
    if case.name in X.DEVICE_FALLBACK:
        assert info["fused"] == 0 and info["passes"] >= 2, info
    else:
        assert info["fused"] == 1 and info["passes"] == 1, info


@ALL_DT
def test_bases_one_element_off_a_16_byte_boundary(gpu_lib, dt):
    X.check_all(DEV, X.OFFSET_CASE, dt, offset=1)
    X.check_kind(DEV, X.OFFSET_CASE, X.COHERENCE, dt, offset=1)


@ALL_DT
def test_no_fusion(gpu_lib, dt):
    X.identity_no_fusion(DEV, dt)


@ALL_DT
def test_a_signal_with_itself(gpu_lib, dt):
    X.identity_same_pointer(DEV, dt)


@ALL_DT
def test_a_signal_and_its_double(gpu_lib, dt):
    X.identity_doubled(DEV, dt)


@ALL_DT
def test_swapped_pair_gives_the_conjugate(gpu_lib, dt):
    X.identity_swap(DEV, dt)


@ALL_DT
def test_one_frame_is_fully_coherent(gpu_lib, dt):
    X.identity_one_frame(DEV, dt)


@ALL_DT
def test_pxx_is_the_welch_plans(gpu_lib, dt):
    X.identity_welch(DEV, dt)


@ALL_DT
def test_zero_power(gpu_lib, dt):
    X.identity_zero_x(DEV, dt)


@pytest.mark.parametrize("dt", (X.F32, X.C128), ids=X.dtype_id)
def test_a_poisoned_pair_stays_alone(gpu_lib, dt):
    X.identity_poisoned_pair(DEV, dt)


def test_refusals(gpu_lib):
    """bad arguments return NULL / -1, nothing is launched"""
    import fftlib
    lib = gpu_lib
    for real, dispatch in ((lib.fft_gpu_plan_cross_frames_real_hip, lib.fft_gpu_plan_cross_frames_real), (lib.fft_gpu_plan_cross_frames_hip, lib.fft_gpu_plan_cross_frames)):
        for n, hop, slen in ((96, 16, 128), (64, 0, 128), (64, 65, 128), (64, 16, 63)):
            assert real(n, hop, slen, 2, 1, None, 3, fftlib.PREC_F32) is None and dispatch(n, hop, slen, 2, 1, None, 3, fftlib.PREC_F32) is None, (n, hop, slen)
        assert real(64, 16, 128, 2, 4, None, 3, fftlib.PREC_F32) is None  # USER without values
        assert real(64, 16, 128, 2, 1, None, 4, fftlib.PREC_F32) is None and real(64, 16, 128, 2, 1, None, -1, fftlib.PREC_F32) is None  # a bad kind
    assert lib.fft_gpu_plan_cross_frames_real_hip(2, 1, 128, 2, 1, None, 3, fftlib.PREC_F32) is None  # n = 2 real
    plan = fftlib.ExtPlan.cross_frames(64, 16, 128, 2, "hann", "all", np.float32)
    x = np.random.default_rng(3).standard_normal((4, 256)).astype(np.float32)  # two pairs of signals, and room for an (unwanted) result
    buf = fftlib.DeviceBuffer(x.nbytes)
    try:
        buf.upload(x)
        xp, yp, op = buf.ptr, buf.ptr + 4 * 256, buf.ptr + 4 * 512
        ex = lib.fft_gpu_execute_cross_frames_hip
        for args in ((None, 0, yp, 0, op), (xp, 0, None, 0, op), (xp, 0, yp, 0, None), (xp, 127, yp, 0, op), (xp, 0, yp, 127, op),
                     (xp, 0, yp, 0, xp), (xp, 0, yp, 0, yp), (xp, 0, yp, 0, yp + 4 * 200)):
            assert ex(plan.handle, args[0], args[1], args[2], args[3], args[4], 1.0) == -1, args
            assert lib.fft_gpu_execute_cross_frames(plan.handle, args[0], args[1], args[2], args[3], args[4], 1.0) == -1, args
        assert lib.fft_gpu_execute_ptr_hip(plan.handle, xp, op) == -1 and lib.fft_gpu_execute_frames_hip(plan.handle, xp, 0, op, 1.0) == -1
        assert plan.sync() == 0
        assert np.array_equal(buf.download(x.shape, x.dtype).view(np.uint8), x.view(np.uint8))
        assert lib.fft_gpu_frames_count_hip(plan.handle) == 5 and lib.fft_gpu_frames_count(plan.handle) == 5
        assert lib.fft_gpu_cross_chunk_hip(plan.handle) == 32 and lib.fft_gpu_cross_chunk(plan.handle) == 32
        assert plan.cross_out() == ((2, 33, 4), np.dtype(np.float32))
    finally:
        buf.free()
        plan.destroy()


def _two_tone_pair(n, seed=41):
    """two tones plus noise in x; y: the tones at other amplitudes and phases, plus noise of its own"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.cos(2 * np.pi * 0.11 * t) + 0.5 * np.cos(2 * np.pi * 0.27 * t + 0.3) + 0.7 * rng.standard_normal(n)
    y = 0.6 * np.cos(2 * np.pi * 0.11 * t + 1.0) + 0.9 * np.cos(2 * np.pi * 0.27 * t - 0.4) + 0.5 * x + 0.7 * rng.standard_normal(n)
    return x, y


def _host_array(ptr, count, dtype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(count * (2 if np.dtype(dtype) == X.C128 else 1),)).copy().view(dtype)


def test_host_front_ends(gpu_lib):
    """compute_coherence_gpu (the reference's signature: Hann, overlap window_size / 2, rate 1) and fft_coherence_real_gpu against the
    float64 oracle on a two-tone-plus-noise pair, n = 4096, window_size = 256; fft_csd_real_gpu against fftlib.csd.  (The reference's
    own compute_coherence returns 1.0 everywhere and is no oracle.)"""
    import fftlib
    n, ws = 4096, 256
    x, y = _two_tone_pair(n)
    nw = (n - ws // 2) // (ws // 2)
    case = X.Case("host", ws, ws // 2, 1, nw, tail=n - (ws + (nw - 1) * (ws // 2)))
    assert case.signal_len == n
    hb = ws // 2 + 1
    for dt, call in ((X.C128, lambda a, b: gpu_lib.compute_coherence_gpu(a.ctypes.data, b.ctypes.data, n, ws)),
                     (X.F64, lambda a, b: gpu_lib.fft_coherence_real_gpu(a.ctypes.data, b.ctypes.data, n, ws, ws // 2))):
        a, b = np.ascontiguousarray(x.astype(dt)), np.ascontiguousarray(y.astype(dt))
        ptr = call(a, b)
        assert ptr
        coh = _host_array(ptr, hb, np.float64).reshape(1, hb)
        gpu_lib.fft_free(ptr)
        ref = X.reference(case, a.reshape(1, -1), b.reshape(1, -1), dt, fs=1.0)
        err, lim = np.abs(coh - X.coherence_ref(ref)), X.coherence_bound(case, dt, ref)
        print("%s: worst error / bound = %.3f" % (X.dtype_id(dt), float(np.max(err / lim))))
        X._assert_bins(err, lim, "host coherence %s" % X.dtype_id(dt))
        assert np.all(coh >= 0) and np.all(coh <= 1 + 1e-12) and float(np.max(coh)) > 0.5
    pxy = np.zeros(hb, dtype=np.complex128)
    assert gpu_lib.fft_csd_real_gpu(x.ctypes.data, y.ctypes.data, n, X.FS, ws, ws // 2, pxy.ctypes.data) == 0
    assert np.array_equal(pxy, fftlib.csd(x, y, ws, ws // 2, fs=X.FS))
    for bad in ((n, 100, 50), (n, 256, 256), (n, 256, -1), (200, 256, 128), (n, 2, 1)):
        assert not gpu_lib.fft_coherence_real_gpu(x.ctypes.data, y.ctypes.data, bad[0], bad[1], bad[2]), bad
        assert gpu_lib.fft_csd_real_gpu(x.ctypes.data, y.ctypes.data, bad[0], X.FS, bad[1], bad[2], pxy.ctypes.data) == -1, bad
    assert not gpu_lib.compute_coherence_gpu(None, y.ctypes.data, n, ws) and not gpu_lib.compute_coherence_gpu(x.ctypes.data, y.ctypes.data, n, 100)


@ALL_DT
def test_numpy_front_ends(gpu_lib, dt):
    """fftlib.csd / coherence / transfer on [2][1000] pairs: shapes, dtypes, and the float64 values"""
    import fftlib
    n, hop = 128, 32
    nw = (1000 - (n - hop)) // hop
    case = X.Case("py", n, hop, 2, nw, tail=1000 - (n + (nw - 1) * hop))
    assert case.signal_len == 1000
    x, y = X.make_pair(case, dt)
    ref = X.reference(case, x, y, dt)
    cdt = X.C64 if X.real_dtype(dt) == X.F32 else X.C128
    for got, want, lim, odt in ((fftlib.csd(x, y, n, hop, fs=X.FS), ref[2], X.spectrum_bounds(case, dt, ref)[2], cdt),
                                (fftlib.coherence(x, y, n, hop), X.coherence_ref(ref), X.coherence_bound(case, dt, ref), X.real_dtype(dt)),
                                (fftlib.transfer(x, y, n, hop), ref[2] / ref[0], X.transfer_bound(case, dt, ref), cdt)):
        assert got.shape == (2, n // 2 + 1) and got.dtype == odt
        X._assert_bins(np.abs(got.astype(want.dtype) - want), lim, "fftlib front end %s" % X.dtype_id(dt))
    assert fftlib.coherence(x[0], y[0], n, hop).shape == (n // 2 + 1,)  # one pair in, one row out
