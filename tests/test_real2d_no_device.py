"""Without a device the real 2D transform entry points fail loudly (NULL / -1 / an exception), like every other entry point
(tests/test_abi.py)."""
import numpy as np
import pytest


def _no_gpu():
    import fftlib
    return fftlib.load().fft_gpu_available() == 0


def test_real2d_entry_points_are_declared():
    """the library exports every real 2D entry point include/*.h declares, with the signatures fftlib binds"""
    import fftlib
    lib = fftlib.load()
    for name in ("fft_gpu_plan_r2c_2d_hip", "fft_gpu_plan_c2r_2d_hip", "fft_gpu_real2d_bins_hip", "fft_gpu_execute_real2d_hip", "fft_gpu_plan_r2c_2d",
                 "fft_gpu_plan_c2r_2d", "fft_gpu_real2d_bins", "fft_gpu_execute_real2d", "fft_rfft2_gpu", "fft_irfft2_gpu"):
        assert name in fftlib.SIGNATURES and getattr(lib, name)
    assert lib.fft_gpu_real2d_bins_hip(None) == -1 and lib.fft_gpu_real2d_bins(None) == -1
    x = np.ones((8, 16))
    X = np.full((8, 9), 7.0 + 0j)
    assert lib.fft_gpu_execute_real2d_hip(None, x.ctypes.data, 0, X.ctypes.data, 0) == -1
    assert lib.fft_gpu_execute_real2d(None, x.ctypes.data, 0, X.ctypes.data, 0) == -1
    assert np.all(X == 7.0)


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the no-device behaviour cannot be observed")
def test_real2d_entry_points_without_a_device():
    import fftlib
    lib = fftlib.load()
    x = np.ones((8, 16))
    X = np.full((8, 9), 7.0 + 0j)
    for prec in (fftlib.PREC_F32, fftlib.PREC_F64):
        for f in (lib.fft_gpu_plan_r2c_2d_hip, lib.fft_gpu_plan_c2r_2d_hip, lib.fft_gpu_plan_r2c_2d, lib.fft_gpu_plan_c2r_2d):
            assert f(8, 16, 1, prec) is None
    assert lib.fft_rfft2_gpu(x.ctypes.data, 8, 16, X.ctypes.data) == -1
    back = np.full((8, 16), 7.0)
    assert lib.fft_irfft2_gpu(X.ctypes.data, 8, 16, back.ctypes.data) == -1
    assert np.all(X == 7.0) and np.all(back == 7.0)
    with pytest.raises(Exception):
        fftlib.rfft2(x)
    with pytest.raises(Exception):
        fftlib.irfft2(X, 16)
    with pytest.raises(Exception):
        fftlib.ExtPlan.real2d(8, 16)
