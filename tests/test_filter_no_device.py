"""Without a device the filter entry points fail loudly (NULL / -1), like every other entry point (tests/test_abi.py)."""
import numpy as np
import pytest


def _no_gpu():
    import fftlib
    return fftlib.load().fft_gpu_available() == 0


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the no-device behaviour cannot be observed")
def test_filter_entry_points_without_a_device():
    import fftlib
    lib = fftlib.load()
    h = np.ones(5, dtype=np.complex128)
    x = np.ones(100, dtype=np.complex128)
    y = np.full(104, 7.0 + 0j)
    assert lib.fft_gpu_plan_filter_hip(5, h.ctypes.data, 100, 1, 64, 0, fftlib.PREC_F64) is None
    assert lib.fft_gpu_plan_filter(5, h.ctypes.data, 100, 1, 64, 0, fftlib.PREC_F64) is None
    assert lib.fft_gpu_filter_out_len_hip(None) == -1 and lib.fft_gpu_filter_block(None) == -1
    assert lib.fft_gpu_execute_filter_hip(None, x.ctypes.data, 0, y.ctypes.data, 0) == -1
    assert lib.fft_gpu_execute_filter(None, x.ctypes.data, 0, y.ctypes.data, 0) == -1
    assert lib.fft_fir_filter_gpu(x.ctypes.data, 100, h.ctypes.data, 5, y.ctypes.data) == -1
    assert not lib.fft_design_fir_filter_gpu(31, 0, 1000.0, 0.0, 8000.0, 0.0)
    assert np.all(y == 7.0)
