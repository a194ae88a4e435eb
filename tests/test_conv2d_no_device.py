"""Without a device the 2D convolution entry points fail loudly (NULL / -1), like every other entry point (tests/test_abi.py)."""
import ctypes as C

import numpy as np
import pytest


def _no_gpu():
    import fftlib
    return fftlib.load().fft_gpu_available() == 0


def row_pointers(a):
    """a [rows][cols] complex128 -> a C array of row pointers (complex_t**)"""
    return (C.c_void_p * a.shape[0])(*[a[i].ctypes.data for i in range(a.shape[0])])


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the no-device behaviour cannot be observed")
def test_conv2d_entry_points_without_a_device():
    import fftlib
    lib = fftlib.load()
    k = np.ones((3, 3), dtype=np.complex128)
    x = np.ones((8, 8), dtype=np.complex128)
    y = np.full((10, 10), 7.0 + 0j)
    for mode in range(4):
        assert lib.fft_gpu_plan_conv2d_hip(8, 8, 3, 3, k.ctypes.data, 1, mode, fftlib.PREC_F64) is None
        assert lib.fft_gpu_plan_conv2d(8, 8, 3, 3, k.ctypes.data, 1, mode, fftlib.PREC_F64) is None
    assert lib.fft_gpu_plan_conv2d_hip(8, 8, 8, 8, x.ctypes.data, 1, 4, fftlib.PREC_F64) is None
    for f in (lib.fft_gpu_conv2d_out_rows_hip, lib.fft_gpu_conv2d_out_cols_hip, lib.fft_gpu_conv2d_padded_rows_hip, lib.fft_gpu_conv2d_padded_cols_hip,
              lib.fft_gpu_conv2d_out_rows, lib.fft_gpu_conv2d_out_cols, lib.fft_gpu_conv2d_padded_rows, lib.fft_gpu_conv2d_padded_cols):
        assert f(None) == -1
    assert lib.fft_gpu_execute_conv2d_hip(None, x.ctypes.data, 0, y.ctypes.data, 0) == -1
    assert lib.fft_gpu_execute_conv2d(None, x.ctypes.data, 0, y.ctypes.data, 0) == -1
    assert lib.fft_convolution_2d_gpu(row_pointers(x), 8, 8, row_pointers(k), 3, 3, row_pointers(y)) == -1
    out = np.full((8, 8), 7.0 + 0j)
    assert lib.fft_filter_2d_gpu(x.ctypes.data, 8, 8, x.ctypes.data, out.ctypes.data) == -1
    assert np.all(y == 7.0) and np.all(out == 7.0)
