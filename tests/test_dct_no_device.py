"""Without a device the DCT / DST entry points fail loudly (NULL / -1 / an exception), like every other entry point (tests/test_abi.py)."""
import numpy as np
import pytest


def _no_gpu():
    import fftlib
    return fftlib.load().fft_gpu_available() == 0


def test_dct_entry_points_are_declared():
    """the library exports every DCT entry point include/*.h declares, with the signatures fftlib binds; NULL-plan calls touch nothing"""
    import fftlib
    lib = fftlib.load()
    for name in ("fft_gpu_plan_dct_hip", "fft_gpu_plan_dct_2d_hip", "fft_gpu_execute_dct_hip", "fft_gpu_plan_dct", "fft_gpu_plan_dct_2d",
                 "fft_gpu_execute_dct", "fft_dct_gpu", "fft_dct_2d_gpu"):
        assert name in fftlib.SIGNATURES and getattr(lib, name)
    assert (fftlib.DCT2, fftlib.DCT3, fftlib.DST2, fftlib.DST3) == (0, 1, 2, 3)
    assert (fftlib.DCT_NORM_NONE, fftlib.DCT_NORM_INVERSE, fftlib.DCT_NORM_ORTHO) == (0, 1, 2)
    x = np.ones(16)
    y = np.full(16, 7.0)
    assert lib.fft_gpu_execute_dct_hip(None, x.ctypes.data, 0, y.ctypes.data, 0) == -1
    assert lib.fft_gpu_execute_dct(None, x.ctypes.data, 0, y.ctypes.data, 0) == -1
    assert np.all(y == 7.0) and np.all(x == 1.0)
    for f in (fftlib.dct, fftlib.idct, fftlib.dst, fftlib.idst, fftlib.dctn, fftlib.idctn):
        with pytest.raises(NotImplementedError):
            f(np.ones((4, 4)), type=1)
        with pytest.raises(NotImplementedError):
            f(np.ones((4, 4)), type=4)
        with pytest.raises(ValueError):
            f(np.ones((4, 4), dtype=np.complex64))


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the no-device behaviour cannot be observed")
def test_dct_entry_points_without_a_device():
    import fftlib
    lib = fftlib.load()
    x = np.ones((8, 16))
    y = np.full((8, 16), 7.0)
    for prec in (fftlib.PREC_F32, fftlib.PREC_F64):
        assert lib.fft_gpu_plan_dct_hip(16, 8, 0, 0, prec) is None and lib.fft_gpu_plan_dct(16, 8, 0, 0, prec) is None
        assert lib.fft_gpu_plan_dct_2d_hip(8, 16, 1, 0, 0, prec) is None and lib.fft_gpu_plan_dct_2d(8, 16, 1, 0, 0, prec) is None
    assert lib.fft_dct_gpu(x.ctypes.data, 16, 0, 0, y.ctypes.data) == -1
    assert lib.fft_dct_2d_gpu(x.ctypes.data, 8, 16, 0, 0, y.ctypes.data) == -1
    assert np.all(y == 7.0) and np.all(x == 1.0)
    for f in (fftlib.dct, fftlib.idct, fftlib.dst, fftlib.idst, fftlib.dctn, fftlib.idctn):
        with pytest.raises(Exception):
            f(x)
    with pytest.raises(Exception):
        fftlib.ExtPlan.dct(16, 8)
    with pytest.raises(Exception):
        fftlib.ExtPlan.dct2d(8, 16)
