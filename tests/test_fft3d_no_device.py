"""Without a device the 3D entry points fail loudly (NULL / -1 / an exception), like every other entry point (tests/test_abi.py)."""
import numpy as np
import pytest


def _no_gpu():
    import fftlib
    return fftlib.load().fft_gpu_available() == 0


def test_fft3d_entry_points_are_declared():
    """the library exports every 3D entry point include/*.h declares, with the signatures fftlib binds; bad arguments touch nothing"""
    import fftlib
    lib = fftlib.load()
    for name in ("fft_gpu_plan_3d_hip", "fft_gpu_plan_3d", "fft_gpu_dft_3d"):
        assert name in fftlib.SIGNATURES and getattr(lib, name)
    x = np.ones((2, 8, 8), dtype=np.complex128)
    y = np.full((2, 8, 8), 7, dtype=np.complex128)
    assert lib.fft_gpu_dft_3d(None, y.ctypes.data, 2, 8, 8, -1) == -1
    assert lib.fft_gpu_dft_3d(x.ctypes.data, y.ctypes.data, 2, 0, 8, -1) == -1
    assert np.all(y == 7) and np.all(x == 1)
    for f in (fftlib.fftn, fftlib.ifftn):
        with pytest.raises(ValueError):
            f(np.ones((4, 4), dtype=np.complex64))
        with pytest.raises(ValueError):
            f(np.ones((4, 4, 4)))


@pytest.mark.skipif(not _no_gpu(), reason="a GPU is present: the no-device behaviour cannot be observed")
def test_fft3d_entry_points_without_a_device(capfd):
    import fftlib
    lib = fftlib.load()
    x = np.ones((2, 8, 8), dtype=np.complex128)
    y = np.full((2, 8, 8), 7, dtype=np.complex128)
    for prec in (fftlib.PREC_F32, fftlib.PREC_F64):
        assert lib.fft_gpu_plan_3d_hip(2, 8, 8, 1, -1, prec) is None and lib.fft_gpu_plan_3d(2, 8, 8, 1, -1, prec) is None
    assert lib.fft_gpu_dft_3d(x.ctypes.data, y.ctypes.data, 2, 8, 8, -1) == -1
    assert np.all(y == 7) and np.all(x == 1)
    assert capfd.readouterr().err.strip(), "the failure says nothing on stderr"
    for f in (fftlib.fftn, fftlib.ifftn):
        with pytest.raises(Exception):
            f(x)
    with pytest.raises(Exception):
        fftlib.ExtPlan.plan3d(2, 8, 8)
