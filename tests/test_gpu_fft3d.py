"""The 3D transform plan (fft_gpu_plan_3d_hip) on the device, at the cases of tests/fft3d_ladder.py: every value of every volume against
numpy's fftn / ifftn in float64, between sentinel guards that must stay bit-identical; each case asserts through plan.info() which path
ran.  Then the plan-info fields, the refusals, the dispatcher twin, the host and the numpy front ends."""
import numpy as np
import pytest

import fft3d_ladder as L

pytestmark = pytest.mark.gpu


def run_plan(depth, rows, cols, n_volumes, inverse, dtype, in_ptr, out_ptr, no_fusion=False, lds_budget=0):
    import fftlib
    lib = fftlib.init()
    prec = fftlib.PREC_F32 if np.dtype(dtype) == L.C64 else fftlib.PREC_F64
    handle = (lib.fft_gpu_plan_3d if inverse else lib.fft_gpu_plan_3d_hip)(depth, rows, cols, n_volumes, 1 if inverse else -1, prec)
    if not handle:
        return -1, None
    plan = fftlib.ExtPlan(handle)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        pi = plan.info()
        assert pi.n == cols and pi.batch == n_volumes and list(pi.factors)[:4] == [cols, rows, depth, 0] and pi.direction == (1 if inverse else -1)
        assert pi.fused in (0, 1) and not (no_fusion and pi.fused)
        if pi.fused:  # ONE launch for the planes, then the depth route: nothing, one or two column passes, or transpose / 1D / transpose
            assert pi.n_passes == (1 if depth == 1 else pi.n_passes) and pi.n_passes >= (1 if depth == 1 else 2)
            if depth > 1 and depth & (depth - 1) == 0:
                assert pi.n_passes in (2, 3), pi.n_passes
        if lib.fft_gpu_execute_ptr_hip(handle, in_ptr, out_ptr) != 0:
            return -2, None
        assert plan.sync() == 0
        return 0, dict(fused=pi.fused, n_passes=pi.n_passes)
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.FUSED + L.COMPOSITION, ids=repr)
def test_cases(gpu_lib, case, dt):
    """every shape of the ladder: both directions, out of place and in place"""
    L.check_case(run_plan, case, dt)


def test_plane_kernel_alone_equals_fft2(gpu_lib):
    case = L.Case(1, 16, 16)
    x = L.volumes(case, L.C64)
    y, info = L.run_once(run_plan, case, L.C64, x, False)
    assert info["fused"] == 1 and info["n_passes"] == 1
    assert float(np.max(L.errors(y, np.fft.fft2(x.astype(np.complex128))) / L.unit(L.C64, case))) <= L.BOUND_K


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.OPERATOR, ids=repr)
def test_impulse(gpu_lib, case, dt):
    L.check_impulse(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("inverse", (False, True), ids=["forward", "inverse"])
@pytest.mark.parametrize("case", L.OPERATOR, ids=repr)
def test_linear_operator(gpu_lib, case, inverse, dt):
    L.check_linear_operator(run_plan, case, dt, inverse)


def test_refusals_allocate_nothing(gpu_lib):
    """sizes below 1 and depth rows cols > 2^30: NULL at plan time, before any allocation"""
    import ctypes as C
    import fftlib
    lib = fftlib.init()
    a0, s0 = C.c_longlong(), C.c_longlong()
    lib.fft_gpu_debug_counters_hip(C.byref(a0), C.byref(s0))
    for args in ((0, 8, 8, 1), (8, 0, 8, 1), (8, 8, 0, 1), (8, 8, 8, 0), (1 << 11, 1 << 10, 1 << 10, 1), (1 << 10, 1 << 10, (1 << 10) + 1, 1)):
        assert lib.fft_gpu_plan_3d_hip(*args, -1, fftlib.PREC_F32) is None and lib.fft_gpu_plan_3d(*args, -1, fftlib.PREC_F64) is None
    a1, s1 = C.c_longlong(), C.c_longlong()
    lib.fft_gpu_debug_counters_hip(C.byref(a1), C.byref(s1))
    assert a1.value == a0.value
    assert lib.fft_gpu_plan_3d_hip(8, 8, 8, 1, -1, 7) is None  # an unknown precision


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_fftn_and_ifftn(gpu_lib, dt):
    """fftlib.fftn / ifftn on 3-D and 4-D arrays: numpy's results, the dtype kept, the round trip within twice the bound"""
    import fftlib
    for shape in ((4, 16, 16), (2, 4, 16, 16), (3, 5, 6, 7)):
        case = L.Case(*shape[-3:], V=1 if len(shape) == 3 else shape[0])
        x = L.volumes(case, dt).reshape(shape)
        X = fftlib.fftn(x)
        assert X.dtype == np.dtype(dt) and X.shape == x.shape
        ref = L.reference(x.reshape((case.V,) + shape[-3:]), False)
        assert float(np.max(L.errors(X.reshape(ref.shape), ref) / L.unit(dt, case))) <= L.BOUND_K
        back = fftlib.ifftn(X)
        assert back.dtype == np.dtype(dt)
        e = L.errors(back.reshape(ref.shape), x.reshape(ref.shape).astype(np.complex128)) / L.unit(dt, case)
        print("ifftn(fftn(x)) - x, %s %s: %.3f u log2 n" % (shape, np.dtype(dt).name, float(np.max(e))))
        assert float(np.max(e)) <= 2 * L.BOUND_K
    with pytest.raises(ValueError):
        fftlib.fftn(np.ones((4, 4), dtype=dt))
    with pytest.raises(ValueError):
        fftlib.ifftn(np.ones((4, 4, 4)))


def test_host_front_end(gpu_lib):
    """fft_gpu_dft_3d on host arrays, both directions, in place and out of place"""
    import fftlib
    lib = fftlib.init()
    case = L.Case(4, 8, 16, V=1)
    x = L.volumes(case, L.C128)[0]
    y = np.empty_like(x)
    assert lib.fft_gpu_dft_3d(x.ctypes.data, y.ctypes.data, 4, 8, 16, -1) == 0
    assert float(L.errors(y[None], np.fft.fftn(x)[None])[0] / L.unit(L.C128, case)) <= L.BOUND_K
    assert lib.fft_gpu_dft_3d(y.ctypes.data, y.ctypes.data, 4, 8, 16, 1) == 0
    assert float(L.errors(y[None], x[None])[0] / L.unit(L.C128, case)) <= 2 * L.BOUND_K
    assert lib.fft_gpu_dft_3d(None, y.ctypes.data, 4, 8, 16, -1) == -1 and lib.fft_gpu_dft_3d(x.ctypes.data, y.ctypes.data, 0, 8, 16, -1) == -1
