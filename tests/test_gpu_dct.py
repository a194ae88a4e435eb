"""The DCT / DST plans (fft_gpu_plan_dct_hip / fft_gpu_plan_dct_2d_hip) on the device, at the cases of tests/dct_ladder.py: every row
against the float64 reference, outputs between sentinel guards and gaps that must stay bit-identical, NaN in every input gap; each case
asserts through plan.info() which path ran, and runs FFT_GPU_OPT_NO_FUSION on the same data.  Then the refusals, the host and the numpy
front ends."""
import numpy as np
import pytest

import dct_ladder as L

pytestmark = pytest.mark.gpu


def _run(handle, lib, via_dispatcher, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion, n, batch):
    import fftlib
    if not handle:
        return -1, 0
    plan = fftlib.ExtPlan(handle)
    try:
        if no_fusion:
            plan.set_option(fftlib.OPT_NO_FUSION, 1)
        pi = plan.info()
        assert pi.n == n and pi.batch == batch and pi.fused in (0, 1) and pi.n_passes >= 1 and pi.factors[0] >= 1, (pi.n, pi.batch, pi.fused, pi.n_passes)
        if (lib.fft_gpu_execute_dct if via_dispatcher else lib.fft_gpu_execute_dct_hip)(handle, in_ptr, in_pitch, out_ptr, out_pitch) != 0:
            return -2, pi.fused
        assert plan.sync() == 0
        return 0, pi.fused
    finally:
        plan.destroy()


def run_plan(n, batch, type, norm, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False):
    import fftlib
    lib = fftlib.init()
    prec = fftlib.PREC_F32 if np.dtype(dtype) == L.F32 else fftlib.PREC_F64
    disp = (type & 1) != 0  # the type III plans go through the dispatcher's twins
    handle = (lib.fft_gpu_plan_dct if disp else lib.fft_gpu_plan_dct_hip)(n, batch, type, norm, prec)
    return _run(handle, lib, disp, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion, n, batch)


def run_plan2d(rows, cols, M, type, norm, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False):
    import fftlib
    lib = fftlib.init()
    prec = fftlib.PREC_F32 if np.dtype(dtype) == L.F32 else fftlib.PREC_F64
    disp = (type & 1) != 0
    handle = (lib.fft_gpu_plan_dct_2d if disp else lib.fft_gpu_plan_dct_2d_hip)(rows, cols, M, type, norm, prec)
    return _run(handle, lib, disp, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion, cols, M)


def _cases(cases):
    return [pytest.param(c, dt, id="%s-%s" % (c, "fp32" if dt == L.F32 else "fp64")) for c in cases for dt in c.dtypes]


@pytest.mark.parametrize("type", L.TYPES, ids=[L.TYPE_NAMES[t] for t in L.TYPES])
@pytest.mark.parametrize("case,dt", _cases(L.FUSED + L.FALLBACK))
def test_cases(gpu_lib, case, dt, type):
    """every shape of the ladder: the case's norms, the plan's own path and FFT_GPU_OPT_NO_FUSION"""
    L.check_case(run_plan, case, dt, type)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("type", (L.DCT2, L.DST3), ids=["dct2", "dst3"])
@pytest.mark.parametrize("case", L.CASES_2D, ids=repr)
def test_2d(gpu_lib, case, type, dt):
    L.check_2d(run_plan2d, case, dt, type, L.ORTHO if case.name == "8x16" else L.NONE)
    L.check_2d(run_plan2d, case, dt, type, L.NONE, no_fusion=True)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("type", L.TYPES, ids=[L.TYPE_NAMES[t] for t in L.TYPES])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_impulses_and_linear_operator(gpu_lib, type, dt, no_fusion):
    L.check_impulses(run_plan, dt, type, no_fusion=no_fusion)
    L.check_linear_operator(run_plan, dt, type, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("sine", (False, True), ids=["dct", "dst"])
@pytest.mark.parametrize("n", (64, 12))
def test_identities(gpu_lib, n, sine, dt):
    L.check_identities(run_plan, dt, sine, n=n)


def test_refusals(gpu_lib):
    """every NULL / -1 condition; nothing is launched"""
    import fftlib
    lib = gpu_lib
    P = fftlib.PREC_F32
    for args in ((0, 3, 0, 0), (16, 0, 0, 0), (-16, 3, 0, 0), (16, 3, 4, 0), (16, 3, -1, 0), (16, 3, 0, 3), (16, 3, 0, -1), (1 << 20, 1 << 12, 0, 0)):
        assert lib.fft_gpu_plan_dct_hip(*args, P) is None and lib.fft_gpu_plan_dct(*args, P) is None, args
    for args in ((0, 16, 1, 0, 0), (8, 0, 1, 0, 0), (8, 16, 0, 0, 0), (8, 16, 1, 4, 0), (8, 16, 1, 0, 3), (1 << 16, 1 << 15, 1, 0, 0)):
        assert lib.fft_gpu_plan_dct_2d_hip(*args, P) is None and lib.fft_gpu_plan_dct_2d(*args, P) is None, args
    one = fftlib.ExtPlan.dct(16, 3, fftlib.DCT2, fftlib.DCT_NORM_NONE, np.float32)
    two = fftlib.ExtPlan.dct2d(4, 4, 2, fftlib.DCT2, fftlib.DCT_NORM_NONE, np.float32)
    other = fftlib.ExtPlan.r2c(16, 3, np.float32)
    x = np.arange(200, dtype=np.float32)
    buf = fftlib.DeviceBuffer(x.nbytes)
    try:
        buf.upload(x)
        a, b = buf.ptr, buf.ptr + 400
        f = lib.fft_gpu_execute_dct_hip
        assert f(one.handle, a, 15, b, 16) == -1 and f(one.handle, a, 16, b, 15) == -1      # a pitch smaller than the row
        assert f(two.handle, a, 15, b, 16) == -1 and f(two.handle, a, 16, b, 15) == -1      # ... than the matrix
        assert f(one.handle, None, 0, b, 0) == -1 and f(one.handle, a, 0, None, 0) == -1 and f(None, a, 0, b, 0) == -1
        assert f(other.handle, a, 0, b, 0) == -1 and lib.fft_gpu_execute_dct(other.handle, a, 0, b, 0) == -1  # a plan of another kind
        assert lib.fft_gpu_execute_ptr_hip(one.handle, a, b) == -1                          # not the DCT execute
        assert one.sync() == 0 and two.sync() == 0
        assert np.array_equal(buf.download(x.shape, x.dtype).view(np.uint8), x.view(np.uint8))
    finally:
        buf.free()
        one.destroy()
        two.destroy()
        other.destroy()


def test_host_front_ends(gpu_lib):
    """fft_dct_gpu / fft_dct_2d_gpu on host pointers against the reference, and their refusals"""
    rng = np.random.default_rng(2)
    for n in (64, 12):
        x = rng.standard_normal(n)
        for t in L.TYPES:
            y = np.zeros(n)
            assert gpu_lib.fft_dct_gpu(x.ctypes.data, n, t, L.ORTHO, y.ctypes.data) == 0
            e = float(L.errors(y[None], L.reference(x[None], t, L.ORTHO))[0]) / L.unit(L.F64, n)
            print("fft_dct_gpu n = %d %s: %.3f u log2 N" % (n, L.TYPE_NAMES[t], e))
            assert e <= L.BOUND_K
    img = rng.standard_normal((16, 8))
    out = np.zeros((16, 8))
    assert gpu_lib.fft_dct_2d_gpu(img.ctypes.data, 16, 8, L.DCT2, L.NONE, out.ctypes.data) == 0
    e = float(L.errors(out.reshape(1, -1), L.reference2d(img[None], L.DCT2, L.NONE).reshape(1, -1))[0]) / L.unit(L.F64, 128)
    assert e <= L.BOUND_K
    assert gpu_lib.fft_dct_gpu(None, 16, 0, 0, out.ctypes.data) == -1 and gpu_lib.fft_dct_gpu(img.ctypes.data, 0, 0, 0, out.ctypes.data) == -1
    assert gpu_lib.fft_dct_gpu(img.ctypes.data, 16, 4, 0, out.ctypes.data) == -1 and gpu_lib.fft_dct_gpu(img.ctypes.data, 16, 0, 3, out.ctypes.data) == -1
    assert gpu_lib.fft_dct_2d_gpu(img.ctypes.data, 0, 8, 0, 0, out.ctypes.data) == -1 and gpu_lib.fft_dct_2d_gpu(img.ctypes.data, 16, 8, 0, 0, None) == -1


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_numpy_front_end(gpu_lib, dt):
    """fftlib.dct / idct / dst / idst / dctn / idctn against the reference, scipy's argument conventions"""
    import fftlib
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 64)).astype(dt)
    flat = x.reshape(-1, 64)
    for norm, nm in ((None, L.NONE), ("ortho", L.ORTHO)):
        for f, fi, t2, t3 in ((fftlib.dct, fftlib.idct, L.DCT2, L.DCT3), (fftlib.dst, fftlib.idst, L.DST2, L.DST3)):
            for type, t in ((2, t2), (3, t3)):
                X = f(x, type=type, norm=norm)
                assert X.dtype == np.dtype(dt) and X.shape == x.shape
                assert float(np.max(L.errors(X.reshape(-1, 64), L.reference(flat, t, nm)) / L.unit(dt, 64))) <= L.BOUND_K
                back = fi(X, type=type, norm=norm)
                assert float(np.max(L.errors(back.reshape(-1, 64), flat.astype(np.float64)) / L.unit(dt, 64))) <= 2 * L.BOUND_K
    img = rng.standard_normal((3, 12, 9)).astype(dt)
    X = fftlib.dctn(img, norm="ortho")
    assert float(np.max(L.errors(X.reshape(3, -1), L.reference2d(img, L.DCT2, L.ORTHO).reshape(3, -1)) / L.unit(dt, 108))) <= L.BOUND_K
    back = fftlib.idctn(X, norm="ortho")
    assert float(np.max(L.errors(back.reshape(3, -1), img.astype(np.float64).reshape(3, -1)) / L.unit(dt, 108))) <= 2 * L.BOUND_K
