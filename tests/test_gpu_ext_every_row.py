"""Every row of the 2D, real and fused-consumer plans (csrc/fft_plans_ext.h) against a float64 reference, on the device, at the
cases of tests/ext_ladder.py, through accuracy.check_execute_io: per-row inputs, a NaN-filled output between two guards, the
worst bin of every row within K u log2(length), inputs unchanged, and -- where the plan allows in == out -- the in-place result
bit-identical to the out-of-place one.  Each case asserts through plan.info() that the path it was written for ran."""
import numpy as np
import pytest

import accuracy as A
import ext_ladder as L

pytestmark = pytest.mark.gpu


def _ids(v):
    return None if isinstance(v, (str, dict)) and (isinstance(v, dict) or " " in v) else str(v)


def _run_ptr(plan):
    def run(d_in, _, d_out):
        plan.execute_ptr(d_in, d_out)
        assert plan.sync() == 0
    return run


@pytest.mark.parametrize("rows,cols,nm,dtype,path,why", L.GPU_2D, ids=_ids)
def test_2d_every_matrix_every_path(gpu_lib, rows, cols, nm, dtype, path, why):
    import fftlib
    x = L.complex_rows(rows * cols, nm, dtype, seed=rows + cols)
    for d in (-1, 1):
        plan = fftlib.ExtPlan.fft2d(rows, cols, nm, d, dtype)
        try:
            info = plan.info()
            assert info.n_passes == {L.DIRECT: 1, L.STRIDED: 2, L.TRANSPOSE: 0, L.ROWS: 0}[path], (why, info.n_passes)
            if path == L.TRANSPOSE:
                assert info.workspace_bytes >= x.nbytes, why  # the transposed image
            assert bool(info.bluestein_m) == ((cols & (cols - 1)) != 0), (why, info.bluestein_m)  # the rows
            A.check_execute_io(_run_ptr(plan), x, rows * cols, dtype, "2d", L.ref_2d(rows, cols, d), n=rows * cols, inplace=True,
                               label="2D %d x %d x %d dir %+d (%s)" % (rows, cols, nm, d, why))
        finally:
            plan.destroy()


def _check_core(info, expect, batch, why):
    if "n_passes" in expect:
        assert info.n_passes == expect["n_passes"], (why, info.n_passes)
    if "chunk_lt" in expect:
        assert 0 < info.chunk_batch < expect["chunk_lt"], (why, info.chunk_batch)
    if "chunk" in expect:
        assert info.chunk_batch == expect["chunk"], (why, info.chunk_batch)
    if "bluestein" in expect:
        assert info.bluestein_m > 0, why
    if "team_kernel" in expect:
        assert info.team_kernel > 0 and info.team_tiles > 0, (why, info.team_kernel)


@pytest.mark.parametrize("n,batch,dtype,policy,expect,why", L.GPU_REAL, ids=_ids)
def test_r2c_c2r_every_row(gpu_lib, n, batch, dtype, policy, expect, why):
    """r2c: every row against rfft of the float64 input.  c2r: every row against irfft, of the r2c result (Hermitian by
    construction up to rounding: the imaginary parts of its bins 0 and n/2 are exactly zero) and of random half spectra with those
    two imaginary parts zeroed -- c2r_merge_kernel propagates them into the result where numpy's irfft ignores them.  In place
    through one buffer of batch * (n/2 + 1) complex values."""
    import fftlib
    cdt = L.C64 if dtype == L.F32 else L.C128
    hb = n // 2 + 1
    x = L.real_rows(n, batch, dtype, seed=n)
    try:
        if policy:
            fftlib.set_policy(**policy)
        fwd, inv = fftlib.ExtPlan.r2c(n, batch, dtype), fftlib.ExtPlan.c2r(n, batch, dtype)
    finally:
        fftlib.set_policy(team=1, min_batch=0, chunk_mb=0)
    try:
        for plan in (fwd, inv):
            _check_core(plan.info(), expect, batch, why)
        label = "n=%d batch=%d %s (%s)" % (n, batch, dtype, why)
        X = {}

        def run_r2c(d_in, _, d_out):
            fwd.execute_ptr(d_in, d_out)
            assert fwd.sync() == 0
            if d_in != d_out:
                X["dev"] = A.d2h(d_out, (batch, hb), cdt)

        A.check_execute_io(run_r2c, x, hb, cdt, "r2c", L.ref_r2c, n=n, inplace=True, label="r2c " + label)
        spectra = [X["dev"]]
        if X["dev"].nbytes <= 16 << 20:
            spectra.append(L.half_spectra(n, batch, cdt, seed=n + 1))
        else:
            assert np.all(X["dev"][:, 0].imag == 0) and np.all(X["dev"][:, -1].imag == 0)
        for S in spectra:
            A.check_execute_io(_run_ptr(inv), S, n, dtype, "c2r", L.ref_c2r(n), n=n, inplace=True, label="c2r " + label)
        if "team_kernel" in expect:
            assert fwd.lib.fft_gpu_plan_team_status_hip(fwd.handle) in (0, 1), why  # the team kernel (or its fallback) did the work
    finally:
        fwd.destroy()
        inv.destroy()


@pytest.mark.parametrize("kind,nx,nh,batch,dtype,policy,fused,expect,why", L.GPU_FUSED, ids=_ids)
def test_fused_consumers_every_row(gpu_lib, kind, nx, nh, batch, dtype, policy, fused, expect, why):
    """Fused, with the element-wise steps as kernels of their own (NO_FUSION) and with the middle passes unchained (NO_CHAIN):
    every row of every variant against the float64 reference (computed once), output between guards, inputs unchanged."""
    import fftlib
    x = L.complex_rows(nx, batch, dtype, seed=nx)
    y = L.complex_rows(nx, batch, dtype, seed=nx + 1) if kind == "xcorr" else None
    h = L.complex_rows(nh if kind == "conv" else nx, 1, dtype, seed=nh + 7)[0] if kind in ("conv", "circ") else None
    w_out, dt_out = L.fused_out(kind, nx, nh, dtype)
    fs = 48000.0
    try:
        if policy:
            fftlib.set_policy(**policy)
        plan = fftlib.ExtPlan.fused(kind, nx, batch, h, dtype)
    finally:
        fftlib.set_policy(team=1, min_batch=0, chunk_mb=0)
    try:
        assert plan.out_len == w_out
        ref = L.ref_fused(kind, nx, nh, h, fs)
        expected = ref(x, y) if kind == "xcorr" else ref(x)

        def run(d_x, d_y, d_out):
            plan.execute_fused(d_x, d_y, d_out, fs)
            assert plan.sync() == 0

        for no_fusion, no_chain in ((0, 0), (1, 0), (0, 1)):
            plan.set_option(fftlib.OPT_NO_FUSION, no_fusion)
            plan.set_option(fftlib.OPT_NO_CHAIN, no_chain)
            info = plan.info()
            _check_core(info, expect, batch, why)
            if fused is not None:
                assert info.fused == (0 if no_fusion else min(fused, 1) if no_chain else fused), (why, no_fusion, no_chain, info.fused)
            A.check_execute_io(run, x, w_out, dt_out, L.FUSED_FAMILY[kind], None, x2=y, n=nx, m=L.fused_m(kind, nx, nh), scale="rms_or_bin",
                               expected=expected, label="%s %d + %d x %d %s no_fusion=%d no_chain=%d (%s)" % (kind, nx, nh, batch, dtype, no_fusion, no_chain, why))
        if kind == "psd" and nx >= 4:  # the doubling condition: bins 0 and nx/2 single, their neighbours doubled -- checked above bin by bin,
            w = L.hann(nx)             # here once more against the undoubled value, so that the reference's own slice cannot hide it
            p0 = np.abs(np.fft.fft(x[:1].astype(np.complex128) * w)[0]) ** 2 / (fs * 0.375 * nx)
            assert np.allclose(expected[0, [0, nx // 2]], p0[[0, nx // 2]], rtol=1e-12)
            assert np.allclose(expected[0, [1, nx // 2 - 1]], 2 * p0[[1, nx // 2 - 1]], rtol=1e-12)
    finally:
        plan.destroy()
