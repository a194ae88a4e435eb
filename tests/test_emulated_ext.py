"""CPU emulation (tests/emu) of the plans built on the batched engine for the "next" rows of the scope table
(SURVEY.md 8f): 2D complex transforms, r2c / c2r, fused convolution / correlation / periodogram -- the unmodified
planner and kernel source against the oracle's restatement of the reference's applications."""
import numpy as np
import pytest

import emu_lib as E
import oracle_lib as O


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.complex128) - b) / np.linalg.norm(b))


TOL = {np.dtype(np.complex64): 3e-5, np.dtype(np.complex128): 1e-12, np.dtype(np.float32): 3e-5, np.dtype(np.float64): 1e-12}


def lcg(shape, seed, dtype):
    n = int(np.prod(shape))
    return O.gen_lcg(n, seed, 1).reshape(shape).astype(dtype)


@pytest.mark.parametrize("rows,cols,nm,dtype,lds,path", [
    (32, 64, 2, np.complex64, 0, 1),      # direct column pass
    (64, 32, 1, np.complex128, 0, 1),
    (16, 24, 3, np.complex64, 0, 1),      # cols not a power of two (rows: Bluestein over cols), still a multiple of the lane access
    (8, 5, 2, np.complex64, 0, 2),        # odd cols: 16-byte accesses impossible -> transpose path
    (12, 32, 2, np.complex128, 0, 2),     # rows not a power of two -> transpose + Bluestein
    (256, 8, 1, np.complex64, 1024, 3),   # rows do not fit one LDS tile of this budget -> two strided passes (16 x 16)
    (64, 32, 2, np.complex128, 4096, 3),  # the one-pass tile would be narrow (< 64-byte segments) -> two strided passes (8 x 8)
    (512, 8, 1, np.complex64, 2048, 3),   # 32 x 16: unequal factors, the twiddle index is the row offset
    (64, 100, 2, np.complex64, 4096, 3),  # column count not a power of two: the last column tile is partly padding
    (128, 6, 1, np.complex64, 1024, 3),
    (64, 5, 1, np.complex64, 0, 2),       # odd column count -> transpose path
    (1, 64, 2, np.complex64, 0, 0),       # a single row: rows only
])
def test_fft2d_emulated(rows, cols, nm, dtype, lds, path):
    x = lcg((nm, rows, cols), rows * 131 + cols, dtype)
    for d in (-1, 1):
        for inplace in (False, True):
            y, info = E.emu_fft2d(x, d, lds_budget=lds, inplace=inplace)
            assert info[0] == path, info[0]
            assert rel(y, O.oracle_fft2d(x.astype(np.complex128), d)) < TOL[np.dtype(dtype)], (d, inplace)
    # round trip: the inverse is scaled once
    y, _ = E.emu_fft2d(x, -1, lds_budget=lds)
    z, _ = E.emu_fft2d(y, 1, lds_budget=lds)
    assert rel(z, x.astype(np.complex128)) < TOL[np.dtype(dtype)]


@pytest.mark.parametrize("n", [2, 4, 8, 64, 1024, 6, 100, 1, 3, 9, 31, 101])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_r2c_c2r_emulated(n, dtype):
    batch = 3
    x = lcg((batch, n), n + 5, np.complex128).real.astype(dtype)
    X = E.emu_r2c(x)
    ref = O.oracle_r2c(x.astype(np.float64))
    assert X.shape == (batch, n // 2 + 1)
    assert rel(X, ref) < TOL[np.dtype(dtype)], n
    back = E.emu_c2r(X, n)
    assert np.linalg.norm(back - x) / np.linalg.norm(x) < TOL[np.dtype(dtype)] * 2, n
    assert rel(E.emu_c2r(ref.astype(X.dtype), n), O.oracle_c2r(ref, n)) < TOL[np.dtype(dtype)] * 2


@pytest.mark.parametrize("nx,nh,dtype,lds", [(100, 17, np.complex128, 0), (100, 17, np.complex64, 0), (101, 8, np.complex64, 0),
                                             (700, 401, np.complex128, 8192), (1, 1, np.complex128, 0), (5, 1, np.complex64, 0),
                                             (1500, 600, np.complex128, 40000), (2000, 148, np.complex64, 4096)])
def test_fused_linear_convolution_emulated(nx, nh, dtype, lds):
    x = lcg((4, nx), nx, dtype)
    h = lcg((nh,), nh + 3, dtype)
    ref = O.oracle_conv_linear(x.astype(np.complex128), h.astype(np.complex128))
    for no_fusion in (False, True):
        y, info = E.emu_fused("conv", x, h=h, lds_budget=lds, no_fusion=no_fusion)
        # info[1]: 1 fused ends, 2 also forward-last + inverse-first pass as one kernel (the last two cases: 64 x 64, 16 x 16 x 16)
        # ... 3: the padded transform is a single pass: FFT -> product -> inverse FFT as ONE kernel (TileHooks::mid_tab)
        # (two-pass plans with unequal factors chain through the mirrored split where the tiles agree: 1 or 2 there)
        want = (0,) if (no_fusion or info[2] == 0) else (2,) if nx >= 1500 else (3,) if info[0] == 1 else (1, 2)
        assert info[1] in want, info
        assert rel(y, ref) < TOL[np.dtype(dtype)] * 4, (nx, nh, no_fusion)
    # and against the defining sum (reference direct_convolution, convolution.c:19-31)
    direct = np.stack([np.convolve(r, h.astype(np.complex128)) for r in x.astype(np.complex128)])
    assert rel(ref, direct) < 1e-11


CHAINED_CASES = {("xcorr", 1500, 40000), ("autocorr", 1500, 4096), ("circ", 4096, 40000)}


@pytest.mark.parametrize("kind,n,dtype,lds", [("circ", 64, np.complex128, 0), ("circ", 2048, np.complex64, 4096),
                                              ("autocorr", 100, np.complex128, 0), ("autocorr", 1000, np.complex64, 4096),
                                              ("xcorr", 100, np.complex128, 0), ("xcorr", 333, np.complex64, 0),
                                              ("xcorr", 1500, np.complex128, 4096), ("xcorr", 1500, np.complex128, 40000),
                                              ("autocorr", 1500, np.complex64, 4096), ("circ", 4096, np.complex128, 40000)])
def test_fused_correlations_emulated(kind, n, dtype, lds):
    """info[1] == 2: the middle of FFT -> product -> IFFT ran as ONE kernel (fft_kernels_chain.h), see CHAINED_CASES"""
    x = lcg((3, n), n, dtype)
    y = lcg((3, n), n + 1, dtype)
    h = lcg((n,), n + 2, dtype)
    x64, y64, h64 = (a.astype(np.complex128) for a in (x, y, h))
    ref = {"circ": lambda: O.oracle_conv_circular(x64, h64), "autocorr": lambda: O.oracle_autocorr(x64),
           "xcorr": lambda: O.oracle_xcorr(x64, y64)}[kind]()
    chained = False
    for no_fusion in (False, True):
        out, info = E.emu_fused(kind, x, y=y if kind == "xcorr" else None, h=h if kind == "circ" else None, lds_budget=lds,
                                no_fusion=no_fusion)
        assert info[1] in ((0,) if no_fusion else (1, 2, 3))
        if not no_fusion and info[0] == 1:
            assert info[1] == (1 if kind == "xcorr" else 3), (kind, info)  # per-transform products keep two kernels
        chained = chained or info[1] == 2
        assert rel(out, ref) < TOL[np.dtype(dtype)] * 4, (kind, n, no_fusion)
    assert chained or (kind, n, lds) not in CHAINED_CASES, (kind, n, lds, info)


@pytest.mark.parametrize("n,dtype,lds", [(64, np.complex128, 0), (1024, np.complex64, 0), (4096, np.complex128, 4096)])
def test_fused_periodogram_emulated(n, dtype, lds):
    x = lcg((3, n), n, dtype)
    ref = O.oracle_periodogram(x.astype(np.complex128), 48000.0)
    for no_fusion in (False, True):
        psd, info = E.emu_fused("psd", x, lds_budget=lds, no_fusion=no_fusion, fs=48000.0)
        assert psd.shape == (3, n // 2 + 1)
        assert np.linalg.norm(psd - ref) / np.linalg.norm(ref) < TOL[np.dtype(dtype)] * 4


@pytest.mark.parametrize("kind", ["xcorr", "circ"])
def test_chained_pass_over_several_launch_groups(kind, monkeypatch):
    """Forward-last + inverse-first pass as ONE kernel (fft_kernels_chain.h) with the batch cut into launch groups
    (FFT_HIP_CHUNK_MB = 1: 16 transforms of m = 4096 fp64 per group, 40 = 16 + 16 + 8): the per-transform spectral table of the
    cross-correlation must follow the group offset."""
    monkeypatch.setenv("FFT_HIP_CHUNK_MB", "1")
    n, batch = (1500, 40) if kind == "xcorr" else (4096, 40)
    x = lcg((batch, n), n, np.complex128)
    y = lcg((batch, n), n + 1, np.complex128)
    h = lcg((n,), n + 2, np.complex128)
    out, info = E.emu_fused(kind, x, y=y if kind == "xcorr" else None, h=h if kind == "circ" else None, lds_budget=40000)
    assert info[1] == 2 and info[3] == 16, info  # chained, launch groups of 16
    ref = O.oracle_xcorr(x, y) if kind == "xcorr" else O.oracle_conv_circular(x, h)
    assert rel(out, ref) < TOL[np.dtype(np.complex128)] * 4


# ---------------------------------------------------------------------------------------------------------------------------
# every row against float64 (tests/accuracy.py), outputs between sentinel rows (emu_lib.*_guarded), at the cases of
# tests/ext_ladder.py: the same properties the GPU runs in tests/test_gpu_ext_every_row.py
# ---------------------------------------------------------------------------------------------------------------------------
import accuracy as A  # noqa: E402
import ext_ladder as L  # noqa: E402


def _same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what


@pytest.mark.parametrize("rows,cols,nm,dtype,lds,path,why", L.EMU_2D, ids=lambda v: None if isinstance(v, str) else str(v))
def test_fft2d_every_matrix_emulated(rows, cols, nm, dtype, lds, path, why):
    x = L.complex_rows(rows * cols, nm, dtype, seed=rows + cols).reshape(nm, rows, cols)
    for d in (-1, 1):
        y, info = E.emu_fft2d_guarded(x, d, lds_budget=lds)
        assert info[0] == path, (why, info[0])
        A.check_rows(y.reshape(nm, -1), x.reshape(nm, -1), d, "2d", n=rows * cols, ref=L.ref_2d(rows, cols, d), label="emulated 2D: " + why)
        z, _ = E.emu_fft2d_guarded(x, d, lds_budget=lds, inplace=True)
        _same_bits(z, y, "2D in place differs from out of place: " + why)


@pytest.mark.parametrize("dtype", [L.F32, L.F64], ids=str)
@pytest.mark.parametrize("n,batch", L.EMU_REAL)
def test_r2c_c2r_every_row_emulated(n, batch, dtype):
    """r2c against rfft of the float64 input; c2r of r2c results and of random Hermitian half spectra (L.half_spectra says why
    only those) against irfft; guards, untouched inputs, in place through one buffer of batch * (n/2 + 1) complex values."""
    x = L.real_rows(n, batch, dtype, seed=n)
    X = E.emu_r2c_guarded(x)
    assert X.shape == (batch, n // 2 + 1)
    A.check_rows(X, x, -1, "r2c", n=n, ref=L.ref_r2c, label="emulated r2c")
    _same_bits(E.emu_r2c_guarded(x, inplace=True), X, "r2c in place differs")
    for S in (X, L.half_spectra(n, batch, X.dtype, seed=n + 1)):
        back = E.emu_c2r_guarded(S, n)
        A.check_rows(back, S, 1, "c2r", n=n, ref=L.ref_c2r(n), label="emulated c2r")
        _same_bits(E.emu_c2r_guarded(S, n, inplace=True), back, "c2r in place differs")


def _fused_emulated(kind, nx, nh, batch, dtype, lds, fused, passes, why, monkeypatch, chunk=None):
    x = L.complex_rows(nx, batch, dtype, seed=nx)
    y = L.complex_rows(nx, batch, dtype, seed=nx + 1) if kind == "xcorr" else None
    h = L.complex_rows(nh if kind == "conv" else nx, 1, dtype, seed=nh + 7)[0] if kind in ("conv", "circ") else None
    w_out, dt_out = L.fused_out(kind, nx, nh, dtype)
    ref = L.ref_fused(kind, nx, nh, h, fs=48000.0)
    X = ref(x, y) if kind == "xcorr" else ref(x)  # computed once, shared by the variants
    assert X.shape == (batch, w_out)
    for no_fusion, no_chain in ((0, 0), (1, 0), (0, 1)):
        if no_chain:
            monkeypatch.setenv("FFT_EMU_NO_CHAIN", "1")
        out, info = E.emu_fused_guarded(kind, x, y=y, h=h, lds_budget=lds, no_fusion=bool(no_fusion), fs=48000.0)
        monkeypatch.delenv("FFT_EMU_NO_CHAIN", raising=False)
        assert out.dtype == dt_out and out.shape == (batch, w_out)
        assert info[0] == passes and info[1] == (0 if no_fusion else min(fused, 1) if no_chain else fused), (why, info)
        if chunk:
            assert info[3] == chunk, info
        A.check_rows(out, X, 0, L.FUSED_FAMILY[kind], out.dtype, n=nx, m=L.fused_m(kind, nx, nh), ref=lambda Xs: Xs, scale="rms_or_bin",
                     label="emulated %s (%s) no_fusion=%d no_chain=%d" % (kind, why, no_fusion, no_chain))


@pytest.mark.parametrize("kind,nx,nh,batch,dtype,lds,fused,passes,why", L.EMU_FUSED, ids=lambda v: None if isinstance(v, str) and " " in v else str(v))
def test_fused_every_row_emulated(kind, nx, nh, batch, dtype, lds, fused, passes, why, monkeypatch):
    _fused_emulated(kind, nx, nh, batch, dtype, lds, fused, passes, why, monkeypatch)


@pytest.mark.parametrize("kind,nx,dtype,chunk", [("xcorr", 1500, L.C128, 16), ("autocorr", 1500, L.C64, 32)], ids=str)
def test_fused_every_row_over_launch_groups_emulated(kind, nx, dtype, chunk, monkeypatch):
    """FFT_HIP_CHUNK_MB = 1: m = 4096 runs in launch groups of 16 (fp64) / 32 (fp32) transforms, 37 = 16 + 16 + 5 / 32 + 5; the
    cross-correlation's per-transform table must follow the group offset in the chained kernel and in the two-kernel path."""
    monkeypatch.setenv("FFT_HIP_CHUNK_MB", "1")
    _fused_emulated(kind, nx, 0, 37, dtype, 40000, 2, 2, "launch groups", monkeypatch, chunk=chunk)


@pytest.mark.parametrize("kind,nx,nh", [("conv", 101, 8), ("conv", 100, 18), ("conv", 127, 2), ("conv", 128, 1), ("autocorr", 33, 0), ("xcorr", 33, 0)])
def test_budget_too_small_for_m_128_fp64_is_refused(kind, nx, nh):
    """fp64, lds_budget = 4096, m = 128: the plan build fails, and that is the budget doing what it should, not a planner gap.
    A multi-pass split needs both factors >= 16 (Pow2Plan::build: l1 = 4 ... log2n - 4), so n = 32, 64, 128 are single-pass
    sizes by construction; the single-pass tile of 128 complex128 values (2 KiB) and its tables do not fit 4096 bytes, so no
    schedule exists -- the plain 1D plan of n = 128 refuses the same budget.  The device plans with 160 KiB, where every such
    size fits; one step more budget (8192) or one size up (m = 256 = 16 x 16) builds and passes."""
    x = L.complex_rows(nx, 3, L.C128, seed=nx)
    y = L.complex_rows(nx, 3, L.C128, seed=nx + 1) if kind == "xcorr" else None
    h = L.complex_rows(nh, 1, L.C128, seed=3)[0] if kind == "conv" else None
    assert L.fused_m(kind, nx, nh) == 128
    with pytest.raises(RuntimeError, match="emu_fused failed"):
        E.emu_fused(kind, x, y=y, h=h, lds_budget=4096)
    with pytest.raises(RuntimeError, match="emu_fft failed"):
        E.emu_fft(L.complex_rows(128, 3, L.C128, seed=1), lds_budget=4096)
    out, info = E.emu_fused_guarded(kind, x, y=y, h=h, lds_budget=8192)
    assert info[0] == 1
    ref = L.ref_fused(kind, nx, nh, h)
    A.check_rows(out, ref(x, y) if kind == "xcorr" else ref(x), 0, L.FUSED_FAMILY[kind], out.dtype, n=nx, m=128, ref=lambda Xs: Xs, scale="rms_or_bin")
    out, info = E.emu_fused_guarded("autocorr", L.complex_rows(100, 3, L.C128, seed=2), lds_budget=4096)  # m = 256: two passes of 16
    assert info[0] == 2 and info[2] == 8
