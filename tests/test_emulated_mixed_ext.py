"""CPU emulation (tests/emu/emu_mixed_ext.cpp) of the 2D and real plans with their 7-smooth lengths on the mixed-radix engine
(what FFT_GPU_ALGO_MIXED_RADIX selects through fft_gpu_plan_2d_algo_hip / fft_gpu_plan_r2c_1d_algo_hip /
fft_gpu_plan_c2r_1d_algo_hip): the unmodified planner and kernel source at the cases of tests/mixed_ext_ladder.py.

Every result sits between sentinel rows, every input must be unchanged, every row is checked bin by bin against float64
(accuracy.check_rows), in place must give the bits of out of place, and every case asserts its path through the library's info
words.  Families 2d_mixed / r2c_mixed / c2r_mixed, K = 8 (see tests/test_gpu_mixed_ext.py for the measured values)."""
import numpy as np
import pytest

import accuracy as A
import emu_mixed_ext_lib as E
import ext_ladder as X
import mixed_ext_ladder as L

for _f in ("2d_mixed", "r2c_mixed", "c2r_mixed"):
    A.BOUND_K.setdefault(_f, 8)

_ids = lambda v: None if isinstance(v, str) and " " in v else str(v)  # noqa: E731


def _same_bits(a, b, what):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what


def test_ladders_name_the_engine_their_lengths_get():
    """The engine and pass count a case states are those its length has: a GPU case that misstates them fails here, without a device."""
    for n, _, _, eng, passes, why in L.GPU_REAL:
        core = n // 2 if n % 2 == 0 else n
        assert L.engine(core) == eng, why
        assert passes == ((1 if core <= L.MAX_L else 2) if eng == L.MIXED else None), why
    for n, _, lds, eng, _, why in L.EMU_REAL:
        assert L.engine(n // 2 if n % 2 == 0 else n) == eng, why
    for rows, _, _, path, colk, why in L.GPU_2D:
        assert colk == (L.engine(rows) if path == L.TRANSPOSE else None), why
        assert path == (L.ROWS if rows == 1 else L.TRANSPOSE if rows & (rows - 1) else L.DIRECT), why
    for rows, _, _, _, path, colk, _, why in L.EMU_2D:
        assert colk == (L.engine(rows) if path == L.TRANSPOSE else None), why


def _budget(lds, dtype):
    return L.small_budget(dtype) if lds == L.SMALL else lds


@pytest.mark.parametrize("dtype", [L.C64, L.C128], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rows,cols,nm,lds,path,colk,colpasses,why", L.EMU_2D, ids=_ids)
def test_2d_every_matrix_emulated(rows, cols, nm, lds, path, colk, colpasses, why, dtype):
    x = X.complex_rows(rows * cols, nm, dtype, seed=rows + cols).reshape(nm, rows, cols)
    budget = _budget(lds, dtype)
    for d in (-1, 1):
        y, info = E.fft2d(x, d, lds_budget=budget)
        assert info[0] == path, (why, info)
        assert info[1] == L.engine(cols) and (info[5] > 0) == (L.engine(cols) == L.MIXED), (why, info)
        if path == L.TRANSPOSE:
            assert info[2] == colk and info[3] == colpasses, (why, info)
        A.check_rows(y.reshape(nm, -1), x.reshape(nm, -1), d, "2d_mixed", n=rows * cols, ref=X.ref_2d(rows, cols, d), label="emulated 2D: " + why)
        z, _ = E.fft2d(x, d, lds_budget=budget, inplace=True)
        _same_bits(z, y, "2D in place differs from out of place: " + why)


def test_2d_column_tiles_outnumber_the_workgroups():
    """30 x 8 x 40: 320 column transforms in tiles of 136 (fp32: 4096 // 30) are three tiles, of 68 (fp64) five, on the
    emulation's 3 workgroups; 1000 x 8 x 2 fp64: two transforms per tile, eight tiles."""
    _, info = E.fft2d(X.complex_rows(240, 40, L.C128, seed=1).reshape(40, 30, 8), -1)
    assert info[0] == L.TRANSPOSE and info[2] == L.MIXED and info[4] == 68, info
    _, info = E.fft2d(X.complex_rows(8000, 2, L.C128, seed=1).reshape(2, 1000, 8), -1)
    assert info[0] == L.TRANSPOSE and info[2] == L.MIXED and info[4] == 2, info


def test_2d_without_smooth_is_the_parent_plan():
    """smooth = 0: the plans tests/ext_ladder.py asserts -- (12, 32) is TRANSPOSE with chirp-z columns, (36, 64) too."""
    for rows, cols in ((12, 32), (36, 64), (6, 10)):
        x = X.complex_rows(rows * cols, 2, L.C128, seed=3).reshape(2, rows, cols)
        y, info = E.fft2d(x, -1, smooth=False)
        assert info[0] == L.TRANSPOSE and info[2] == L.CHIRPZ and info[1] != L.MIXED, info
        A.check_rows(y.reshape(2, -1), x.reshape(2, -1), -1, "2d", n=rows * cols, ref=X.ref_2d(rows, cols, -1))


@pytest.mark.parametrize("dtype", [L.F32, L.F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n,batch,lds,eng,passes,why", L.EMU_REAL, ids=_ids)
def test_r2c_c2r_every_row_emulated(n, batch, lds, eng, passes, why, dtype):
    """r2c against rfft of the float64 input; c2r of the r2c result and of random Hermitian half spectra against irfft; in place
    through one buffer of batch * (n/2 + 1) complex values."""
    budget = _budget(lds, dtype)
    x = X.real_rows(n, batch, dtype, seed=n)
    S, info = E.r2c(x, lds_budget=budget)
    assert info[0] == eng, (why, info)
    if eng == L.MIXED:
        core = n // 2 if n % 2 == 0 else n
        assert info[1] == passes and info[2] * info[3] == core, (why, info)
    assert S.shape == (batch, n // 2 + 1)
    fam = ("r2c_mixed", "c2r_mixed") if eng == L.MIXED else ("r2c", "c2r")
    A.check_rows(S, x, -1, fam[0], n=n, ref=X.ref_r2c, label="emulated r2c: " + why)
    _same_bits(E.r2c(x, lds_budget=budget, inplace=True)[0], S, "r2c in place differs: " + why)
    for H in (S, X.half_spectra(n, batch, S.dtype, seed=n + 1)):
        back, info = E.c2r(H, n, lds_budget=budget)
        assert info[0] == eng, (why, info)
        A.check_rows(back, H, 1, fam[1], n=n, ref=X.ref_c2r(n), label="emulated c2r: " + why)
        _same_bits(E.c2r(H, n, lds_budget=budget, inplace=True)[0], back, "c2r in place differs: " + why)


@pytest.mark.parametrize("n", [12, 30])
def test_r2c_pairs_k0_and_half(n):
    """Bins 0 and n/2 of the split are real and equal sum(x) and sum((-1)^j x_j); bin h/2 (2k = h, n = 12) pairs with itself."""
    x = X.real_rows(n, 5, L.F64, seed=n)
    S, _ = E.r2c(x)
    assert np.all(S[:, 0].imag == 0) and np.all(S[:, -1].imag == 0)
    assert np.allclose(S[:, 0].real, x.sum(axis=1), rtol=0, atol=1e-13 * n)
    assert np.allclose(S[:, -1].real, (x * (-1.0) ** np.arange(n)).sum(axis=1), rtol=0, atol=1e-13 * n)
    if (n // 2) % 2 == 0:
        k = n // 4
        assert np.allclose(S[:, k], np.fft.rfft(x, axis=1)[:, k], rtol=0, atol=1e-13 * n)


def test_real_without_smooth_is_the_parent_plan():
    for n in (1000, 90, 945):
        x = X.real_rows(n, 3, L.F64, seed=n)
        S, info = E.r2c(x, smooth=False)
        assert info[0] == L.CHIRPZ, info
        A.check_rows(S, x, -1, "r2c", n=n, ref=X.ref_r2c)


def test_launch_groups_of_a_two_pass_core(monkeypatch):
    """FFT_HIP_CHUNK_MB = 1 and n = 88200 fp64 (h = 44100: 689 KiB per transform): five transforms run in groups of one."""
    monkeypatch.setenv("FFT_HIP_CHUNK_MB", "1")
    n, batch = 88200, 5
    x = X.real_rows(n, batch, L.F64, seed=n)
    S, info = E.r2c(x)
    assert info[0] == L.MIXED and info[1] == 2 and info[4] == 1, info
    A.check_rows(S, x, -1, "r2c_mixed", n=n, ref=X.ref_r2c)
    back, info = E.c2r(S, n)
    assert info[4] == 1, info
    A.check_rows(back, S, 1, "c2r_mixed", n=n, ref=X.ref_c2r(n))
