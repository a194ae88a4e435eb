"""The mixed-radix plan for 7-smooth lengths (csrc/fft_mixed_radix.h, ffteng::MixedRadixPlan) under the CPU emulation: the
unmodified kernel and planner source, a workgroup as host threads (tests/emu/emu_mixed.cpp, a library of its own).

Truth is the float64 transform of the input actually given (accuracy.fft_ref); the metric is accuracy.py's worst bin per
transform, the bound its K * u * log2(n) with K = 8, the project's K for its Stockham schedules.  Nothing is thinned: all 235
single-pass sizes run in both precisions and directions, out of place into a NaN-filled output and in place.

K table of the family (FFT_ACCURACY_REPORT over tests/test_gpu_mixed_radix.py on the MI355X, worst e_b / (u log2 n)):
    mixed_radix   K = 8    measured fp32 2.83 (n = 15) / fp64 3.44 (n = 15)
"""
import numpy as np
import pytest

import accuracy as A
import emu_mixed_lib as E
import mixed_radix_ladder as L

A.BOUND_K.setdefault("mixed_radix", 8)

C64, C128 = np.complex64, np.complex128


def _check(n, batch, dtype, d, lds_budget=0, family="mixed_radix", m=None, kind=E.KIND_MIXED):
    x = A.normal_rows(n, 0, batch, dtype, seed=n)
    y, info = E.emu_mixed(x, d, lds_budget)
    assert info[0] == kind, (n, info)
    A.check_rows(y, x, d, family, m=m, label="emulated %s n=%d" % (np.dtype(dtype).name, n))
    yi, _ = E.emu_mixed(x, d, lds_budget, inplace=True)
    assert np.array_equal(yi.view(np.uint8), y.view(np.uint8)), "in place differs from out of place, n=%d" % n
    return info


@pytest.mark.parametrize("dtype", [C64, C128], ids=["fp32", "fp64"])
@pytest.mark.parametrize("d", [-1, 1], ids=["fwd", "inv"])
def test_every_single_pass_size(dtype, d):
    assert len(L.SINGLE_PASS) == 235
    for n in L.SINGLE_PASS:
        info = _check(n, 3, dtype, d)
        assert info[1:4] == [1, n, 1], (n, info)


@pytest.mark.parametrize("dtype", [C64, C128], ids=["fp32", "fp64"])
def test_tile_rows_table_matches_the_planner(dtype):
    """mixed_radix_ladder.tile_rows(), from which the GPU tests derive their grid-filling batches, is the planner's choice."""
    for n in L.LADDER_SIZES:
        for batch in (1, 2, 7):
            _, info = E.emu_mixed(np.zeros((batch, n), dtype=dtype), -1)
            assert info[5] == L.tile_rows(n, dtype, batch), (n, batch, info[5], L.tile_rows(n, dtype, batch))
    # a full tile: enough rows that the batch does not bound it (small n only: the emulation runs them all)
    for n in (6, 15, 105, 1000, 1029, 3000, 4050):
        batch = L.tile_rows(n, dtype, 1 << 30) + 1
        _, info = E.emu_mixed(np.zeros((batch, n), dtype=dtype), -1)
        assert info[5] == L.tile_rows(n, dtype, batch) == L.tile_rows(n, dtype, 1 << 30), (n, info[5])
        assert L.lds_bytes(n, dtype, info[5]) <= L.LDS_BUDGET


@pytest.mark.parametrize("dtype", [C64, C128], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [4200, 6561, 16807, 44100, 100000])
def test_two_pass(n, dtype):
    for d in (-1, 1):
        info = _check(n, 2, dtype, d)
        assert info[1] == 2 and info[2] * info[3] == n and max(info[2], info[3]) <= 4096, info


@pytest.mark.parametrize("dtype", [C64, C128], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n", [360, 1000, 1029, 2401, 4050])
def test_small_sizes_forced_onto_two_passes(n, dtype):
    """An LDS budget too small for a tile of n: the planner splits, and the split fits the budget."""
    budget = 8192 if dtype == C64 else 16384
    for d in (-1, 1):
        info = _check(n, 3, dtype, d, lds_budget=budget)
        assert info[1] == 2 and info[2] * info[3] == n and max(info[2], info[3]) <= 4096, info


def test_ragged_batches_and_many_tiles_per_workgroup():
    """Batches that leave a partly filled last tile and give each of the emulation's three workgroups several tiles."""
    for n, batch in ((6, 2051), (15, 1000), (35, 400), (105, 123), (1000, 19), (2187, 9)):
        for dtype in (C64, C128):
            _check(n, batch, dtype, -1)


@pytest.mark.parametrize("n", [1009, 4100])
def test_other_lengths_fall_back_to_chirp_z(n):
    """A prime and a composite with a factor 41, asked for with the mixed-radix algorithm: chirp-z does them, correctly."""
    m = 1 << int(np.ceil(np.log2(2 * n - 1)))
    for dtype in (C64, C128):
        for d in (-1, 1):
            _check(n, 2, dtype, d, family="bluestein", m=m, kind=E.KIND_CHIRPZ)


def test_a_power_of_two_keeps_its_plan():
    _check(1024, 2, C64, -1, family="multipass", kind=E.KIND_POW2)


def _passes():
    """fft_gpu_mixed_radix_passes_hip of the product library where it is built (it needs no device), else the emulation's."""
    try:
        import fftlib
        return fftlib.mixed_radix_passes
    except Exception:
        return E.passes


def test_passes_exhaustively_to_100000():
    p = _passes()
    for n in range(-3, 100001):
        want = 0 if not L.is_smooth7(n) else (1 if n <= 4096 else 2)
        assert p(n) == want, (n, p(n), want)


def test_passes_of_every_smooth_length_to_2_23():
    p = _passes()
    smooth = L.smooth_numbers(1 << 23)
    assert 2000 < len(smooth) < 2800
    for n in smooth:
        assert p(n) == (1 if n <= 4096 else 2), n
        assert E.passes(n) == p(n)
    for n in (9565938, (1 << 23) + 1, 1 << 24, 2 ** 23 * 3 // 2, 0, -6, 2 ** 31 - 1):
        assert p(n) == 0, n
    assert L.is_smooth7(9565938)


def test_public_names():
    import fftlib
    assert fftlib.ALGO_MIXED_RADIX == 7 and fftlib.ALGO_NAMES["mixed_radix"] == 7
    lib = fftlib.load()
    assert lib.fft_gpu_mixed_radix_passes_hip(1000) == 1 and lib.fft_gpu_mixed_radix_passes_hip(44100) == 2
    assert hasattr(lib, "fft_mixed_radix_gpu") and hasattr(lib, "fft_gpu_set_smooth_policy_hip")
    assert fftlib.set_smooth_policy(-1) == 0  # the default: AUTO keeps chirp-z
