"""Overlap-save FIR filtering (csrc/fft_plans_ext.h FilterPlan) in the CPU emulation: the unmodified kernel source -- the bounded framed
load and the valid-part framed store of tile_fft_kernel, filter_gather_kernel, filter_scatter_kernel -- at the cases of
tests/filter_ladder.py, every signal against direct convolution, between guards, with NaN in every gap.  The last test runs the same
paths in a stand-alone program under AddressSanitizer on exactly sized heap buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy as A
import emu_filter_lib as EF
import filter_ladder as L
from frames_ladder import HostMemory


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", HostMemory())


def run_plan(h, signal_len, n_signals, n, mode, dtype, x_ptr, x_pitch, y_ptr, y_pitch, no_fusion=False, no_chain=False, lds_budget=0,
             x2_ptr=None, y2_ptr=None):
    rc, info = EF.filter(x_ptr, y_ptr, h, signal_len, n_signals, n, mode, x_pitch, y_pitch, 1 if np.dtype(dtype) == L.C64 else 0, lds_budget,
                         no_fusion, no_chain, x2_ptr, y2_ptr)
    if rc == 0 and info[1] == 3:
        assert info[3] == 1, info  # ONE launch per execute
    return rc, info[1], info[5]


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.SMALL, ids=repr)
def test_small_cases(case, dt):
    """every block length, tap count, signal length and layout of the ladder, all three modes, fused against NO_FUSION"""
    for mode in L.MODES:
        L.check_paths_agree(run_plan, case, mode, dt)


@pytest.mark.parametrize("case", L.LARGEST, ids=repr)
def test_largest(case):
    """n = 4096 fp32 / 2048 fp64: one launch, against the gather / middle / scatter fallback (FFT_GPU_OPT_NO_FUSION) on the same data"""
    for mode in L.MODES:
        L.check_paths_agree(run_plan, case, mode, case.dtypes[0])


@pytest.mark.parametrize("case", L.ABOVE, ids=repr)
def test_above_the_largest(case):
    """one n above the largest and one long filter report the fallback"""
    for mode in L.MODES:
        L.check(run_plan, case, mode, case.dtypes[0])


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_no_chain_and_multi_pass_fallbacks(dt):
    """NO_CHAIN (hooked passes: 1) and a two-pass core under a small LDS budget (chained: 2) on the straddling case"""
    L.check(run_plan, L.CASE_STRADDLE, L.FULL, dt, label="no_chain", expect_path=(1,), no_chain=True)
    case = L.Case("n256-2pass", 256, 17, 1000, 3, xpad=1, ypad=1)
    L.check(run_plan, case, L.CENTRED, dt, label="two passes", expect_path=(1, 2), lds_budget=4096)


def test_frames_exact_refusal_falls_back():
    """2 signals x 50000 blocks: tile columns x blocks per signal exceed 2^32, the multiply-high split is not exact, the plan falls back"""
    case = L.Case("exact", 4, 3, 2 * 50000 - 2, 2, fused=False)
    L.check(run_plan, case, L.FULL, L.C64, expect_path=(0, 1, 2))


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_impulses(dt):
    L.check_impulses(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_linear_operator(dt, no_fusion):
    L.check_linear_operator(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_two_executes(dt, no_fusion):
    L.check_two_executes(run_plan, dt, no_fusion=no_fusion)


def test_refusals():
    """every NULL / -1 condition: nothing is launched"""
    x = np.zeros((2, 300), dtype=np.complex64)
    y = np.full((2, 400), 7, dtype=np.complex64)
    h = np.ones(5, dtype=np.complex64)

    def go(h=h, slen=200, S=2, n=64, xp=300, yp=400, xptr=x.ctypes.data, yptr=y.ctypes.data):
        return EF.filter(xptr, yptr, h, slen, S, n, L.FULL, xp, yp, 1)[0]

    assert go() == 0
    y[:] = 7
    assert go(h=np.zeros(0, dtype=np.complex64)) == -1   # n_taps < 1
    assert go(slen=0) == -1 and go(S=0) == -1
    assert go(n=48) == -1                                 # not a power of two
    assert go(n=4) == -1                                  # n <= n_taps - 1
    assert go(xp=199) == -2 and go(yp=203) == -2          # a pitch smaller than the row
    assert go(yptr=x.ctypes.data) == -2                   # d_y == d_x
    assert go(S=1, yptr=x.ctypes.data + 8 * 199, yp=0) == -2  # d_y starts on the last input sample
    assert np.all(y == 7)


def test_memory_safety_under_asan(tmp_path):
    """tests/emu/emu_filter_main.cpp, built with -fsanitize=address,undefined: both paths on exactly sized heap buffers, a clean exit"""
    exe = str(tmp_path / "emu_filter_main")
    subprocess.run(["g++", "-O0", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-I" + EF.CSRC, os.path.join(EF.EMU_DIR, "emu_filter_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(r.stdout[-2000:])
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0 and "all cases passed" in r.stdout
