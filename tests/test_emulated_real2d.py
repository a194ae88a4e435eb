"""The real 2D transform plan (csrc/fft_plans_ext.h Real2DPlan) in the CPU emulation: the unmodified kernel source --
tile_fft_colpass_kernel, real2d_copy_kernel and the hooked rows kernel -- at the cases of tests/real2d_ladder.py, every value of every
matrix against numpy's rfft2 / irfft2, between guards, with NaN in every gap.  The column pass alone runs at column counts that leave a
ragged last tile.  The last test runs both paths in a stand-alone program under AddressSanitizer on exactly sized heap buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy as A
import emu_real2d_lib as ER
import real2d_ladder as L
from frames_ladder import HostMemory


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", HostMemory())


def run_plan(rows, cols, n_matrices, inverse, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False, lds_budget=0, min_seg=0):
    rc, info = ER.real2d(in_ptr, in_pitch, out_ptr, out_pitch, rows, cols, n_matrices, inverse, 1 if np.dtype(dtype) == L.F32 else 0, lds_budget, no_fusion,
                         min_seg)
    if rc == 0 and info[0] == 1 and (not inverse or out_pitch == 0):
        assert info[5] == 2, info  # TWO launches per fused execute (an inverse into pitched matrices adds the copy)
    if rc == 0 and info[0] == 1:
        assert info[3] > 0 and (cols // 2) % info[3] == 0 and info[4] == cols // 2 // info[3] + 1, info  # one live column in the last tile
    return rc, dict(fused=info[0], n_passes=info[1], bins=info[2], tile_cols=info[3])


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.FUSED + L.FALLBACK, ids=repr)
def test_cases(case, dt):
    """every shape of the ladder: both directions, the plan's path and NO_FUSION, the round trip"""
    L.check_case(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.NARROW, ids=repr)
def test_narrow_tiles(case, dt):
    """the LDS budget narrows the column tile to C = V and C = 2 V columns: 32 / 16 (fp32) full tiles per matrix and the one-column tile"""
    for inverse in (False, True):
        L.check(run_plan, case, dt, inverse)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("inverse", (False, True), ids=["forward", "inverse"])
@pytest.mark.parametrize("n_cols", (5, 9, 17))
def test_column_pass_alone(n_cols, inverse, dt):
    """The column pass alone at n_cols = 5, 9, 17 with in_ld != out_ld, value by value and (where the pitches allow) with 16-byte accesses
    on the input side: P = 64 (two radix-8 exchanges through LDS); the columns behind n_cols hold NaN on the way in and stay NaN on the
    way out."""
    cdt = L.CDT[np.dtype(dt)]
    P, nm = 64, 3
    in_ld, out_ld = n_cols + 3, n_cols + 2
    rng = np.random.default_rng(n_cols)
    x = np.full((nm, P, in_ld), np.nan, dtype=cdt)
    x[:, :, :n_cols] = (rng.standard_normal((nm, P, n_cols)) + 1j * rng.standard_normal((nm, P, n_cols))).astype(cdt)
    ref = (np.fft.ifft if inverse else np.fft.fft)(x[:, :, :n_cols].astype(np.complex128), axis=1)
    for vec in (0, 1) if in_ld % L.V[np.dtype(dt)] == 0 else (0,):
        y, C, n_ct = ER.colpass(x, n_cols, out_ld, inverse, 1.0 / P if inverse else 1.0, vec)
        assert n_ct == (n_cols + C - 1) // C and n_ct * C > n_cols, (C, n_ct)
        assert np.all(np.isnan(y[:, :, n_cols:])), "a dead column was stored"
        e = L.errors(y[:, :, :n_cols], ref) / (A.U[cdt] * np.log2(P))
        print("column pass P = %d, n_cols = %d, C = %d, vec = %d: %s u log2 P" % (P, n_cols, C, vec, np.round(e, 3)))
        assert float(np.max(e)) <= L.BOUND_K


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_largest_fused_and_twice_that(dt):
    L.check_largest_fused(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_longest_rows(dt):
    L.check_longest_rows(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_ignored_imaginary_parts(dt, no_fusion):
    L.check_ignored_imaginary_parts(run_plan, L.Case("8x16", 8, 16), dt, no_fusion)
    L.check_ignored_imaginary_parts(run_plan, L.Case("12x12", 12, 12, fused=False), dt, no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_impulses(dt, no_fusion):
    L.check_impulses(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("inverse", (False, True), ids=["forward", "inverse"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_linear_operator(dt, inverse, no_fusion):
    L.check_linear_operator(run_plan, dt, inverse, no_fusion=no_fusion)


def test_refusals():
    """every -1 / -2 condition: nothing is launched"""
    x = np.zeros(2 * 140, dtype=np.float32)
    X = np.full(2 * 80, 7, dtype=np.complex64)

    def go(rows=8, cols=16, M=2, inverse=False, ip=140, op=80, iptr=x.ctypes.data, optr=X.ctypes.data):
        return ER.real2d(iptr, ip, optr, op, rows, cols, M, inverse, 1)[0]

    assert go() == 0
    X[:] = 7
    assert go(rows=0) == -1 and go(cols=0) == -1 and go(M=0) == -1
    assert go(rows=1 << 16, cols=1 << 15, M=1) == -1                        # rows cols > 2^30
    assert go(ip=127) == -2 and go(op=71) == -2                             # a pitch smaller than the matrix
    assert go(iptr=None) == -2 and go(optr=None) == -2
    assert go(optr=x.ctypes.data) == -2                                     # d_out == d_in
    assert go(M=1, optr=x.ctypes.data + 4 * 127, op=0) == -2                # d_out starts on the last input value
    assert go(inverse=True, iptr=X.ctypes.data, optr=X.ctypes.data + 8, ip=80, op=140) == -2
    assert np.all(X == 7)


def test_memory_safety_under_asan(tmp_path):
    """tests/emu/emu_real2d_main.cpp, built with -fsanitize=address,undefined: both paths and both directions on exactly sized heap
    buffers, the column pass alone with a ragged last tile, a clean exit.  (Most of its time is the compile of the whole engine with the
    sanitizers.)"""
    exe = str(tmp_path / "emu_real2d_main")
    subprocess.run(["g++", "-O0", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-I" + ER.CSRC, os.path.join(ER.EMU_DIR, "emu_real2d_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(r.stdout[-3000:])
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0 and "all cases passed" in r.stdout
