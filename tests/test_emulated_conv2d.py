"""The 2D convolution / spectrum-filtering plan (csrc/fft_plans_ext.h Conv2DPlan) in the CPU emulation: the unmodified kernel source --
tile_fft_colround_kernel, conv2d_pad_kernel, conv2d_crop_kernel -- at the cases of tests/conv2d_ladder.py, every matrix against direct
2D convolution, between guards, with NaN in every gap.  The column round alone runs at row lengths that leave a partial last tile.  The
last test runs both paths in a stand-alone program under AddressSanitizer on exactly sized heap buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy as A
import conv2d_ladder as L
import emu_conv2d_lib as EC
from frames_ladder import HostMemory


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", HostMemory())


def run_plan(k, rows, cols, n_matrices, mode, dtype, x_ptr, x_pitch, y_ptr, y_pitch, no_fusion=False, lds_budget=0, min_seg=0, x2_ptr=None, y2_ptr=None):
    rc, info = EC.conv2d(x_ptr, y_ptr, k, rows, cols, n_matrices, mode, x_pitch, y_pitch, 1 if np.dtype(dtype) == L.C64 else 0, lds_budget, no_fusion,
                         min_seg, x2_ptr, y2_ptr)
    if rc == 0 and info[0] == 1 and x_pitch == 0 and y_pitch == 0:
        assert info[7] == 3, info  # THREE launches per execute of contiguous matrices (single-pass rows)
    return rc, dict(fused=info[0], n_passes=info[1], P=info[2], Q=info[3], out_rows=info[4], out_cols=info[5], tile_cols=info[6])


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.SMALL, ids=repr)
def test_small_cases(case, dt):
    """every shape of the ladder: the plan's path and NO_FUSION on three pitched matrices, then one contiguous matrix"""
    L.check_paths_agree(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.IDENTITY, ids=repr)
def test_identity_kernel(case, dt):
    L.check_identity(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.NARROW, ids=repr)
def test_narrow_tiles(case, dt):
    """the LDS budget narrows the column tile to C = V and C = 2 V columns: many tiles per matrix, every one a full tile"""
    L.check(run_plan, case, dt)
    L.check(run_plan, case, dt, no_fusion=True)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("Q,budget", [(6, 0), (12, {L.C64: 5000, L.C128: 9500})], ids=["one-partial-tile", "full-then-partial"])
def test_partial_last_tile(dt, Q, budget):
    """The column round alone at a row length the plan never makes (Q no power of two): the last tile of C = 8 columns has 2 (Q = 6) or 4
    (Q = 12) dead columns, which load zeros, read nothing of H and store nothing.  P = 64: two radix-8 exchanges through LDS."""
    dt = np.dtype(dt)
    P, rows_in, rows_out, nm = 64, 50, 37, 3
    rng = np.random.default_rng(5 + Q)
    x = (rng.standard_normal((nm, rows_in, Q)) + 1j * rng.standard_normal((nm, rows_in, Q))).astype(dt)
    H = (rng.standard_normal((P, Q)) + 1j * rng.standard_normal((P, Q))).astype(dt)
    y, C, n_ct = EC.colround(x, H, rows_out, 1 if dt == L.C64 else 0, budget[dt] if budget else 0)
    assert C == 8 and n_ct == (Q + 7) // 8 and n_ct * C > Q, (C, n_ct)
    xp = np.zeros((nm, P, Q), dtype=np.complex128)
    xp[:, :rows_in] = x
    ref = np.fft.ifft(np.fft.fft(xp, axis=1) * H.astype(np.complex128), axis=1)[:, :rows_out]
    e = L.errors(y, ref) / (A.U[dt] * np.log2(P))
    print("column round P = %d, Q = %d, C = %d: %s u log2 P" % (P, Q, C, np.round(e, 3)))
    assert float(np.max(e)) <= L.BOUND_K


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_largest_fused_and_one_above(dt):
    L.check_largest_fused(run_plan, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_impulses(dt, no_fusion):
    L.check_impulses(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_linear_operator(dt, no_fusion):
    L.check_linear_operator(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_two_executes(dt, no_fusion):
    L.check_two_executes(run_plan, dt, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_spectrum_mode(dt):
    L.check_spectrum(run_plan, dt)


def test_refusals():
    """every NULL / -1 condition: nothing is launched"""
    x = np.zeros((2, 40), dtype=np.complex64)
    y = np.full((2, 80), 7, dtype=np.complex64)
    k = np.ones((3, 3), dtype=np.complex64)

    def go(k=k, rows=5, cols=6, M=2, mode=L.FULL, xp=40, yp=80, xptr=x.ctypes.data, yptr=y.ctypes.data):
        return EC.conv2d(xptr, yptr, k, rows, cols, M, mode, xp, yp, 1)[0]

    assert go() == 0
    y[:] = 7
    assert go(rows=0) == -1 and go(cols=0) == -1 and go(M=0) == -1 and go(k=np.zeros((0, 0), dtype=np.complex64)) == -1
    assert go(mode=5) == -1 and go(mode=-1) == -1
    assert go(k=np.ones((6, 3), dtype=np.complex64), mode=L.VALID) == -1 and go(k=np.ones((3, 7), dtype=np.complex64), mode=L.VALID) == -1
    assert go(mode=L.CIRCULAR) == -1                                               # 5 x 6: no powers of two
    assert go(rows=4, cols=8, k=np.ones((5, 3), dtype=np.complex64), mode=L.CIRCULAR) == -1  # a kernel larger than the image
    assert go(rows=4, cols=8, mode=L.SPECTRUM) == -1                               # H is not rows x cols
    assert go(rows=1 << 16, cols=1 << 15, k=np.ones((1, 1), dtype=np.complex64), M=1) == -1  # P Q > 2^30
    assert go(xp=29) == -2 and go(yp=55) == -2                                     # a pitch smaller than the matrix
    assert go(yptr=x.ctypes.data) == -2                                            # d_y == d_x
    assert go(M=1, yptr=x.ctypes.data + 8 * 29, yp=0) == -2                        # d_y starts on the last input value
    assert np.all(y == 7)


def test_memory_safety_under_asan(tmp_path):
    """tests/emu/emu_conv2d_main.cpp, built with -fsanitize=address,undefined: both paths on exactly sized heap buffers, a clean exit.
    (Like the filter plan's sanitizer test, most of its time is the compile of the whole engine with the sanitizers.)"""
    exe = str(tmp_path / "emu_conv2d_main")
    subprocess.run(["g++", "-O0", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-I" + EC.CSRC, os.path.join(EC.EMU_DIR, "emu_conv2d_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(r.stdout[-2000:])
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0 and "all cases passed" in r.stdout
