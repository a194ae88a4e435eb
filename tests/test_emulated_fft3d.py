"""The 3D transform plan (csrc/fft_plans_ext.h Plan3D) in the CPU emulation: the unmodified kernel source -- plane_fft_kernel, the column
passes, the transposes and the 2D plan of the composition -- at the cases of tests/fft3d_ladder.py, every value of every volume against
numpy's fftn / ifftn, between guards.  A narrowed LDS budget forces the many-strip layouts and the composition at small shapes.  The last
test runs both paths in a stand-alone program under AddressSanitizer on exactly sized heap buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy as A
import emu_fft3d_lib as E3
import fft3d_ladder as L
from frames_ladder import HostMemory


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", HostMemory())


LAST = {}


def run_plan(depth, rows, cols, n_volumes, inverse, dtype, in_ptr, out_ptr, no_fusion=False, lds_budget=0):
    rc, info = E3.fft3d(in_ptr, out_ptr, depth, rows, cols, n_volumes, inverse, 1 if np.dtype(dtype) == L.C64 else 0, lds_budget, no_fusion,
                         unprefetched=lds_budget > 0)  # a narrowed budget: the many-strip layouts the device plan leaves to the composition
    LAST.clear()
    LAST.update(info)
    if rc == 0 and depth & (depth - 1) == 0 and (info["fused"] or (rows & (rows - 1) == 0 and cols & (cols - 1) == 0 and min(rows, cols) > 1)):
        assert info["n_passes"] == info["launches"], info  # what the plan reports is what it launches (a length of 1 in place launches nothing)
    if rc == 0 and info["fused"]:
        assert info["launches"] == 1 + (0, 1, 2, 3)[info["depth_route"]], info  # ONE launch for the planes, then the depth route
    return rc, info


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.FUSED + L.COMPOSITION, ids=repr)
def test_cases(case, dt):
    """every shape of the ladder: both directions, out of place and in place"""
    if case.rows == 128:  # the emulation's budget is the MI355X's: more than two strips per step in fp32, no fit in fp64 -- the composition
        case = L.Case(case.depth, case.rows, case.cols, V=case.V, fused=False)
    L.check_case(run_plan, case, dt)
    if case.depth == 3:
        assert LAST["depth_route"] == 3
    if case.depth == 1:
        assert LAST["depth_route"] == 0 and LAST["launches"] == (1 if case.fused else LAST["launches"])


def test_plane_kernel_alone_equals_fft2():
    """depth = 1: the plane kernel alone, against numpy's fft2 of every plane"""
    case = L.Case(1, 16, 16)
    x = L.volumes(case, L.C128)
    y, info = L.run_once(run_plan, case, L.C128, x, False)
    assert info["fused"] == 1 and info["launches"] == 1
    e = L.errors(y, np.fft.fft2(x)) / L.unit(L.C128, case)
    assert float(np.max(e)) <= L.BOUND_K


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape,budget,strips,prefetch", (((4, 32, 32), 0, 1, 4), ((4, 32, 32), 20 * 1024, None, 0), ((2, 16, 64), 24 * 1024, None, None),
                                                          ((2, 64, 16), 24 * 1024, None, None)), ids=repr)
def test_strip_layouts(shape, budget, strips, prefetch, dt):
    """the LDS budget picks the strip shape: one strip with the register prefetch, and many strips without it, same results"""
    case = L.Case(*shape)
    for inverse in (False, True):
        for in_place in (False, True):
            L.check(run_plan, case, dt, inverse, in_place, lds_budget=budget, report=False)
            print(LAST)
            if budget:
                assert LAST["row_strips"] > 1 and LAST["col_strips"] > 1, LAST
            if strips is not None and np.dtype(dt) == L.C64:
                assert LAST["row_strips"] == strips, LAST
            if prefetch is not None and np.dtype(dt) == L.C64:
                assert LAST["prefetch"] == prefetch, LAST


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_many_strips_at_the_full_budget(dt):
    """128 x 128 (fp32) and 64 x 128 (fp64) planes with take_unprefetched: eight strips per step inside the MI355X's 160 KiB"""
    case = L.Case(2, 128, 128, V=1) if np.dtype(dt) == L.C64 else L.Case(2, 64, 128, V=1)
    for inverse in (False, True):
        L.check(run_plan, case, dt, inverse, in_place=inverse, lds_budget=160 * 1024, report=False)
        assert LAST["prefetch"] == 0 and LAST["row_strips"] == 8, LAST


def test_small_budget_leaves_the_composition():
    case = L.Case(2, 32, 32, fused=False)
    L.check(run_plan, case, L.C64, False, lds_budget=8 * 1024, report=False)
    assert LAST["fused"] == 0 and LAST["threads"] == 0


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.OPERATOR, ids=repr)
def test_impulse(case, dt):
    L.check_impulse(run_plan, case, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("inverse", (False, True), ids=["forward", "inverse"])
@pytest.mark.parametrize("case", L.OPERATOR, ids=repr)
def test_linear_operator(case, inverse, dt):
    L.check_linear_operator(run_plan, case, dt, inverse)


def test_refusals():
    """sizes below 1 and depth rows cols > 2^30 are refused at plan time: no allocation, nothing launched"""
    x = np.full(64, 7, dtype=np.complex64)

    def go(d, r, c, v=1):
        return E3.fft3d(x.ctypes.data, x.ctypes.data, d, r, c, v, False, 1)[0]

    assert go(0, 8, 8) == -1 and go(8, 0, 8) == -1 and go(8, 8, 0) == -1 and go(1, 8, 8, 0) == -1
    assert go(1 << 11, 1 << 10, 1 << 10) == -1           # depth rows cols = 2^31
    assert go(1 << 10, 1 << 10, 1 << 10 | 1) == -1       # just above 2^30
    assert go(1, 1 << 15, 1 << 15, 4) == -1              # rows cols volumes >= 2^31
    assert np.all(x == 7)


def test_memory_safety_under_asan(tmp_path):
    """tests/emu/emu_fft3d_main.cpp, built with -fsanitize=address,undefined: both paths, both directions, every strip layout on exactly
    sized heap buffers, a clean exit.  (Most of its time is the compile of the whole engine with the sanitizers.)"""
    exe = str(tmp_path / "emu_fft3d_main")
    subprocess.run(["g++", "-O0", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-I" + E3.CSRC, os.path.join(E3.EMU_DIR, "emu_fft3d_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(r.stdout[-4000:])
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0 and "all cases passed" in r.stdout
