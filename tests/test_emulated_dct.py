"""The cosine / sine transform plans (csrc/fft_plans_ext.h DctPlan, Dct2DPlan) in the CPU emulation: the unmodified kernel source --
dct_rows_kernel, dct_pre_kernel, dct_post_kernel, transpose_real_kernel -- at the cases of tests/dct_ladder.py, every row against the
float64 reference, between guards, with NaN in every gap.  The reference itself is checked against scipy where scipy imports.  The last
test runs both paths in a stand-alone program under AddressSanitizer on exactly sized heap buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy as A
import dct_ladder as L
import emu_dct_lib as ED
from frames_ladder import HostMemory


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", HostMemory())


def _prec(dtype):
    return 1 if np.dtype(dtype) == L.F32 else 0


def run_plan(n, batch, type, norm, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False):
    info = (ED.C.c_int * 4)()
    rc = ED.lib().emu_dct(in_ptr, in_pitch, out_ptr, out_pitch, n, batch, type, norm, _prec(dtype), 1 if no_fusion else 0, info)
    if rc == 0 and info[0] == 1:
        assert info[1] == 1, list(info)  # ONE launch per fused execute
    return rc, info[0]


def run_plan2d(rows, cols, M, type, norm, dtype, in_ptr, in_pitch, out_ptr, out_pitch, no_fusion=False):
    return ED.dct2d(in_ptr, in_pitch, out_ptr, out_pitch, rows, cols, M, type, norm, _prec(dtype), no_fusion)


def test_reference_against_scipy():
    """the float64 numpy reference of the ladder is scipy.fft's dct / dst / idct / idst, both of its branches (matrix and 2N extension)"""
    sf = pytest.importorskip("scipy.fft")
    x = np.random.default_rng(0).standard_normal((2, 100))
    for n in (1, 2, 9, 64, 100):
        for t, f, ty in ((L.DCT2, sf.dct, 2), (L.DCT3, sf.dct, 3), (L.DST2, sf.dst, 2), (L.DST3, sf.dst, 3)):
            for norm, name in ((L.NONE, None), (L.ORTHO, "ortho")):
                assert np.max(np.abs(L.reference(x[:, :n], t, norm) - f(x[:, :n], type=ty, norm=name))) < 1e-12, (n, t, norm)
        assert np.max(np.abs(L.reference(x[:, :n], L.DCT3, L.INVERSE) - sf.idct(x[:, :n], type=2))) < 1e-12
        assert np.max(np.abs(L.reference(x[:, :n], L.DST2, L.INVERSE) - sf.idst(x[:, :n], type=3))) < 1e-12
    y = np.random.default_rng(1).standard_normal((2, 5, 9))
    assert np.max(np.abs(L.reference2d(y, L.DCT2, L.ORTHO) - sf.dctn(y, type=2, norm="ortho", axes=(-2, -1)))) < 1e-12


def _cases(cases):
    return [pytest.param(c, dt, id="%s-%s" % (c, "fp32" if dt == L.F32 else "fp64")) for c in cases for dt in c.dtypes]


@pytest.mark.parametrize("type", L.TYPES, ids=[L.TYPE_NAMES[t] for t in L.TYPES])
@pytest.mark.parametrize("case,dt", _cases(L.FUSED + L.FALLBACK))
def test_cases(case, dt, type):
    """every shape of the ladder: the case's norms, the plan's own path and NO_FUSION"""
    L.check_case(run_plan, case, dt, type)


def test_tile_rows_of_the_batch_cases():
    """the batch cases n16-batch129 / -batch257 are one tile plus one row: the tile of a large batch at N = 16 is 128 (fp64) / 256 (fp32) rows"""
    info = (ED.C.c_int * 4)()
    for dt, rows in ((L.F32, 256), (L.F64, 128)):
        x = np.zeros((rows + 1, 16), dtype=dt)
        assert ED.lib().emu_dct(x.ctypes.data, 0, x.ctypes.data, 0, 16, rows + 1, 0, 0, _prec(dt), 0, info) == 0
        assert list(info)[:3] == [1, 1, rows], list(info)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("type", (L.DCT2, L.DST3), ids=["dct2", "dst3"])
@pytest.mark.parametrize("case", L.CASES_2D, ids=repr)
def test_2d(case, type, dt):
    L.check_2d(run_plan2d, case, dt, type, L.ORTHO if case.name == "8x16" else L.NONE)
    L.check_2d(run_plan2d, case, dt, type, L.NONE, no_fusion=True)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("type", L.TYPES, ids=[L.TYPE_NAMES[t] for t in L.TYPES])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_impulses_and_linear_operator(type, dt, no_fusion):
    L.check_impulses(run_plan, dt, type, no_fusion=no_fusion)
    L.check_linear_operator(run_plan, dt, type, no_fusion=no_fusion)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("sine", (False, True), ids=["dct", "dst"])
@pytest.mark.parametrize("n", (64, 12))
def test_identities(n, sine, dt):
    L.check_identities(run_plan, dt, sine, n=n)


def test_refusals():
    """every -1 / -2 condition: nothing is launched"""
    x = np.zeros(3 * 20, dtype=np.float32)
    y = np.full(3 * 20, 7, dtype=np.float32)

    def go(n=16, batch=3, type=0, norm=0, ip=20, op=20, iptr=x.ctypes.data, optr=y.ctypes.data):
        info = (ED.C.c_int * 4)()
        return ED.lib().emu_dct(iptr, ip, optr, op, n, batch, type, norm, 1, 0, info)

    assert go() == 0
    y[:] = 7
    assert go(n=0) == -1 and go(batch=0) == -1 and go(type=4) == -1 and go(type=-1) == -1 and go(norm=3) == -1 and go(norm=-1) == -1
    assert go(n=1 << 20, batch=1 << 12) == -1      # n batch > 2^31 - 1
    assert go(ip=15) == -2 and go(op=15) == -2     # a pitch smaller than the row
    assert go(iptr=None) == -2 and go(optr=None) == -2
    assert np.all(y == 7)
    assert ED.dct2d(x.ctypes.data, 0, y.ctypes.data, 0, 0, 4, 1, 0, 0, 1)[0] == -1
    assert ED.dct2d(x.ctypes.data, 15, y.ctypes.data, 0, 4, 4, 1, 0, 0, 1)[0] == -2
    assert np.all(y == 7)


def test_memory_safety_under_asan(tmp_path):
    """tests/emu/emu_dct_main.cpp, built with -fsanitize=address,undefined: the fused and the fallback path, all four types, 1D and 2D, on
    exactly sized heap buffers at element-aligned bases, a clean exit.  (Most of its time is the compile of the engine with the
    sanitizers.)"""
    exe = str(tmp_path / "emu_dct_main")
    subprocess.run(["g++", "-O0", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-I" + ED.CSRC, os.path.join(ED.EMU_DIR, "emu_dct_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(r.stdout[-3000:])
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0 and "all cases passed" in r.stdout
