"""The frames plans on REAL signals (csrc/fft_plans_ext.h FramesPlan with real_input) in the CPU emulation: the unmodified kernel
source -- the packed real load and the r2c split in the store of tile_fft_kernel (HOOK bit 6), frames_pack_real_kernel,
psd_onesided_rows_kernel -- at the cases of tests/rframes_ladder.py, every row against float64, between guards, with NaN in every
sample no frame covers."""
import numpy as np
import pytest

import accuracy as A
import emu_rframes_lib as ER
import frames_ladder as L
import rframes_ladder as R


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", L.HostMemory())


def _prec(dt):
    return 1 if np.dtype(dt) == R.F32 else 0


def _runner(case, kind, dt, seen, lds_budget=0, no_fusion=False):
    def run(x_ptr, pitch, out_ptr):
        rc, info = ER.rframes(x_ptr, out_ptr, case.n, case.hop, case.signal_len, case.n_signals, pitch, case.window, R.user_window(case, dt),
                              kind, _prec(dt), lds_budget, no_fusion, R.FS)
        assert rc == 0, rc
        seen.append(info)
    return run


def _run_case(case, kind, dt, lds_budget=0, no_fusion=False, fused=1, passes=1, offset=0, x=None, expected=None):
    """check() of one plan; asserts the path it took.  Returns (rows, info)."""
    seen = []
    y = R.check(_runner(case, kind, dt, seen, lds_budget, no_fusion), case, kind, dt, offset=offset, x=x, expected=expected)
    info = seen[0]
    assert info[2] == case.nw
    assert (fused is None or info[1] == fused) and (passes is None or info[0] == passes), info
    if info[1]:  # one launch carries load, window, transform, split and store; Welch adds the mean
        assert info[3] == (2 if kind == R.WELCH else 1), info
        assert info[5] == (1 if R.vec_loads_allowed(case, dt, offset) else 0), ("in_vec_ok", case, info)
    else:  # pack, the core's passes, split (+ power) (+ mean)
        assert info[5] == -1 and info[3] >= 3, info
    return y, info


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.SMALL, ids=repr)
def test_small_cases(case, dt):
    for kind in case.kinds:
        # (n = 4: a core of length 2 has no hooked kernel, the plan takes its fallback -- fused where round_capable() holds)
        y, info = _run_case(case, kind, dt, passes=None, fused=0 if case.n == 4 else 1)
        if case.name == "a":  # tiles of 64 (fp32) / 32 (fp64) frames: every tile straddles signals, the last one is ragged
            assert info[4] == (64 if dt == R.F32 else 32) and (case.n_signals * case.nw) % info[4] != 0 and info[4] % case.nw != 0
        if case.name in ("c-pad1", "b-hop15") or (case.name in ("c-pad2", "b-hop18") and dt == R.F32):
            assert info[5] == 0, info


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_input_one_real_off_a_16_byte_boundary(dt):
    for kind in R.OFFSET_CASE.kinds:
        y, info = _run_case(R.OFFSET_CASE, kind, dt, offset=1)
        assert info[5] == 0, info


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_impulses_against_the_closed_form(dt):
    """frame w = a unit impulse at sample w: row w is W_n^(w k), which separates even / odd packing and twiddle-sign errors"""
    x, X = R.impulse_input(R.IMPULSES, dt)
    _run_case(R.IMPULSES, R.STFT, dt, x=x, expected=X)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.EMU_F, ids=repr)
def test_one_launch_path_at_512(case, dt):
    for kind in case.kinds:
        _run_case(case, kind, dt)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case,budget,passes", R.EMU_G, ids=lambda v: repr(v))
def test_multi_pass_fallback(case, budget, passes, dt):
    for kind in case.kinds:
        _run_case(case, kind, dt, lds_budget=budget, fused=0, passes=passes)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_no_fusion_on_case_a(dt):
    """the unfused path on (a), within the same bound; also with signals that start at odd reals"""
    for kind in R.CASE_A.kinds:
        _run_case(R.CASE_A, kind, dt, no_fusion=True, fused=0)
    _run_case(next(c for c in R.SMALL if c.name == "c-pad1"), R.POWER, dt, no_fusion=True, fused=0)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_rows_equal_the_complex_plan_on_a_zero_imaginary_part(dt):
    case = R.CASE_A
    cdt = R.complex_dtype(dt)
    for kind in case.kinds:
        def run_complex(x_ptr, pitch, out_ptr):
            rc, _ = ER.cframes(x_ptr, out_ptr, case.n, case.hop, case.signal_len, case.n_signals, pitch, case.window, None, kind,
                               1 if cdt == L.C64 else 0, 0, False, R.FS)
            assert rc == 0
        R.check_consistency(_runner(case, kind, dt, []), run_complex, case, kind, dt)


def test_refusals():
    """bad arguments are refused before anything is launched"""
    x = np.zeros((2, 256), dtype=np.float32)
    out = np.zeros((2 * 16, 33), dtype=np.complex64)
    args = dict(n_signals=2, signal_pitch=256, window=R.HANN, w_host=None, kind=R.STFT, prec=1)
    good = dict(n=64, hop=16, signal_len=128)
    assert ER.rframes(x.ctypes.data, out.ctypes.data, **good, **args)[0] == 0
    for bad in (dict(n=2, hop=1), dict(n=96, hop=16), dict(hop=0), dict(hop=65), dict(signal_len=63)):
        assert ER.rframes(x.ctypes.data, out.ctypes.data, **{**good, **bad}, **args)[0] == -1, bad
    assert ER.rframes(x.ctypes.data, out.ctypes.data, **good, **{**args, "window": R.USER})[0] == -1  # USER without values
    assert ER.rframes(x.ctypes.data, out.ctypes.data, **good, **{**args, "signal_pitch": 127})[0] == -2  # pitch < signal_len
    before = x.copy()
    assert ER.rframes(x.ctypes.data, x.ctypes.data, **good, **args)[0] == -2  # d_out == d_x
    assert np.array_equal(x, before)
