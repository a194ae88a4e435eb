"""The inverse STFT plan (csrc/fft_plans_ext.h IFramesPlan) in the CPU emulation: the unmodified kernel source -- the Hermitian rows
load of tile_fft_kernel (HOOK bit 7), iframes_merge_kernel, frames_overlap_add_kernel -- at the cases of tests/iframes_ladder.py,
every sample of every signal against float64, the output pre-filled with a NaN pattern between guards."""
import numpy as np
import pytest

import accuracy as A
import emu_iframes_lib as EI
import frames_ladder as L
import iframes_ladder as R


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", L.HostMemory())


def _prec(dt):
    return 1 if np.dtype(dt) == R.F32 else 0


def _runner(case, dt, seen, lds_budget=0, no_fusion=False):
    def run(X_ptr, y_ptr, pitch):
        rc, info = EI.iframes(X_ptr, y_ptr, case.n, case.hop, case.nw, case.n_signals, pitch, case.window, R.user_window(case, dt),
                              _prec(dt), lds_budget, no_fusion)
        assert rc == 0, rc
        seen.append(info)
    return run


def _run_case(case, dt, lds_budget=0, no_fusion=False, fused=1, passes=1, X=None, expected=None):
    """check() of one plan; asserts the path it took.  Returns (signals, info)."""
    seen = []
    y, lost = R.check(_runner(case, dt, seen, lds_budget, no_fusion), case, dt, X=X, expected=expected,
                      family="iframes" if fused else "iframes_fallback")
    info = seen[0]
    assert info[2] == case.out_len and info[5] == lost, info
    assert info[1] == fused and (passes is None or info[0] == passes), info
    if info[1]:  # one launch carries load, merge, transform and store; the overlap-add is the second
        assert info[3] == 2, info
    else:  # merge, the core's passes, overlap-add
        assert info[3] >= 3, info
    return y, info


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.SMALL, ids=repr)
def test_small_cases(case, dt):
    # (n = 4: a core of length 2 has no hooked kernel, the plan takes its fallback)
    y, info = _run_case(case, dt, passes=None, fused=0 if case.n == 4 else 1)
    if case.name == "a":  # tiles of 64 (fp32) / 32 (fp64) frames: tiles straddle signals, the last one is ragged
        assert info[4] == (64 if dt == R.F32 else 32) and (case.n_signals * case.nw) % info[4] != 0 and info[4] % case.nw != 0
    if case.name == "h-hann":
        assert info[5] == 2 and np.all(y[:, 0] == 0) and np.all(y[:, -1] == 0)
    if case.name == "h-rect":
        assert info[5] == 0


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_edge_bin_imaginary_parts_are_ignored(dt, no_fusion):
    R.check_edge_bins_ignored(_runner(R.CASE_A, dt, [], no_fusion=no_fusion), R.CASE_A, dt)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("no_fusion", (False, True), ids=["fused", "fallback"])
def test_a_nan_frame_poisons_exactly_its_samples(dt, no_fusion):
    R.check_nan_frame(_runner(R.CASE_A, dt, [], no_fusion=no_fusion), R.CASE_A, dt)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_impulses_against_the_closed_form(dt):
    X, y = R.impulse_spectra(R.IMPULSES, dt)
    _, limit, scale, lost = R.reference(R.IMPULSES, X, dt)
    _run_case(R.IMPULSES, dt, X=X, expected=(y, limit, scale, lost))


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.ROUND_TRIPS, ids=repr)
def test_round_trip(case, dt):
    """istft(stft(x)) against x; the forward leg is the real frames plan"""
    x = R.round_trip_input(case, dt)
    X = np.empty((case.n_signals, case.nw, case.bins), dtype=R.complex_dtype(dt))
    assert EI.rstft(x.ctypes.data, X.ctypes.data, case.n, case.hop, case.out_len, case.n_signals, case.window, None, _prec(dt)) == 0
    _run_case(case, dt, X=X, expected=R.round_trip_expected(case, x, dt))


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", R.EMU_F, ids=repr)
def test_one_launch_path_at_512(case, dt):
    _run_case(case, dt)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case,budget,passes", R.EMU_G, ids=lambda v: repr(v))
def test_multi_pass_fallback(case, budget, passes, dt):
    _run_case(case, dt, lds_budget=budget, fused=0, passes=passes)


@pytest.mark.parametrize("dt", R.BOTH, ids=["fp32", "fp64"])
def test_no_fusion_agrees_with_the_fused_path(dt):
    """the unfused path on (a) within the bound of float64, and within twice the bound of the fused signals"""
    case = R.CASE_A
    a, _ = _run_case(case, dt, no_fusion=True, fused=0)
    b, _ = _run_case(case, dt)
    _, limit, scale, _ = R.reference(case, R.make_spectra(case, dt), dt)
    R.sample_check(a, b.astype(np.float64), 2 * limit, scale, case, dt, "no_fusion vs fused")


def test_refusals():
    """bad arguments are refused before anything is launched"""
    X = np.zeros((2 * 5, 33), dtype=np.complex64)
    y = np.full((2, 128), 7.0, dtype=np.float32)
    args = dict(signal_pitch=0, window=R.HANN, w_host=None, prec=1)
    good = dict(n=64, hop=16, n_frames=5, n_signals=2)
    assert EI.iframes(X.ctypes.data, y.ctypes.data, **good, **args)[0] == 0
    for bad in (dict(n=2, hop=1), dict(n=96), dict(n=0), dict(hop=0), dict(hop=65), dict(n_frames=0), dict(n_signals=0),
                dict(n_frames=65536, n_signals=65536), dict(n=1 << 20, n_frames=1 << 21, n_signals=1)):
        assert EI.iframes(X.ctypes.data, y.ctypes.data, **{**good, **bad}, **args)[0] == -1, bad
    assert EI.iframes(X.ctypes.data, y.ctypes.data, **good, **{**args, "window": R.USER})[0] == -1  # USER without values
    y[:] = 7.0
    assert EI.iframes(X.ctypes.data, y.ctypes.data, **good, **{**args, "signal_pitch": 127})[0] == -2  # pitch < out_len
    assert EI.iframes(None, y.ctypes.data, **good, **args)[0] == -2
    assert EI.iframes(X.ctypes.data, None, **good, **args)[0] == -2
    assert np.all(y == 7.0)
    before = X.copy()
    assert EI.iframes(X.ctypes.data, X.ctypes.data, **good, **args)[0] == -2  # d_y == d_X
    assert np.array_equal(X, before)
