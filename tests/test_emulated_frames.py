"""The plans on overlapping frames (STFT, spectrogram, Welch: csrc/fft_plans_ext.h FramesPlan) in the CPU emulation: the unmodified
kernel source -- the framed load and the one-sided power store of tile_fft_kernel, frames_mean_kernel -- at the cases of
tests/frames_ladder.py, every frame against float64, between guards, with NaN in every sample no frame covers."""
import numpy as np
import pytest

import accuracy as A
import emu_frames_lib as EF
import frames_ladder as L


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", L.HostMemory())


def _prec(dt):
    return 1 if np.dtype(dt) == L.C64 else 0


def _run_case(case, kind, dt, lds_budget=0, no_fusion=False, fused=1, passes=1):
    """check() of one plan; asserts the path it took.  Returns (rows, info)."""
    seen = []

    def run(x_ptr, pitch, out_ptr):
        rc, info = EF.frames(x_ptr, out_ptr, case.n, case.hop, case.signal_len, case.n_signals, pitch, case.window, L.user_window(case, dt),
                             kind, _prec(dt), lds_budget, no_fusion, L.FS)
        assert rc == 0, rc
        seen.append(info)

    y = L.check(run, case, kind, dt)
    info = seen[0]
    assert info[2] == case.nw
    assert info[1] == fused and (passes is None or info[0] == passes), info
    if fused:  # one launch carries load, window, transform and store; Welch adds the mean
        assert info[3] == (2 if kind == L.WELCH else 1), info
    return y, info


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.SMALL, ids=repr)
def test_small_cases(case, dt):
    """(a) - (e), (h), (j)"""
    for kind in case.kinds:
        y, info = _run_case(case, kind, dt)
        if case.name in ("a", "b", "c"):  # tiles of 64 (fp32) / 32 (fp64) frames: every tile straddles signals, the last one is ragged
            assert info[4] == (64 if dt == L.C64 else 32) and (case.n_signals * case.nw) % info[4] != 0 and info[4] % case.nw != 0


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", L.EMU_F, ids=repr)
def test_single_pass_frame(case, dt):
    """(f) at n = 256"""
    for kind in case.kinds:
        _run_case(case, kind, dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case,budget,passes", L.EMU_G, ids=lambda v: repr(v))
def test_multi_pass_fallback(case, budget, passes, dt):
    """(g): a core of two / three passes runs the per-signal fallback"""
    for kind in case.kinds:
        _run_case(case, kind, dt, lds_budget=budget, fused=0, passes=passes)


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_welch_of_one_frame_is_the_periodogram(dt):
    """(i): WELCH with nw = 1, hop = n, Hann equals FUSED_PSD of the same rows to within the bound"""
    case = L.Case("i", 64, 64, 5, 1, kinds=(L.WELCH,))
    x = L.make_input(case, dt)
    y, _ = _run_case(case, L.WELCH, dt)
    p = EF.psd(x[:, :case.n], L.FS)
    e, k = A.row_errors(y, p.astype(np.float64), scale="rms_or_bin")
    A.assert_within(e, k, L.bound(L.WELCH, dt, case.n), "welch(nw = 1) vs FUSED_PSD")


@pytest.mark.parametrize("dt", L.BOTH, ids=["fp32", "fp64"])
def test_no_fusion_on_case_a(dt):
    """(k): the unfused path on (a), within the same bound"""
    for kind in L.CASE_A.kinds:
        _run_case(L.CASE_A, kind, dt, no_fusion=True, fused=0)


def test_unaligned_signals_on_the_fallback():
    """(c) with no_fusion: signals that do not start 16-byte aligned take the value-by-value kernels"""
    case = next(c for c in L.SMALL if c.name == "c")
    _run_case(case, L.POWER, L.C64, no_fusion=True, fused=0)


def test_refusals():
    """(l): bad arguments are refused before anything is launched"""
    x = np.zeros((2, 256), dtype=np.complex64)
    out = np.zeros((2 * 16, 64), dtype=np.complex64)
    args = dict(n_signals=2, signal_pitch=256, window=L.HANN, w_host=None, kind=L.STFT, prec=1)
    good = dict(n=64, hop=16, signal_len=128)
    assert EF.frames(x.ctypes.data, out.ctypes.data, **good, **args)[0] == 0
    for bad in (dict(hop=0), dict(hop=65), dict(n=100, hop=16), dict(signal_len=63), dict(n=1, hop=1)):
        assert EF.frames(x.ctypes.data, out.ctypes.data, **{**good, **bad}, **args)[0] == -1, bad
    assert EF.frames(x.ctypes.data, out.ctypes.data, **good, **{**args, "window": L.USER})[0] == -1  # USER without values
    before = x.copy()
    assert EF.frames(x.ctypes.data, x.ctypes.data, **good, **args)[0] == -2  # d_out == d_x
    assert np.array_equal(x, before)
