"""The cross frames plans (csrc/fft_plans_ext.h CrossFramesPlan) in the CPU emulation: the unmodified plan and kernel source --
the inner frames plan in STFT mode, frames_cross_partial_kernel, frames_cross_finish_kernel -- at the cases of tests/cross_ladder.py:
every bin of Pxx, Pyy, Pxy, coherence and H1 against float64 numpy, everything between guards, NaN in every sample no frame covers.
The reference project's compute_coherence is no oracle (it writes 1.0 into every bin); the oracle is cross_ladder.reference."""
import numpy as np
import pytest

import accuracy as A
import cross_ladder as X
import emu_cross_lib as EC
import frames_ladder as L


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", L.HostMemory())


def _prec(dt):
    return 1 if X.real_dtype(dt) == X.F32 else 0


class Emu:
    """cross_ladder's backend on the emulation."""

    def __init__(self, lds_budget=0):
        self.lds_budget = lds_budget

    def run(self, case, kind, dt, x_ptr, x_pitch, y_ptr, y_pitch, out_ptrs, no_fusion=False, max_grid=0, block=0):
        rc, info = EC.cross(x_ptr, x_pitch, y_ptr, y_pitch, out_ptrs[0], case.n, case.hop, case.signal_len, case.n_signals, case.window,
                            X.user_window(case, dt), kind, X.is_real(dt), _prec(dt), self.lds_budget, no_fusion, max_grid, block, X.FS,
                            out2_ptr=out_ptrs[1] if len(out_ptrs) > 1 else None)
        assert rc == 0, rc
        hb = case.hb
        # two inner executes and the two reduction kernels; the partial sums stay a small fraction of the rows they sum up
        assert info["launches"] >= 4 and info["part_bytes"] == case.n_signals * info["chunks"] * hb * 32
        assert info["rows_bytes"] == case.n_signals * case.nw * (hb if X.is_real(dt) else case.n) * 2 * X.real_dtype(dt).itemsize
        return info

    def welch(self, case, dt, x_ptr, pitch, out_ptr):
        assert EC.welch(x_ptr, out_ptr, case.n, case.hop, case.signal_len, case.n_signals, pitch, case.window, X.user_window(case, dt),
                        X.is_real(dt), _prec(dt), X.FS) == 0


EMU = Emu()
ALL_DT = pytest.mark.parametrize("dt", X.DTYPES, ids=X.dtype_id)


def test_the_coherence_bound_is_not_vacuous():
    """A condition on the inputs, from the float64 reference alone: the propagated coherence bound stays below 1e-2 in fp32 at every
    bin of every case (the fp64 bound is 2^-29 of it), and the coherence itself away from 0 and 1."""
    for case in X.SMALL + X.BIG + [X.IDENT, X.OFFSET_CASE]:
        for dt in case.dtypes:
            x, y = X.make_pair(case, dt)
            ref = X.reference(case, x, y, dt)
            b = X.coherence_bound(case, X.F32 if X.is_real(dt) else X.C64, ref)
            assert np.all(np.isfinite(b)) and float(np.max(b)) < 1e-2, (case, X.dtype_id(dt), float(np.max(b)))
            if case.nw >= 30:
                c = X.coherence_ref(ref)
                assert 0.1 < float(np.min(c)) and float(np.max(c)) < 0.99, (case, float(np.min(c)), float(np.max(c)))


def test_chunk_rule():
    """C = max(32, ceil(nw / ceil(2^18 / (S hb)))): a function of (nw, S, hb) alone; S * chunks * hb reaches about 2^18 threads for
    few long signals, and the partial sums stay below 1/16 (fp32) of the rows."""
    for nw, S, hb in ((1, 1, 3), (31, 2, 5), (32, 2, 5), (33, 2, 5), (75, 2, 5), (524287, 1, 513), (524287, 8, 513), (100000, 1, 8193),
                      (2000000, 1, 33), (4000, 64, 513)):
        C = EC.chunk_len(nw, S, hb)
        assert C == X.chunk_rule(nw, S, hb), (nw, S, hb, C)
        chunks = -(-nw // C)
        assert C >= 32 and S * chunks * hb <= (1 << 18) + S * hb
        if nw >= 32 * (1 << 18) // (S * hb):  # enough frames: the device is filled
            assert S * chunks * hb >= (1 << 17), (nw, S, hb, chunks)
    assert EC.chunk_len(524287, 1, 513) == 1024  # S = 1, n = 1024, hop = 512, 2^28 samples: 512 chunks, 262656 threads


@pytest.mark.parametrize("case,dt", [(c, dt) for c in X.SMALL for dt in c.dtypes], ids=lambda v: v.name if isinstance(v, X.Case) else X.dtype_id(v))
def test_small_cases(case, dt):
    info = X.run_case(EMU, case, dt)
    assert info["fused"] == (0 if (case.n == 4 and X.is_real(dt)) else 1), info
    assert info["C"] == 32 and info["chunks"] == {31: 1, 32: 1, 33: 2, 75: 3}.get(case.nw, 1)


@pytest.mark.parametrize("case", X.BIG, ids=repr)
def test_one_step_past_the_one_launch_range(case):
    """n = 16384 fp32 / 8192 and 16384 fp64, real signals: on the device the inner plan's pack, multi-pass core and split at 16384.
    (The emulation's LDS budget holds the fp64 cores in one pass, so only the fp32 case takes the fallback here; the fallback with a
    multi-pass core in fp64 is test_fallback_with_a_multi_pass_core.)"""
    info = X.run_case(EMU, case, case.dtypes[0])
    if case.dtypes[0] == X.F32:
        assert info["fused"] == 0 and info["passes"] >= 2, info


@ALL_DT
def test_bases_one_element_off_a_16_byte_boundary(dt):
    X.check_all(EMU, X.OFFSET_CASE, dt, offset=1)
    X.check_kind(EMU, X.OFFSET_CASE, X.COHERENCE, dt, offset=1)


@ALL_DT
def test_no_fusion(dt):
    X.identity_no_fusion(EMU, dt)


@ALL_DT
def test_fallback_with_a_multi_pass_core(dt):
    """an LDS budget that gives the inner core two passes at n = 512"""
    case = X.Case("g-2pass", 512, 256, 2, 3)
    _, info = X.check_all(Emu(lds_budget=4096), case, dt)
    assert info["fused"] == 0 and info["passes"] == 2, info


@ALL_DT
def test_a_signal_with_itself(dt):
    X.identity_same_pointer(EMU, dt)


@ALL_DT
def test_a_signal_and_its_double(dt):
    X.identity_doubled(EMU, dt)


@ALL_DT
def test_swapped_pair_gives_the_conjugate(dt):
    X.identity_swap(EMU, dt)


@ALL_DT
def test_one_frame_is_fully_coherent(dt):
    X.identity_one_frame(EMU, dt)


@ALL_DT
def test_pxx_is_the_welch_plans(dt):
    X.identity_welch(EMU, dt)


@ALL_DT
def test_zero_power(dt):
    X.identity_zero_x(EMU, dt)


@pytest.mark.parametrize("dt", (X.F32, X.C128), ids=X.dtype_id)
def test_a_poisoned_pair_stays_alone(dt):
    X.identity_poisoned_pair(EMU, dt)


@pytest.mark.parametrize("dt", (X.F32, X.F64), ids=X.dtype_id)
def test_results_do_not_depend_on_the_launch_geometry(dt):
    """256-thread workgroups on the default grid, 64-thread workgroups on a grid of 3, one workgroup of 32 threads: bit-identical"""
    case = next(c for c in X.SMALL if c.name == "chunk-75")
    x, y = X.make_pair(case, dt)
    for kind in (X.ALL, X.COHERENCE):
        a, _ = X.execute(EMU, case, kind, dt, x, y)
        for max_grid, block in ((3, 64), (1, 32)):
            b, _ = X.execute(EMU, case, kind, dt, x, y, max_grid=max_grid, block=block)
            assert X.bits_equal(a, b), (X.KIND_NAMES[kind], max_grid, block)


def test_refusals():
    """bad arguments are refused before anything is launched"""
    x = np.random.default_rng(1).standard_normal((2, 256)).astype(np.float32)
    out = np.zeros((2, 33 * 4), dtype=np.float32)
    args = dict(n_signals=2, window=X.HANN, w_host=None, kind=X.ALL, real_input=True, prec=1)
    good = dict(n=64, hop=16, signal_len=128)

    def go(xp, xpitch, yp, ypitch, op, **kw):
        return EC.cross(xp, xpitch, yp, ypitch, op, **{**good, **args, **kw})[0]

    xp, op = x.ctypes.data, out.ctypes.data
    assert go(xp, 256, xp, 256, op) == 0
    for bad in (dict(n=96), dict(n=2, hop=1), dict(hop=0), dict(hop=65), dict(signal_len=63), dict(window=X.USER), dict(kind=4), dict(kind=-1)):
        assert go(xp, 256, xp, 256, op, **bad) == -1, bad
    assert go(xp, 128, xp, 128, op, n=2, hop=1, real_input=False) == 0  # n = 2 is a complex plan's smallest
    before, was = x.copy(), out.copy()
    for a in ((None, 256, xp, 256, op), (xp, 256, None, 256, op), (xp, 256, xp, 256, None), (xp, 127, xp, 256, op), (xp, 256, xp, 127, op),
              (xp, 256, xp, 256, xp), (xp, 256, xp + 4 * 256, 128, xp + 4 * 300)):  # NULLs, short pitches, an output that is / overlaps an input
        assert go(*a) == -2, a
    assert np.array_equal(x, before) and np.array_equal(out, was)
