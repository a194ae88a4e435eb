"""Every path as a linear operator, in the CPU emulation (tests/emu: the unmodified planner and kernel source), at the cases of
tests/operator_ladder.py and the sizes the emulation reaches.

A. unit impulses against the closed-form column of the DFT matrix, through accuracy.check_execute / check_execute_io on host memory
   (guards, untouched input, in place bit-identical); accuracy.check_rows prints each case's worst e / (u log2 n) before it asserts; each case asserts its path.
B. a poisoned transform (NaN / one Inf / overflowing values) leaves every other transform of the batch bit-identical.
C. execute(2^s x) == 2^s execute(x) bit for bit; zeros in, zeros out."""
import ctypes as C

import numpy as np
import pytest

import accuracy as A
import emu_frames_lib as EF
import emu_lib as E
import emu_mixed_ext_lib as EMX
import emu_mixed_lib as EM
import ext_ladder as XL
import frames_ladder as FL
import operator_ladder as L
import single_pass_ladder as SL

ALGO = {"auto": 0, "radix2": 1, "radix4": 2, "split_radix": 3, "radix2_global": 4, "radix2_shfl": 6}
DT_IDS = ["fp32", "fp64"]


@pytest.fixture(autouse=True)
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", FL.HostMemory())


def _prec(dt):
    return 1 if np.dtype(dt) in (L.C64, L.F32) else 0


def _js(n, factors=(), every=L.EMU_ALL_IMPULSES):
    return L.positions(n, factors, every=every)


def _inplace(rows, n):
    """The in-place rerun (bit-identical to out of place) only where the batch is small: above 2^18 points it would double the
    emulation's time, and in place is covered at these sizes by tests/test_emulated_kernels.py and on the device."""
    return rows * n <= 1 << 18


class EmuPlan:
    """A raw-pointer plan of the emulation for accuracy.check_execute: call(in_ptr, out_ptr, info) -> rc."""

    def __init__(self, call, direction):
        self.call, self.direction, self.info = call, direction, None

    def execute_ptr(self, d_in, d_out):
        info = (C.c_int * 8)()
        assert self.call(d_in, d_out, info) == 0, "the emulated plan was refused"
        self.info = list(info)

    def sync(self):
        return 0


def _fft(n, batch, d, dt, algo=0, lds=0):
    return EmuPlan(lambda i, o, info: E.lib().emu_fft(i, o, n, batch, d, _prec(dt), algo, lds, info), d)


def _team(monkeypatch, n, batch, d, dt, log2seats, n_xcc, threads, lds, tiles=4):
    monkeypatch.setenv("FFT_HIP_TEAM", "2")  # every size, any batch (as emu_lib.emu_fft_team)
    monkeypatch.setenv("FFT_HIP_TEAM_TILES", str(tiles))
    mode = (log2seats + 1) | (n_xcc << 4) | (threads << 8)
    return EmuPlan(lambda i, o, info: E.lib().emu_fft_team(i, o, n, batch, d, _prec(dt), lds, mode, info), d)


def _mixed(n, batch, d, dt, lds=0):
    return EmuPlan(lambda i, o, info: EM.lib().emu_mixed(i, o, n, batch, d, _prec(dt), lds, info), d)


def _impulse_1d(make, n, dt, family, expect, label, m=None, factors=(), every=L.EMU_ALL_IMPULSES):
    """Both directions of one 1D plan family on the impulses of n."""
    js = _js(n, factors, every)
    inplace = _inplace(len(js), m or n)
    x = L.impulses(n, js, dt)
    for d in (-1, 1):
        plan = make(len(js), d)
        L.closed_form_checked(L.ref_1d(n, d), L.ref_1d(n, d, np.longdouble), x, family, dt, n, m, label=label)
        A.check_execute(plan, x, family, m=m, ref=L.ref_1d(n, d), kind="impulse", inplace=inplace,
                        expect=lambda: expect(plan.info), label="%s n=%d dir=%+d" % (label, n, d))


# ---------------------------------------------------------------------------------------------------------------------------
# A. impulses
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n", L.SINGLE_PASS_AUTO)
def test_impulses_single_pass_auto(n, dt):
    def expect(info):
        assert info[0] == 1 and info[1] == n.bit_length() - 1, info
    _impulse_1d(lambda b, d: _fft(n, b, d, dt, 0, SL.LDS_BUDGET), n, dt, "multipass", expect, "single pass auto")


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("algo,n", L.SINGLE_PASS_EXPLICIT, ids=str)
def test_impulses_explicit_families(algo, n, dt):
    family = algo if algo in ("radix2_global", "radix2_shfl") else "multipass"

    def expect(info):
        if algo in ("radix2_global", "radix2_shfl"):  # their own kernels: the plan holds no tile pass and runs the batch as one chunk
            assert info[0] == 0 and info[7] == len(_js(n)) and not info[6], info
        else:
            assert info[0] == 1 and info[1] == n.bit_length() - 1, info
    _impulse_1d(lambda b, d: _fft(n, b, d, dt, ALGO[algo], SL.LDS_BUDGET), n, dt, family, expect, algo)


def test_impulses_wide_row(monkeypatch):
    """wide_row_kernel in its emulated shape (n = 512 fp32, FFT_EMU_WIDE)."""
    monkeypatch.setenv("FFT_EMU_WIDE", "1")

    def expect(info):
        assert info[6] & 16, "wide_row_kernel was not planned"
    _impulse_1d(lambda b, d: _fft(512, b, d, L.C64), 512, L.C64, "wide_row", expect, "wide row")


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n,lds,passes", L.EMU_MULTIPASS)
def test_impulses_multi_pass(n, lds, passes, dt):
    def expect(info):
        assert info[0] == passes, info
    _impulse_1d(lambda b, d: _fft(n, b, d, dt, 0, lds), n, dt, "multipass", expect, "%d passes" % passes)


TEAM_DEFER = [(4096, L.C64, 2, 2, 16, 16384), (2048, L.C64, 2, 2, 16, 8192), (2048, L.C128, 2, 3, 16, 16384)]
TEAM_QUAD = [(4096, 2, 2, 64, 8192), (1024, 1, 2, 32, 4096), (2048, 2, 2, 32, 4096)]


@pytest.mark.parametrize("n,dt,log2seats,n_xcc,threads,lds", TEAM_DEFER, ids=str)
def test_impulses_team_kernel(n, dt, log2seats, n_xcc, threads, lds, monkeypatch):
    """The sampled positions (every workgroup of the emulated grid is a set of host threads that spin at the team barriers)."""
    def expect(info):
        assert info[0] // 100 == 4 and info[5] == 1, info
    _impulse_1d(lambda b, d: _team(monkeypatch, n, b, d, dt, log2seats, n_xcc, threads, lds), n, dt, "team_defer", expect, "team", every=0)


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n,log2seats,n_xcc,threads,lds", TEAM_QUAD, ids=str)
def test_impulses_team_quad_kernel(n, log2seats, n_xcc, threads, lds, dt, monkeypatch):
    monkeypatch.setenv("FFT_EMU_TEAM_QUAD", "1")

    def expect(info):
        assert info[0] // 100 == 4 and info[6] & 8 and info[5] == 1, info
    _impulse_1d(lambda b, d: _team(monkeypatch, n, b, d, dt, log2seats, n_xcc, threads, lds * (2 if dt == L.C128 else 1)), n, dt,
                "team_quad", expect, "team quad", every=0)


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n", L.MIXED_ALL + L.MIXED_SAMPLED[:2])
def test_impulses_mixed_radix(n, dt):
    """Every impulse at every single-pass length of the ladder (6 ... 4050); 4200 and 44100 run two passes at the sampled positions."""
    passes = 1 if n <= 4096 else 2
    seen = {}

    def expect(info):
        assert info[0] == EM.KIND_MIXED and info[1] == passes, info
        seen["f"] = info[2:4]
    js = L.positions(n) if passes == 1 else None
    if js is None:
        probe = _mixed(n, 1, -1, dt)
        x1 = L.impulses(n, [0], dt)
        A.check_execute(probe, x1, "mixed_radix", ref=L.ref_1d(n, -1), kind="impulse", expect=lambda: expect(probe.info))
        js = _js(n, [seen["f"][0]] + L.prime_factors(seen["f"][1]))
    x = L.impulses(n, js, dt)
    for d in (-1, 1):
        plan = _mixed(n, len(js), d, dt)
        L.closed_form_checked(L.ref_1d(n, d), L.ref_1d(n, d, np.longdouble), x, "mixed_radix", dt, n, label="mixed radix")
        A.check_execute(plan, x, "mixed_radix", ref=L.ref_1d(n, d), kind="impulse", expect=lambda: expect(plan.info),
                        inplace=_inplace(len(js), n), label="mixed radix n=%d dir=%+d" % (n, d))


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n,lds,passes", [(7, 0, 1), (1009, 0, 1), (1009, 4096, 2), (2049, 4096, 3)])
def test_impulses_chirp_z(n, lds, passes, dt, monkeypatch):
    """Fused, with the element-wise steps as kernels of their own and unchained; the bound is at log2 m."""
    m = L.chirpz_m(n)
    for env, fused in ((None, None), ("FFT_EMU_NO_FUSION", 0), ("FFT_EMU_NO_CHAIN", 1)):
        if env:
            monkeypatch.setenv(env, "1")

        def expect(info):
            assert info[0] == 10 + passes, info
            assert (info[4] == fused) if fused is not None else (info[4] == 3 if passes == 1 else info[4] in (1, 2)), info
        _impulse_1d(lambda b, d: _fft(n, b, d, dt, 0, lds), n, dt, "bluestein", expect, "chirp-z %s" % (env or "fused"), m=m)
        if env:
            monkeypatch.delenv(env)


def _run_real(n, batch, r2c, dt, mixed):
    def run(i, _, o):
        if mixed:
            info = (C.c_int * 8)()
            assert EMX.lib().emu_mixed_real(i, o, n, batch, r2c, _prec(dt), 0, 1, info) == 0
        else:
            E.lib().emu_real.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4
            assert E.lib().emu_real(i, o, n, batch, r2c, _prec(dt)) == 0
    return run


@pytest.mark.parametrize("dt", [L.F32, L.F64], ids=DT_IDS)
@pytest.mark.parametrize("n", L.REAL)
def test_impulses_r2c_c2r(n, dt):
    """r2c: real impulses against the first n/2 + 1 entries of the column; c2r: one-hot Hermitian half spectra against
    2 cos(2 pi j k / n) / n.  n = 1000 runs its core on the mixed-radix engine."""
    cdt = L.C64 if dt == L.F32 else L.C128
    mixed = n == 1000
    hb = n // 2 + 1
    js = _js(n, L.prime_factors(n), every=1024 if n in (1024, 1000) else 128)  # 1009, 1006: a chirp-z core, sampled
    x = L.impulses(n, js, dt)
    inplace = _inplace(len(js), n)
    L.closed_form_checked(L.ref_r2c(n), L.ref_r2c(n, np.longdouble), x, "r2c", dt, n, label="r2c")
    A.check_execute_io(_run_real(n, len(js), 1, dt, mixed), x, hb, cdt, "r2c", L.ref_r2c(n), n=n, inplace=inplace, kind="impulse", label="r2c n=%d" % n)
    jh = js[js <= n // 2]
    X = L.impulses(hb, jh, cdt)
    L.closed_form_checked(L.ref_c2r(n), L.ref_c2r(n, np.longdouble), X, "c2r", dt, n, label="c2r")
    A.check_execute_io(_run_real(n, len(jh), 0, dt, mixed), X, n, dt, "c2r", L.ref_c2r(n), n=n, inplace=inplace, kind="impulse", label="c2r n=%d" % n)


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("rows,cols,mixed", L.TWO_D, ids=str)
def test_impulses_2d(rows, cols, mixed, dt):
    js = L.positions_2d(rows, cols)  # every (r, c) ...
    if rows * cols == 2048:          # ... but at 32 x 64 (2048^2 points an execute): every row r at the sampled columns positions(64)
        js = (np.arange(rows)[:, None] * cols + L.positions(cols, every=0)[None, :]).reshape(-1)
    x = L.impulses(rows * cols, js, dt)
    for d in (-1, 1):
        seen = []

        def run(i, _, o):
            info = (C.c_int * 8)()
            if mixed:
                assert EMX.lib().emu_mixed_fft2d(i, o, rows, cols, len(js), d, _prec(dt), 0, 1, info) == 0
            else:
                E.lib().emu_fft2d.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_int)]
                assert E.lib().emu_fft2d(i, o, rows, cols, len(js), d, _prec(dt), 0, info) == 0
            seen.append(list(info))
        L.closed_form_checked(L.ref_2d(rows, cols, d), L.ref_2d(rows, cols, d, np.longdouble), x, "2d", dt, rows * cols, label="2D")
        A.check_execute_io(run, x, rows * cols, dt, "2d", L.ref_2d(rows, cols, d), n=rows * cols, inplace=_inplace(len(js), rows * cols),
                           kind="impulse", label="2D %d x %d dir=%+d" % (rows, cols, d))
        assert seen[0][0] == (XL.DIRECT if rows == 32 else XL.TRANSPOSE), seen[0]


# ---------------------------------------------------------------------------------------------------------------------------
# B, C. exact conditions, one size per path family
# ---------------------------------------------------------------------------------------------------------------------------
def _ptr_run(plan):
    def run(i, _, o):
        plan.execute_ptr(i, o)
    return run


EXACT_1D = [(name, dt) for name in ("single_pass", "radix2_shfl", "radix2_global", "two_pass", "three_pass", "wide_row", "team", "team_quad",
                                    "mixed_radix", "mixed_two_pass", "chirp_z", "chirp_z_two_pass")
            for dt in L.BOTH if not (name == "wide_row" and dt == L.C128)]  # the emulated wide-row shape is fp32 (n = 512)


@pytest.mark.parametrize("name,dt", EXACT_1D, ids=lambda v: v if isinstance(v, str) else v.name)
def test_exact_conditions_1d(name, dt, monkeypatch):
    c = 4
    if name == "single_pass":
        n, make = 64, lambda b, d: _fft(64, b, d, dt, 0, SL.LDS_BUDGET)
        c = SL.cmax(6, dt)  # a batch above Cmax plans the full tile
    elif name == "radix2_shfl":
        n, make = 128, lambda b, d: _fft(128, b, d, dt, 6)  # four transforms (waves) per workgroup
    elif name == "radix2_global":
        n, make = 64, lambda b, d: _fft(64, b, d, dt, 4)
    elif name == "two_pass":
        n, make = 256, lambda b, d: _fft(256, b, d, dt, 0, 4096)
    elif name == "three_pass":
        n, make = 4096, lambda b, d: _fft(4096, b, d, dt, 0, 4096)
    elif name == "wide_row":
        monkeypatch.setenv("FFT_EMU_WIDE", "1")
        n, make, c = 512, lambda b, d: _fft(512, b, d, dt), 3  # one row per workgroup step, 3 emulated CUs
    elif name == "team":
        n, make, c = 2048, lambda b, d: _team(monkeypatch, 2048, b, d, dt, 2, 2, 16, 8192 * (2 if dt == L.C128 else 1)), 4  # four teams
    elif name == "team_quad":
        monkeypatch.setenv("FFT_EMU_TEAM_QUAD", "1")
        n, make, c = 1024, lambda b, d: _team(monkeypatch, 1024, b, d, dt, 1, 2, 32, 4096 * (2 if dt == L.C128 else 1)), 2
    elif name == "mixed_radix":
        n, make = 30, lambda b, d: _mixed(30, b, d, dt)
        c = 4096 // 30 // (1 if dt == L.C64 else 2)
    elif name == "mixed_two_pass":
        n, make, c = 4200, lambda b, d: _mixed(4200, b, d, dt), 1
    elif name == "chirp_z":
        n, make = 101, lambda b, d: _fft(101, b, d, dt, 0, SL.LDS_BUDGET)
        c = SL.cmax(8, dt)  # the core's tile at m = 256; asserted below on the plan that ran
    else:
        n, make, c = 1009, lambda b, d: _fft(1009, b, d, dt, 0, 4096), 2
    batch, rows = L.neighbour_batch(c)
    x = L.normal_scaled(n, batch, dt, seed=n)
    for d in (-1, 1):
        plan = make(batch, d)
        L.exact_conditions(_ptr_run(plan), x, rows, "%s %s n=%d batch=%d dir=%+d" % (name, np.dtype(dt).name, n, batch, d))
        if name == "chirp_z":
            assert plan.info[0] == 11 and plan.info[4] == 3 and 1 << plan.info[2] == c, plan.info


def test_tile_widths_match_the_planner():
    """The tile the exact-condition batches are built around is the planner's: single pass n = 64 plans Cmax at a batch of
    2 Cmax + ..., the mixed-radix plan of n = 30 the tile of mixed_radix_ladder.tile_rows."""
    import mixed_radix_ladder as ML
    for dt in L.BOTH:
        c = SL.cmax(6, dt)
        batch, _ = L.neighbour_batch(c)
        plan = _fft(64, batch, -1, dt, 0, SL.LDS_BUDGET)
        x = np.zeros((batch, 64), dtype=dt)
        y = np.empty_like(x)
        plan.execute_ptr(x.ctypes.data, y.ctypes.data)
        assert 1 << plan.info[2] == c, plan.info
        assert ML.tile_rows(30, dt, 1 << 20) == 4096 // 30 // (1 if dt == L.C64 else 2)


@pytest.mark.parametrize("dt", [L.F32, L.F64], ids=DT_IDS)
@pytest.mark.parametrize("n", [64, 1000, 1009])
def test_exact_conditions_real(n, dt):
    cdt = L.C64 if dt == L.F32 else L.C128
    hb, batch, rows = n // 2 + 1, 11, [0, 4, 10]
    x = L.normal_scaled(n, batch, dt, seed=n)
    L.exact_conditions(_run_real(n, batch, 1, dt, n == 1000), x, rows, "r2c %s n=%d" % (dt.name, n), w_out=hb, dtype_out=cdt)
    X = XL.half_spectra(n, batch, cdt, seed=n + 1)
    L.exact_conditions(_run_real(n, batch, 0, dt, n == 1000), X, rows, "c2r %s n=%d" % (dt.name, n), w_out=n, dtype_out=dt)


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("rows,cols,mixed", [(32, 8, False), (12, 32, False), (6, 10, True)], ids=str)
def test_exact_conditions_2d(rows, cols, mixed, dt):
    """A poisoned matrix of the batch leaves the other matrices bit-identical."""
    nm = 5
    x = L.normal_scaled(rows * cols, nm, dt, seed=rows + cols)
    for d in (-1, 1):
        def run(i, _, o):
            info = (C.c_int * 8)()
            if mixed:
                assert EMX.lib().emu_mixed_fft2d(i, o, rows, cols, nm, d, _prec(dt), 0, 1, info) == 0
            else:
                E.lib().emu_fft2d.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_int)]
                assert E.lib().emu_fft2d(i, o, rows, cols, nm, d, _prec(dt), 0, info) == 0
        L.exact_conditions(run, x, [0, 3], "2D %d x %d %s dir=%+d" % (rows, cols, np.dtype(dt).name, d))


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("kind,nx,nh,lds", [("conv", 99, 27, 0), ("circ", 64, 0, 0), ("autocorr", 100, 0, 0), ("xcorr", 333, 0, 0),
                                            ("psd", 64, 0, 0), ("conv", 901, 101, 4096), ("xcorr", 1001, 0, 4096)], ids=str)
def test_exact_conditions_fused(kind, nx, nh, lds, dt):
    """The four fused consumers (and the circular convolution): poison one batch row of x; cross-correlation also one row of y."""
    batch, rows = 11, [0, 5, 10]
    x = XL.complex_rows(nx, batch, dt, seed=nx)
    y = XL.complex_rows(nx, batch, dt, seed=nx + 1) if kind == "xcorr" else None
    h = XL.complex_rows(nh if kind == "conv" else nx, 1, dt, seed=nh + 7)[0] if kind in ("conv", "circ") else None
    w_out, dt_out = XL.fused_out(kind, nx, nh, dt)
    f = E.lib().emu_fused
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                  C.POINTER(C.c_int)]

    def run(i, i2, o):
        info = (C.c_int * 8)()
        assert f(E.FUSED[kind], i, i2, None if h is None else h.ctypes.data, nx, nh, o, batch, _prec(dt), lds, 0, 48000.0, info) == 0
    L.exact_conditions(run, x, rows, "%s %s nx=%d" % (kind, np.dtype(dt).name, nx), degree=2 if kind in ("autocorr", "psd") else 1,
                       w_out=w_out, dtype_out=dt_out, x2=y)


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("case", [c for c in FL.SMALL if c.name in ("a", "c")], ids=repr)
def test_exact_conditions_frames(case, dt):
    """A poisoned signal leaves the other signals' STFT, power and Welch rows bit-identical (frames_ladder cases a and c)."""
    x = A.block_normal_rows(case.pitch, 0, case.n_signals, dt, 7)
    for kind in case.kinds:
        rows_out, width, odt = FL.out_shape(case, kind, dt)

        def run(i, _, o):
            rc, info = EF.frames(i, o, case.n, case.hop, case.signal_len, case.n_signals, case.pitch, case.window, None, kind, _prec(dt), 0,
                                 False, FL.FS)
            assert rc == 0 and info[1] == 1, (rc, info)
        out_rows = (lambda s: (s,)) if kind == FL.WELCH else (lambda s: range(s * case.nw, (s + 1) * case.nw))
        L.exact_conditions(run, x, [0, 12, 29], "frames %s %s %s" % (case, FL.KIND_NAMES[kind], np.dtype(dt).name),
                           degree=1 if kind == FL.STFT else 2, w_out=width, dtype_out=odt, rows_out=rows_out, out_rows=out_rows)
