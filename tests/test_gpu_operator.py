"""Every path as a linear operator, on the device, at the cases of tests/operator_ladder.py.

A. unit impulses against the closed-form column of the DFT matrix through accuracy.check_execute / check_execute_io (guards,
   untouched input, in place bit-identical): the per-bin error of an impulse is the twiddle error, undiluted.  Each case asserts
   through plan.info() / team_status() the path it was written for; accuracy.check_rows prints the worst e / (u log2 n) before it asserts.
B. a poisoned transform (NaN / one Inf / overflowing values) leaves every other transform of the batch bit-identical.
C. execute(2^s x) == 2^s execute(x) bit for bit; zeros in, zeros out."""
import numpy as np
import pytest

import accuracy as A
import ext_ladder as XL
import frames_ladder as FL
import operator_ladder as L
import single_pass_ladder as SL

pytestmark = pytest.mark.gpu

DT_IDS = ["fp32", "fp64"]


def _ptr_run(plan):
    def run(d_in, _, d_out):
        plan.execute_ptr(d_in, d_out)
        assert plan.sync() == 0
    return run


def _impulse_1d(make, n, dt, family, label, m=None, factors=(), batch=None, variants=None):
    """Both directions of one 1D plan on the impulses of n (cycled up to `batch` rows).  make(batch, d) -> (plan, expect)."""
    js = L.positions(n, factors)
    if batch and batch > len(js):
        js = np.resize(js, batch)
    x = L.impulses(n, js, dt)
    for d in (-1, 1):
        plan, expect = make(len(js), d)
        try:
            L.closed_form_checked(L.ref_1d(n, d), L.ref_1d(n, d, np.longdouble), x, family, dt, n, m, label=label)
            for v in variants or (None,):
                if v:
                    v(plan)
                A.check_execute(plan, x, family, m=m, ref=L.ref_1d(n, d), kind="impulse", expect=expect(plan),
                                label="%s n=%d dir=%+d" % (label, n, d))
        finally:
            plan.destroy()


def _single(algo, n, dt):
    import fftlib
    ids = {"auto": 3, "radix2": 1, "radix4": 2, "split_radix": 3, "radix2_global": 4, "radix2_shfl": 6}

    def make(batch, d):
        plan = fftlib.Plan(n, batch, d, dt, fftlib.ALGO_NAMES[algo])

        def expect(p):
            def check():
                info = p.info()
                assert info.algo == ids[algo] and info.team_tiles == 0 and info.bluestein_m == 0, (info.algo, info.team_tiles)
                assert info.n_passes == (n.bit_length() if algo == "radix2_global" else 1), info.n_passes
            return check
        return plan, expect
    return make


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n", L.SINGLE_PASS_AUTO)
def test_impulses_single_pass_auto(gpu_lib, n, dt):
    _impulse_1d(_single("auto", n, dt), n, dt, "multipass", "single pass auto")


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("algo,n", L.SINGLE_PASS_EXPLICIT, ids=str)
def test_impulses_explicit_families(gpu_lib, algo, n, dt):
    family = algo if algo in ("radix2_global", "radix2_shfl") else "multipass"
    _impulse_1d(_single(algo, n, dt), n, dt, family, algo)


@pytest.mark.parametrize("n,dt", L.WIDE_ROW, ids=str)
def test_impulses_wide_row(gpu_lib, n, dt):
    import fftlib

    def make(batch, d):
        plan = fftlib.Plan(n, batch, d, dt)

        def expect(p):
            def check():  # at these sizes only wide_row_kernel is single-pass (fft_hip_backend.hip wide_rows)
                assert p.info().n_passes == 1 and p.info().team_tiles == 0, (p.info().n_passes, p.info().team_tiles)
            return check
        return plan, expect
    _impulse_1d(make, n, dt, "wide_row", "wide row")


def _passes(n, dt, batch=4):
    import fftlib
    plan = fftlib.Plan(n, batch, -1, dt)
    plan.set_option(fftlib.OPT_TEAM_ENABLE, 0)
    p = plan.info().n_passes
    plan.destroy()
    return p


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("passes", [2, 3])
def test_impulses_multi_pass(gpu_lib, passes, dt):
    """The smallest n the planner gives two / three passes, the team kernels switched off (FFT_GPU_OPT_TEAM_ENABLE = 0)."""
    import fftlib
    log2n = next(t for t in range(13, 23) if _passes(1 << t, dt) == passes)
    n = 1 << log2n
    assert _passes(n >> 1, dt) < passes
    if passes == 3:
        assert log2n <= 21, "2^21 is the first three-pass size (fp32)"
    print("multi-pass: %d passes from n = 2^%d (%s)" % (passes, log2n, np.dtype(dt).name))

    def make(batch, d):
        plan = fftlib.Plan(n, batch, d, dt)
        plan.set_option(fftlib.OPT_TEAM_ENABLE, 0)

        def expect(p):
            def check():
                assert p.info().n_passes == passes and p.team_status() != 0, (p.info().n_passes, p.team_status())
            return check
        return plan, expect
    _impulse_1d(make, n, dt, "multipass", "%d passes" % passes)


@pytest.mark.parametrize("log2n,dt", L.TEAM, ids=str)
def test_impulses_team_kernels(gpu_lib, log2n, dt):
    """Every team-kernel instantiation, forced at any batch (team = 2, min_batch = 1), at one round of teams plus a ragged remainder."""
    import fftlib
    fftlib.set_policy(team=2, min_batch=1)
    n = 1 << log2n
    nt = 8 << (20 - log2n - (1 if dt == L.C128 else 0))
    kernel = 2 if (dt == L.C128 and log2n >= 17) else 3
    family = {3: "team_quad", 2: "team_defer"}[kernel]

    def make(batch, d):
        plan = fftlib.Plan(n, batch, d, dt)
        assert plan.info().team_tiles == 4

        def expect(p):
            def check():
                assert p.team_status() == 0 and p.info().team_kernel == kernel, (p.team_status(), p.info().team_kernel)
            return check
        return plan, expect
    _impulse_1d(make, n, dt, family, "team kernel %d" % kernel, batch=nt + 3)


def _mixed(n, dt, passes, seen=None):
    import fftlib

    def make(batch, d):
        plan = fftlib.Plan(n, batch, d, dt, fftlib.ALGO_MIXED_RADIX)

        def expect(p):
            def check():
                info = p.info()
                assert info.algo == 7 and info.n_passes == passes and info.bluestein_m == 0, (info.algo, info.n_passes)
            return check
        return plan, expect
    return make


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n", L.MIXED_ALL + L.MIXED_SAMPLED)
def test_impulses_mixed_radix(gpu_lib, n, dt):
    import fftlib
    passes = 1 if n <= 4096 else 2
    factors = L.prime_factors(n)
    if passes == 2:
        probe = fftlib.Plan(n, 1, -1, dt, fftlib.ALGO_MIXED_RADIX)
        f = list(probe.info().factors)
        probe.destroy()
        assert f[0] * f[1] == n, f
        factors = [f[0]] + L.prime_factors(f[1])
    _impulse_1d(_mixed(n, dt, passes), n, dt, "mixed_radix", "mixed radix", factors=factors)


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("n", L.CHIRPZ)
def test_impulses_chirp_z(gpu_lib, n, dt):
    """Fused, NO_FUSION and NO_CHAIN; the bound is at log2 m."""
    import fftlib
    m = L.chirpz_m(n)
    state = {}

    def make(batch, d):
        plan = fftlib.Plan(n, batch, d, dt)
        assert plan.info().bluestein_m == m, plan.info().bluestein_m
        state["fused"] = plan.info().fused
        if n == 1009:
            assert state["fused"] == 3, state  # one kernel
        assert state["fused"] >= 1

        def expect(p):
            def check():
                assert p.info().fused == state["want"], (p.info().fused, state)
            return check
        return plan, expect

    def variant(no_fusion, no_chain):
        def apply(plan):
            plan.set_option(fftlib.OPT_NO_FUSION, no_fusion)
            plan.set_option(fftlib.OPT_NO_CHAIN, no_chain)
            state["want"] = 0 if no_fusion else min(state["fused"], 1) if no_chain else state["fused"]
        return apply
    _impulse_1d(make, n, dt, "bluestein", "chirp-z", m=m, variants=[variant(0, 0), variant(1, 0), variant(0, 1)])


@pytest.mark.parametrize("dt", [L.F32, L.F64], ids=DT_IDS)
@pytest.mark.parametrize("n", L.REAL)
def test_impulses_r2c_c2r(gpu_lib, n, dt):
    import fftlib
    cdt = L.C64 if dt == L.F32 else L.C128
    algo = fftlib.ALGO_MIXED_RADIX if n == 1000 else fftlib.ALGO_AUTO
    hb = n // 2 + 1
    js = L.positions(n)
    jh = js[js <= n // 2]
    fwd, inv = fftlib.ExtPlan.r2c(n, len(js), dt, algo), fftlib.ExtPlan.c2r(n, len(jh), dt, algo)
    try:
        for p in (fwd, inv):
            info = p.info()
            assert (info.algo == 7) == (n == 1000) and (info.bluestein_m > 0) == (n in (1009, 1006)), (n, info.algo, info.bluestein_m)
        x = L.impulses(n, js, dt)
        L.closed_form_checked(L.ref_r2c(n), L.ref_r2c(n, np.longdouble), x, "r2c", dt, n, label="r2c")
        A.check_execute_io(_ptr_run(fwd), x, hb, cdt, "r2c", L.ref_r2c(n), n=n, inplace=True, kind="impulse", label="r2c n=%d" % n)
        X = L.impulses(hb, jh, cdt)
        L.closed_form_checked(L.ref_c2r(n), L.ref_c2r(n, np.longdouble), X, "c2r", dt, n, label="c2r")
        A.check_execute_io(_ptr_run(inv), X, n, dt, "c2r", L.ref_c2r(n), n=n, inplace=True, kind="impulse", label="c2r n=%d" % n)
    finally:
        fwd.destroy()
        inv.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("rows,cols,mixed", L.TWO_D, ids=str)
def test_impulses_2d(gpu_lib, rows, cols, mixed, dt):
    import fftlib
    js = L.positions_2d(rows, cols)
    x = L.impulses(rows * cols, js, dt)
    for d in (-1, 1):
        plan = fftlib.ExtPlan.fft2d(rows, cols, len(js), d, dt, fftlib.ALGO_MIXED_RADIX if mixed else fftlib.ALGO_AUTO)
        try:
            info = plan.info()
            assert info.n_passes == (1 if rows == 32 else 0), info.n_passes  # direct column pass / the transposed image
            assert (info.algo == 7) == mixed, info.algo
            L.closed_form_checked(L.ref_2d(rows, cols, d), L.ref_2d(rows, cols, d, np.longdouble), x, "2d", dt, rows * cols, label="2D")
            A.check_execute_io(_ptr_run(plan), x, rows * cols, dt, "2d", L.ref_2d(rows, cols, d), n=rows * cols, inplace=True,
                               kind="impulse", label="2D %d x %d dir=%+d" % (rows, cols, d))
        finally:
            plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------------
# B, C. exact conditions, one size per path family
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_1D = ["single_pass", "radix2_shfl", "radix2_global", "wide_row", "two_pass_launch_groups", "three_pass", "team_2^16", "team_2^17",
            "mixed_radix", "mixed_two_pass", "chirp_z", "chirp_z_multi_pass"]


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("name", EXACT_1D)
def test_exact_conditions_1d(gpu_lib, name, dt):
    """Two full tiles and a ragged one; poisoned: the first and the last transform of a tile and the last of the batch (the
    launch-group case: the transforms on both sides of a group boundary)."""
    import fftlib
    import mixed_radix_ladder as ML
    algo, opts, rows = fftlib.ALGO_AUTO, {}, None
    if name == "single_pass":
        n, c = 1024, SL.cmax(10, dt)
    elif name == "radix2_shfl":
        n, c, algo = 128, 4, fftlib.ALGO_RADIX2_SHFL  # four waves, one transform each, per workgroup
    elif name == "radix2_global":
        n, c, algo = 64, 4, fftlib.ALGO_RADIX2_GLOBAL
    elif name == "wide_row":
        n, c = 8192, 3
    elif name == "two_pass_launch_groups":
        n = 1 << 16
        fftlib.set_policy(team=0, chunk_mb=max(1, (4 * n * np.dtype(dt).itemsize) >> 20))
        c, opts = 4, {"chunk": 4, "passes": 2}
        batch, rows = 11, [3, 4, 10]
    elif name == "three_pass":
        n, c, opts = 1 << 21, 1, {"passes": 3}
        fftlib.set_policy(team=0)
    elif name == "team_2^16":  # team_quad_kernel in both precisions
        n, c, opts = 1 << 16, 4, {"kernel": 3}
        fftlib.set_policy(team=2, min_batch=1)
    elif name == "team_2^17":  # fp64: team_defer_kernel; fp32: team_quad_kernel again (no fp32 size runs team_defer)
        n, c, opts = 1 << 17, 4, {"kernel": 2 if dt == L.C128 else 3}
        fftlib.set_policy(team=2, min_batch=1)
    elif name == "mixed_radix":
        n, algo = 30, fftlib.ALGO_MIXED_RADIX
        c = ML.tile_rows(30, dt, 1 << 20)
    elif name == "mixed_two_pass":
        n, c, algo, opts = 4200, 1, fftlib.ALGO_MIXED_RADIX, {"passes": 2}
    elif name == "chirp_z":
        n, c = 1009, SL.cmax(11, dt)
    else:
        n, c = 100003, 1
    if rows is None:
        batch, rows = L.neighbour_batch(c)
    x = L.normal_scaled(n, batch, dt, seed=n)
    for d in (-1, 1):
        plan = fftlib.Plan(n, batch, d, dt, algo)
        try:
            info = plan.info()
            if "passes" in opts:
                assert info.n_passes == opts["passes"] and info.team_tiles == 0, (info.n_passes, info.team_tiles)
            if "chunk" in opts:
                assert info.chunk_batch == opts["chunk"], info.chunk_batch
            if "kernel" in opts:
                assert info.team_kernel == opts["kernel"] and info.team_tiles == 4, (info.team_kernel, info.team_tiles)
            if name.startswith("chirp_z"):
                assert info.bluestein_m == L.chirpz_m(n)
            if name.startswith("mixed"):
                assert info.algo == 7
            L.exact_conditions(_ptr_run(plan), x, rows, "%s %s n=%d batch=%d dir=%+d" % (name, np.dtype(dt).name, n, batch, d))
            if "kernel" in opts:
                assert plan.team_status() == 0, plan.team_status()
        finally:
            plan.destroy()


@pytest.mark.parametrize("dt", [L.F32, L.F64], ids=DT_IDS)
@pytest.mark.parametrize("n", [1024, 1000, 1009])
def test_exact_conditions_real(gpu_lib, n, dt):
    import fftlib
    cdt = L.C64 if dt == L.F32 else L.C128
    algo = fftlib.ALGO_MIXED_RADIX if n == 1000 else fftlib.ALGO_AUTO
    hb, batch, rows = n // 2 + 1, 37, [0, 16, 36]
    fwd, inv = fftlib.ExtPlan.r2c(n, batch, dt, algo), fftlib.ExtPlan.c2r(n, batch, dt, algo)
    try:
        L.exact_conditions(_ptr_run(fwd), L.normal_scaled(n, batch, dt, seed=n), rows, "r2c %s n=%d" % (dt.name, n), w_out=hb, dtype_out=cdt)
        L.exact_conditions(_ptr_run(inv), XL.half_spectra(n, batch, cdt, seed=n + 1), rows, "c2r %s n=%d" % (dt.name, n), w_out=n, dtype_out=dt)
    finally:
        fwd.destroy()
        inv.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("rows,cols,mixed", L.TWO_D, ids=str)
def test_exact_conditions_2d(gpu_lib, rows, cols, mixed, dt):
    """A poisoned matrix of the batch leaves the other matrices bit-identical."""
    import fftlib
    nm = 5
    x = L.normal_scaled(rows * cols, nm, dt, seed=rows + cols)
    for d in (-1, 1):
        plan = fftlib.ExtPlan.fft2d(rows, cols, nm, d, dt, fftlib.ALGO_MIXED_RADIX if mixed else fftlib.ALGO_AUTO)
        try:
            L.exact_conditions(_ptr_run(plan), x, [0, 3], "2D %d x %d %s dir=%+d" % (rows, cols, np.dtype(dt).name, d))
        finally:
            plan.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("kind,nx,nh,fused", [("conv", 999, 27, 3), ("autocorr", 1000, 0, 3), ("xcorr", 1000, 0, 1), ("psd", 4096, 0, 1),
                                              ("conv", 9001, 101, 2), ("xcorr", 4097, 0, 2)], ids=str)
def test_exact_conditions_fused(gpu_lib, kind, nx, nh, fused, dt):
    """The four fused consumers: poison one batch row of x; cross-correlation also one row of y."""
    import fftlib
    batch, rows = 37, [0, 17, 36]
    x = XL.complex_rows(nx, batch, dt, seed=nx)
    y = XL.complex_rows(nx, batch, dt, seed=nx + 1) if kind == "xcorr" else None
    h = XL.complex_rows(nh, 1, dt, seed=nh + 7)[0] if kind == "conv" else None
    w_out, dt_out = XL.fused_out(kind, nx, nh, dt)
    plan = fftlib.ExtPlan.fused(kind, nx, batch, h, dt)
    try:
        assert plan.info().fused == fused, plan.info().fused

        def run(d_x, d_y, d_out):
            plan.execute_fused(d_x, d_y, d_out, 48000.0)
            assert plan.sync() == 0
        L.exact_conditions(run, x, rows, "%s %s nx=%d" % (kind, np.dtype(dt).name, nx), degree=2 if kind in ("autocorr", "psd") else 1,
                           w_out=w_out, dtype_out=dt_out, x2=y)
    finally:
        plan.destroy()


@pytest.mark.parametrize("dt", L.BOTH, ids=DT_IDS)
@pytest.mark.parametrize("case", [c for c in FL.SMALL if c.name in ("a", "c")], ids=repr)
def test_exact_conditions_frames(gpu_lib, case, dt):
    """A poisoned signal leaves the other signals' STFT, power and Welch rows bit-identical (frames_ladder cases a and c)."""
    import fftlib
    x = A.block_normal_rows(case.pitch, 0, case.n_signals, dt, 7)
    for kind in case.kinds:
        rows_out, width, odt = FL.out_shape(case, kind, dt)
        plan = fftlib.ExtPlan.frames(case.n, case.hop, case.signal_len, case.n_signals, "hann", FL.KIND_NAMES[kind], dt)
        try:
            assert plan.info().fused == 1 and plan.nw == case.nw

            def run(d_x, _, d_out):
                plan.execute_frames(d_x, d_out, case.pitch, FL.FS)
                assert plan.sync() == 0
            out_rows = (lambda s: (s,)) if kind == FL.WELCH else (lambda s: range(s * case.nw, (s + 1) * case.nw))
            L.exact_conditions(run, x, [0, 12, 29], "frames %s %s %s" % (case, FL.KIND_NAMES[kind], np.dtype(dt).name),
                               degree=1 if kind == FL.STFT else 2, w_out=width, dtype_out=odt, rows_out=rows_out, out_rows=out_rows)
        finally:
            plan.destroy()
