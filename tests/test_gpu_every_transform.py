"""Every transform of every batch the shipped schedules compute, bin by bin, against a float64 reference (tests/accuracy.py).

The team kernels take their transforms from a device-wide counter, so a stale window read, a lost deferred store or a claim past
the end lands on an arbitrary transform: sampling a few transforms, or comparing peaks and norms, does not see it.  Each batch
here runs through check_execute(): normal inputs that differ per transform, a NaN-filled output between two guard transforms,
e_b <= K u log2(n) for every transform, the input of an out-of-place execute unchanged, in place bit-identical to out of place;
and the plan must have run the schedule under test."""
import numpy as np
import pytest

import accuracy as A

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128


def _expect_team(plan, kernel):
    def check():
        assert plan.team_status() == 0, "the team kernel must have done the work (status %d)" % plan.team_status()
        assert plan.info().team_kernel == kernel
    return check


def _family(kernel):
    return {3: "team_quad", 2: "team_defer", 1: "team_defer"}[kernel]


# the shipped full-batch schedules on the default policy: (log2n, batch, dtype, team kernel, also in place)
SHIPPED = [
    (16, 4096, C64, 3, True),    # BASELINE config 2
    (20, 512, C64, 3, True),     # config 3 (bench.py's flagship)
    (18, 1024, C64, 3, True),    # config 4's per-GPU shard
    (19, 512, C64, 3, False),
    (17, 2048, C64, 3, False),
    (15, 8192, C64, 3, False),
    (19, 256, C128, 2, False),   # bench.py's secondary_fp64 shape: team_defer_kernel
    (16, 257, C128, 3, True),    # fp64 quad sizes one transform past the 256 MiB crossover
    (15, 513, C128, 3, True),
    (14, 1025, C128, 3, True),
]


@pytest.mark.parametrize("log2n,batch,dtype,kernel,inplace", SHIPPED)
def test_shipped_schedule_every_transform(gpu_lib, log2n, batch, dtype, kernel, inplace):
    import fftlib
    n = 1 << log2n
    x = A.normal_rows(n, 0, batch, dtype, seed=log2n)
    for d in (-1, 1):
        plan = fftlib.Plan(n, batch, d, dtype)
        info = plan.info()
        assert info.team_tiles == 4 and info.team_kernel == kernel, (info.team_tiles, info.team_kernel)
        A.check_execute(plan, x, _family(kernel), inplace=inplace, expect=_expect_team(plan, kernel),
                        label="default policy 2^%d x %d" % (log2n, batch), long_rows=2 if dtype == C128 else 0)
        plan.destroy()


# every team-kernel instantiation (the list of test_gpu_parity.py::test_team_kernel_vs_oracle)
TEAM_SIZES = [(20, C64), (19, C64), (18, C64), (17, C64), (15, C64), (16, C64),
              (19, C128), (18, C128), (17, C128), (16, C128), (15, C128), (14, C128)]


def _n_teams(log2n, dtype):
    return 8 << (20 - log2n - (1 if dtype == C128 else 0))


def _team_kernel(log2n, dtype):
    return 2 if (dtype == C128 and log2n >= 17) else 3


@pytest.mark.parametrize("log2n,dtype", TEAM_SIZES)
def test_team_instantiations_at_edge_batches(gpu_lib, log2n, dtype):
    """Batches 1, n_teams - 1 (idle teams), n_teams + 1 (one partial round), 2 n_teams + 3 (a ragged tail; the deferred-store
    epilogue of every team's last transform), both directions, in place and out of place."""
    import fftlib
    fftlib.set_policy(team=2, min_batch=1)  # the team kernel at every batch, also below one transform per team
    n, nt, kernel = 1 << log2n, _n_teams(log2n, dtype), _team_kernel(log2n, dtype)
    for batch in (1, nt - 1, nt + 1, 2 * nt + 3):
        x = A.normal_rows(n, 0, batch, dtype, seed=100 + log2n)
        for d in (-1, 1):
            plan = fftlib.Plan(n, batch, d, dtype)
            assert plan.info().team_tiles == 4
            A.check_execute(plan, x, _family(kernel), expect=_expect_team(plan, kernel),
                            label="team=2 2^%d x %d" % (log2n, batch), long_rows=1 if dtype == C128 else 0)
            plan.destroy()


@pytest.mark.parametrize("log2n,dtype,batch", [(20, C64, 37), (18, C64, 67), (16, C128, 131)])
def test_queued_executes_of_different_data(gpu_lib, log2n, dtype, batch):
    """Three executes on one plan, no sync in between, each with its own input and output; then executes that alternate two inputs
    into ONE output buffer, each checked: between launches the plan's window holds the previous launch's (different) data."""
    import fftlib
    fftlib.set_policy(team=2)
    n, kernel = 1 << log2n, _team_kernel(log2n, dtype)
    fam = _family(kernel)
    xs = [A.normal_rows(n, 0, batch, dtype, seed=200 + i) for i in range(3)]
    rb = n * np.dtype(dtype).itemsize
    nan_row = np.full(n, np.nan, dtype=dtype)
    gin = [A.Guarded(batch, rb) for _ in xs]
    gout = [A.Guarded(batch, rb) for _ in xs]
    plan = fftlib.Plan(n, batch, -1, dtype)
    try:
        for g, h, x in zip(gin, gout, xs):
            A.upload_rows(g, x)
            h.fill(nan_row)
        for g, h in zip(gin, gout):
            plan.execute_ptr(g.ptr, h.ptr)
        assert plan.sync() == 0
        _expect_team(plan, kernel)()
        for i, (g, h, x) in enumerate(zip(gin, gout, xs)):
            assert h.guards_intact() and g.guards_intact(), i
            assert A.input_unchanged(g, x), i
            A.check_device_rows(h, x, -1, fam, label="queued execute %d of 3" % i)
        for it in range(6):
            i = it % 2
            plan.execute_ptr(gin[i].ptr, gout[2].ptr)
            assert plan.sync() == 0
            _expect_team(plan, kernel)()
            assert gout[2].guards_intact()
            A.check_device_rows(gout[2], xs[i], -1, fam, label="alternating execute %d (input %d)" % (it, i))
    finally:
        plan.destroy()
        for g in gin + gout:
            g.free()


@pytest.mark.parametrize("n,batch,dtype", [(1000003, 64, C128), (30011, 5, C64), (100003, 3, C64)])
def test_bluestein_every_transform(gpu_lib, n, batch, dtype):
    """BASELINE config 5 (n = 1000003 fp64 x 64) and fp32 primes, fused, unfused and chained: every transform against float64."""
    import fftlib
    x = A.normal_rows(n, 0, batch, dtype, seed=n % 1000)
    variants = ((0, 0), (1, 0), (0, 1)) if n < 1000000 else ((0, 0),)
    for d in (-1, 1):
        plan = fftlib.Plan(n, batch, d, dtype)
        m = plan.info().bluestein_m
        assert m >= 2 * n - 1 and (m & (m - 1)) == 0
        for no_fusion, no_chain in variants:
            plan.set_option(fftlib.OPT_NO_FUSION, no_fusion)
            plan.set_option(fftlib.OPT_NO_CHAIN, no_chain)
            A.check_execute(plan, x, "bluestein", m=m, inplace=n < 1000000,
                            label="bluestein n=%d fusion=%d chain=%d" % (n, 1 - no_fusion, 1 - no_chain), long_rows=1 if dtype == C128 else 0)
        plan.destroy()


@pytest.mark.parametrize("log2n,dtype", [(21, C64), (21, C128), (22, C64), (24, C64)])
def test_three_pass_every_transform_over_launch_groups(gpu_lib, log2n, dtype):
    """Three-pass sizes with launch groups of two transforms (a small FFT_HIP_CHUNK_MB): five transforms in three groups."""
    import fftlib
    n = 1 << log2n
    batch = 5
    fftlib.set_policy(chunk_mb=max(1, (2 * n * np.dtype(dtype).itemsize) >> 20))
    x = A.normal_rows(n, 0, batch, dtype, seed=log2n)
    for d in (-1, 1):
        plan = fftlib.Plan(n, batch, d, dtype)
        info = plan.info()
        assert info.n_passes == 3 and info.chunk_batch == 2 and info.team_tiles == 0, (info.n_passes, info.chunk_batch)
        A.check_execute(plan, x, "multipass", label="three-pass 2^%d" % log2n, long_rows=1 if dtype == C128 else 0)
        plan.destroy()


@pytest.mark.parametrize("log2n,dtype", [(13, C64), (14, C64), (13, C128)])
def test_wide_row_every_transform(gpu_lib, log2n, dtype):
    """wide_row_kernel sizes, ragged over the 256 workgroups."""
    import fftlib
    n, batch = 1 << log2n, 256 + 37
    x = A.normal_rows(n, 0, batch, dtype, seed=log2n)
    for d in (-1, 1):
        plan = fftlib.Plan(n, batch, d, dtype)
        assert plan.info().n_passes == 1  # at these sizes only wide_row_kernel is single-pass (fft_hip_backend.hip wide_rows)
        A.check_execute(plan, x, "wide_row", label="wide row 2^%d" % log2n, long_rows=2 if dtype == C128 else 0)
        plan.destroy()


@pytest.mark.parametrize("rows,cols,count,dtype", [(512, 256, 9, C64), (256, 512, 5, C128)])
def test_2d_every_matrix(gpu_lib, rows, cols, count, dtype):
    """Batched 2D transforms (rows: one batched 1D execute, columns: the strided column pass): every matrix against numpy's fft2."""
    import fftlib
    x = A.normal_rows(rows * cols, 0, count, dtype, seed=rows + cols)
    for d in (-1, 1):
        plan = fftlib.ExtPlan.fft2d(rows, cols, count, d, dtype)

        def ref(xs):
            xs = np.asarray(xs, dtype=np.complex128).reshape(-1, rows, cols)
            return (np.fft.fft2(xs) if d < 0 else np.fft.ifft2(xs)).reshape(xs.shape[0], -1)

        A.check_execute(plan, x, "2d", direction=d, ref=ref, label="2D %d x %d x %d" % (rows, cols, count), long_rows=0)
        plan.destroy()
