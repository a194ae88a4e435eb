"""The single-pass sizes n = 2^0 ... 2^12 at the batches that give the single-pass kernel every tile shape it gets in use
(tests/single_pass_ladder.py), and the two reference-shaped kernels past the point where their grids start to stride.

Every case runs through accuracy.check_execute_streamed(): both directions, out of place into a guarded NaN-filled output and in
place, every transform bin by bin against float64, and the plan must have run ONE launch group of the single-pass schedule.
n = 1 must return its input bit for bit."""
import numpy as np
import pytest

import accuracy as A
import single_pass_ladder as L

pytestmark = pytest.mark.gpu

ALGO_ID = {"auto": 3, "radix2": 1, "radix4": 2, "split_radix": 3, "radix2_global": 4, "radix2_shfl": 6}  # info.algo (auto plans split_radix)


def _expect(plan, batch, algo, log2n):
    def check():
        info = plan.info()
        passes = log2n + 1 if algo == "radix2_global" else 1
        assert info.n_passes == passes, ("n_passes", info.n_passes, passes)
        assert info.algo == ALGO_ID[algo], ("algo", info.algo, algo)
        assert info.chunk_batch == batch, ("chunk_batch", info.chunk_batch, batch)
        assert info.team_tiles == 0, ("team_tiles", info.team_tiles)
    return check


def _run(algo, log2n, dtype, batch, family="multipass"):
    import fftlib
    n = 1 << log2n
    dt = np.dtype(dtype)
    for d in (-1, 1):
        plan = fftlib.Plan(n, batch, d, dt, fftlib.ALGO_NAMES[algo])
        try:
            A.check_execute_streamed(plan, n, batch, dt, seed=1000 * log2n + (batch % 997), family=family,
                                     expect=_expect(plan, batch, algo, log2n), exact=(n == 1),
                                     label="%s %s n=%d batch=%d dir=%+d" % (algo, dt.name, n, batch, d),
                                     long_rows=1 if dt == np.complex128 else 0)
        finally:
            plan.destroy()


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("log2n", L.LOG2N)
def test_auto_full_ladder(gpu_lib, log2n, dtype):
    for batch in L.LADDER[(log2n, dtype)]:
        _run("auto", log2n, dtype, batch)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("log2n", L.LOG2N[1:])
@pytest.mark.parametrize("algo", ["radix2", "radix4", "split_radix"])
def test_explicit_families(gpu_lib, algo, log2n, dtype):
    for batch in L.explicit_batches(log2n, dtype):
        _run(algo, log2n, dtype, batch)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("log2n", [7, 8, 9, 10])
def test_radix2_shfl_grid_stride(gpu_lib, log2n, dtype):
    """wave_dit_kernel: at most num_cus * 8 workgroups of 4 transforms, so its grid-stride loop starts past 8192 transforms."""
    for batch in (1, 5, 8191, 8193, 3 * 8192 + 5):
        _run("radix2_shfl", log2n, dtype, batch, family="radix2_shfl")


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("log2n", [1, 3, 6, 10, 12])
def test_radix2_global_grid_stride(gpu_lib, log2n, dtype):
    """bitrev_kernel + one radix2_dit_stage_kernel launch per stage: grids of at most 16384 x 256 threads, so their loops start past
    2^22 elements (2^22 butterflies); the last batch puts n * batch past 2^23, ragged."""
    n = 1 << log2n
    for batch in (1, 5, (1 << 23) // n + 3):
        _run("radix2_global", log2n, dtype, batch, family="radix2_global")
