"""One execute past 2^31 elements for every schedule that runs its whole batch in ONE launch (single-pass rows, the wide-row kernel,
radix2_shfl, radix2_global, n = 1, the team kernel) and for the multi-pass launch groups of the same plan: the kernels index with
64-bit offsets (tile_coord, FFT_BID / FFT_NBLOCKS, the grid-stride loops), and nothing else executes them there.

Each case runs one plan through accuracy.check_execute_streamed() in one direction, out of place and then in place: every transform
against float64, guards, the untouched input, in place bit-identical to out of place.  Input, output and checks go in slices, so
the host holds a few GiB whatever the batch.  A case is skipped only when the device has too little free memory for it; the skip
reason gives what it needs and what was free."""
import ctypes as C

import numpy as np
import pytest

import accuracy as A

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
GiB = 1 << 30


def _free_bytes(lib):
    tot, av = C.c_size_t(), C.c_size_t()
    lib.fft_gpu_get_memory_info_hip(C.byref(tot), C.byref(av))
    return av.value


def _need_or_skip(lib, n, batch, dtype, staged=False):
    """Two guarded buffers (input and output; the in-place buffer replaces the input), plus the staged copy of the input that a
    team plan's first in-place execute makes; 1 GiB of slack for the runtime."""
    buf = (batch + 2) * n * np.dtype(dtype).itemsize
    need = 2 * buf + (batch * n * np.dtype(dtype).itemsize if staged else 0) + GiB
    free = _free_bytes(lib)
    print("large-index case n=%d batch=%d %s: need %.1f GiB, free %.1f GiB" % (n, batch, np.dtype(dtype).name, need / GiB, free / GiB))
    if free < need:
        pytest.skip("needs %.1f GiB of free device memory, %.1f GiB free" % (need / GiB, free / GiB))


def _expect_one_launch(plan, batch, passes, algo=None):
    def check():
        info = plan.info()
        assert info.n_passes == passes and info.chunk_batch == batch and info.team_tiles == 0, \
            (info.n_passes, info.chunk_batch, info.team_tiles)
        if algo is not None:
            assert info.algo == algo, info.algo
    return check


# (id, log2n, batch, dtype, algo, direction, n_passes, family)
ONE_LAUNCH = [
    ("rows_fixed_shape", 10, (1 << 21) + 3, C64, "auto", -1, 1, "multipass"),          # 2^31 + 3072 elements, the ROWS_FIX8 tile
    ("rows_many_tiles_per_wg", 4, (1 << 27) + 5, C64, "auto", 1, 1, "multipass"),      # 2^31 + 80: ~2^20 tiles of 128 transforms
    ("shfl_grid_stride", 9, (1 << 22) + 7, C64, "radix2_shfl", -1, 1, "radix2_shfl"),  # 2^31 + 3584
    ("global_radix2", 6, (1 << 25) + 9, C64, "radix2_global", 1, 7, "radix2_global"),  # 2^31 + 576
    ("wide_row", 13, (1 << 18) + 1, C64, "auto", -1, 1, "wide_row"),                   # 2^31 + 8192
    ("n1_int_max", 0, (1 << 31) - 1, C64, "auto", 1, 1, "multipass"),                   # 2^31 - 1: bit-exact identity
    ("fp64_direct_rows", 12, (1 << 17) + 5, C128, "auto", 1, 1, "multipass"),         # 2^29 + 20480 complex128: byte offsets past 2^33
    ("past_2_32", 8, (1 << 24) + 1, C64, "auto", -1, 1, "multipass"),                  # 2^32 + 256
]


@pytest.mark.parametrize("case", ONE_LAUNCH, ids=[c[0] for c in ONE_LAUNCH])
def test_one_launch_past_2_31_elements(gpu_lib, case):
    import fftlib
    name, log2n, batch, dtype, algo, d, passes, family = case
    n = 1 << log2n
    plan = fftlib.Plan(n, batch, d, dtype, fftlib.ALGO_NAMES[algo])
    try:
        _need_or_skip(gpu_lib, n, batch, dtype)
        A.check_execute_streamed(plan, n, batch, dtype, seed=77 + log2n, family=family, exact=(n == 1),
                                 expect=_expect_one_launch(plan, batch, passes,
                                                           fftlib.ALGO_NAMES[algo] if algo != "auto" else None),
                                 label="%s: n=%d batch=%d dir=%+d" % (name, n, batch, d), long_rows=1 if dtype == C128 else 0)
    finally:
        plan.destroy()


def test_config4_on_one_gpu_plus_one(gpu_lib):
    """BASELINE config 4 on ONE GPU plus one transform: n = 2^18 fp32 x (2^13 + 1), 2^31 + 2^18 elements.  The team kernel
    (team_quad_kernel, status 0) does the work; then the same plan with the team kernel switched off runs the multi-pass schedule in
    launch groups."""
    import fftlib
    log2n, batch = 18, (1 << 13) + 1
    n = 1 << log2n
    plan = fftlib.Plan(n, batch, 1, C64)
    try:
        info = plan.info()
        assert info.team_tiles == 4 and info.team_kernel == 3, (info.team_tiles, info.team_kernel)
        _need_or_skip(gpu_lib, n, batch, C64, staged=True)

        def team_did_it():
            assert plan.team_status() == 0, "the team kernel must have done the work (status %d)" % plan.team_status()
            assert plan.info().team_kernel == 3

        A.check_execute_streamed(plan, n, batch, C64, seed=18, family="team_quad", expect=team_did_it,
                                 label="config 4 + 1, team kernel")
        plan.set_option(fftlib.OPT_TEAM_ENABLE, 0)
        chunk = plan.info().chunk_batch
        assert 1 <= chunk < batch and plan.info().n_passes == 2, (chunk, plan.info().n_passes)
        A.check_execute_streamed(plan, n, batch, C64, seed=18, family="multipass", expect=lambda: plan.info().team_tiles == 0 or
                                 pytest.fail("the team kernel is still planned"),
                                 label="config 4 + 1, multi-pass in launch groups of %d" % chunk)
    finally:
        plan.destroy()
