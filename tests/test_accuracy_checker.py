"""The per-transform accuracy checker of tests/accuracy.py, tested on numpy data at the shapes the GPU tests use (no GPU).

A correct result passes; one wrong bin, a 16-byte value pair from another transform, two swapped transforms, a NaN, a changed
guard word and a changed input word are each flagged.  check_execute() runs here on host memory with a numpy "plan"."""
import ctypes as C

import numpy as np
import pytest

import accuracy as A


@pytest.fixture(scope="module")
def batches():
    """16 x 2^20 fp32 and 8 x 2^19 fp64 normal inputs, their numpy results (complex64 computed in fp32: a correct result with
    ordinary fp32 rounding) and the float64 references."""
    out = {}
    for n, batch, dt in ((1 << 20, 16, np.complex64), (1 << 19, 8, np.complex128)):
        x = A.normal_rows(n, 0, batch, dt, seed=3)
        y = np.fft.fft(x, axis=1)
        assert y.dtype == np.dtype(dt)
        out[np.dtype(dt)] = (x, y)
    return out


def _flagged(y, x, family="team_quad"):
    with pytest.raises(A.AccuracyError) as ei:
        A.check_rows(y, x, -1, family, label="self-test")
    return str(ei.value)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_correct_result_passes(batches, dt):
    x, y = batches[np.dtype(dt)]
    e = A.check_rows(y, x, -1, "team_quad", label="numpy", long_rows=2 if dt == np.complex128 else 0)
    assert e.shape == (x.shape[0],) and np.all(np.isfinite(e))
    assert np.max(e) <= A.bound("team_quad", dt, x.shape[1]) / 2
    # the inverse (scaled by 1/n) is measured by the same scale-free metric
    yi = np.fft.ifft(x, axis=1)
    A.check_rows(yi, x, 1, "team_quad", label="numpy inverse")


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_one_bin_off_by_ten_bounds(batches, dt):
    x, y = batches[np.dtype(dt)]
    n = x.shape[1]
    y = y.copy()
    X = A.fft_ref(x[5], -1)
    rms = np.linalg.norm(X) / np.sqrt(n)
    y[5, 12345] += 10 * A.bound("team_quad", dt, n) * rms
    msg = _flagged(y, x)
    assert "1 of %d" % x.shape[0] in msg and "worst transform 5 (bin 12345" in msg, msg


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_sixteen_byte_pair_from_another_transform(batches, dt):
    x, y = batches[np.dtype(dt)]
    y = y.copy()
    k = 777 * 16 // y.itemsize
    y.view(np.uint8)[3, k * y.itemsize:k * y.itemsize + 16] = y.view(np.uint8)[4, k * y.itemsize:k * y.itemsize + 16]
    msg = _flagged(y, x)
    assert "1 of %d" % x.shape[0] in msg and "worst transform 3 (bin %d" % (k + (1 if "bin %d," % (k + 1) in msg else 0)) in msg, msg


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_two_transforms_swapped(batches, dt):
    x, y = batches[np.dtype(dt)]
    y = y.copy()
    y[[1, 6]] = y[[6, 1]]
    msg = _flagged(y, x)
    assert "2 of %d" % x.shape[0] in msg and "[1, 6]" in msg, msg


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_one_nan(batches, dt):
    x, y = batches[np.dtype(dt)]
    y = y.copy()
    y.view(y.real.dtype)[x.shape[0] - 1, 2 * 999 + 1] = np.nan
    msg = _flagged(y, x)
    assert "worst transform %d (bin 999" % (x.shape[0] - 1) in msg and "non-finite 1" in msg, msg


def test_bound_table_within_caps():
    for fam, k in A.BOUND_K.items():
        assert 0 < k <= A.CAP.get(fam, A.POW2_CAP), fam
    assert A.CAP["bluestein"] <= 64 and A.POW2_CAP <= 16
    assert set(A.CAP) == {"bluestein", "fused_conv", "fused_corr", "psd"} and all(c <= 64 for c in A.CAP.values())
    for fam in A.BOUND_K:
        if fam not in A.CAP:  # the families capped at POW2_CAP
            assert A.bound(fam, np.complex64, 1 << 20) < 2e-5, fam
    assert A.bound("bluestein", np.complex128, 1000003, m=1 << 21) == A.BOUND_K["bluestein"] * 2.0 ** -53 * 21  # log2(m), not log2(n)


# ---------------------------------------------------------------------------------------------------------------------------
# check_execute on host memory: a "plan" that computes the transform with numpy, optionally with a defect
# ---------------------------------------------------------------------------------------------------------------------------
class HostMemory:
    def __init__(self):
        self.live = {}

    def alloc(self, nbytes):
        a = np.empty(nbytes + 16, dtype=np.uint8)
        off = (-a.ctypes.data) % 16
        ptr = a.ctypes.data + off
        self.live[ptr] = a
        return ptr, ptr

    def free(self, handle):
        self.live.pop(handle, None)

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        C.memmove(dptr, arr.ctypes.data, arr.nbytes)

    def d2h(self, dptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        C.memmove(out.ctypes.data, dptr, out.nbytes)
        return out


class NumpyPlan:
    def __init__(self, n, batch, direction, dtype, defect=None):
        self.n, self.batch, self.direction, self.dtype, self.defect = n, batch, direction, np.dtype(dtype), defect

    def execute_ptr(self, d_in, d_out):
        mem = A.memory()
        x = mem.d2h(d_in, (self.batch, self.n), self.dtype)
        y = (np.fft.fft(x, axis=1) if self.direction < 0 else np.fft.ifft(x, axis=1)).astype(self.dtype)
        mem.h2d(d_out, y)
        rb = self.n * self.dtype.itemsize
        if self.defect == "guard" and d_in != d_out:
            mem.h2d(d_out + self.batch * rb + 8, np.zeros(1, np.uint32))  # one word past the end of the output
        if self.defect == "input" and d_in != d_out:
            mem.h2d(d_in + 3 * rb + 40, np.zeros(1, np.uint32))  # one word of the input

    def sync(self):
        return 0


@pytest.fixture
def host_memory(monkeypatch):
    monkeypatch.setattr(A, "MEMORY", HostMemory())


@pytest.mark.parametrize("dt,n,batch", [(np.complex64, 1 << 20, 16), (np.complex128, 1 << 19, 8)])
def test_check_execute_on_host_memory(host_memory, dt, n, batch):
    x = A.normal_rows(n, 0, batch, dt, seed=11)
    for d in (-1, 1):
        e = A.check_execute(NumpyPlan(n, batch, d, dt), x, "team_quad", label="numpy plan")
        assert e.shape == (batch,) and np.max(e) <= A.bound("team_quad", dt, n) / 2
    with pytest.raises(AssertionError, match="wrote outside"):
        A.check_execute(NumpyPlan(n, batch, -1, dt, defect="guard"), x, "team_quad")
    with pytest.raises(AssertionError, match="changed its input"):
        A.check_execute(NumpyPlan(n, batch, -1, dt, defect="input"), x, "team_quad")


def test_check_execute_sees_unwritten_output(host_memory):
    """A transform the plan never writes keeps the NaN fill and is flagged."""
    n, batch = 1 << 16, 5
    x = A.normal_rows(n, 0, batch, np.complex64, seed=2)

    class SkipsLast(NumpyPlan):
        def execute_ptr(self, d_in, d_out):
            mem = A.memory()
            xs = mem.d2h(d_in, (self.batch - 1, self.n), self.dtype)
            mem.h2d(d_out, np.fft.fft(xs, axis=1))

    with pytest.raises(A.AccuracyError, match="worst transform 4 .*non-finite 1"):
        A.check_execute(SkipsLast(n, batch, -1, np.complex64), x, "team_quad", inplace=False)


def test_rows_are_regenerable():
    a = A.normal_rows(4096, 0, 10, np.complex64, seed=5)
    b = A.normal_rows(4096, 7, 3, np.complex64, seed=5)
    assert np.array_equal(a[7:], b)
    assert not np.array_equal(a[0], a[1])


def test_two_tone_check_every_transform():
    """check_two_tone: numpy's fp32 result of two-tone inputs passes; one bin of one transform off, or one peak short, is flagged."""
    import oracle_lib as O
    n, batch = 1 << 16, 70
    x = O.gen_two_tone(n, 5, batch, np.complex64)
    y = np.fft.fft(x, axis=1)
    assert np.max(A.check_two_tone(y, 5, n, "multipass")) <= A.bound_two_tone("multipass", np.complex64, n) / 2
    lim = A.bound_two_tone("multipass", np.complex64, n) * np.sqrt(1.25 * n)
    bad = y.copy()
    bad[65, 777] += 3 * lim
    with pytest.raises(A.AccuracyError, match="worst transform 70 \\(bin 777"):
        A.check_two_tone(bad, 5, n, "multipass")
    bad = y.copy()
    f, _ = O.two_tone_bins(n, 5 + 66)
    bad[66, f] -= 3 * lim
    with pytest.raises(A.AccuracyError, match="worst transform 71 \\(bin %d" % f):
        A.check_two_tone(bad, 5, n, "multipass")


# ---------------------------------------------------------------------------------------------------------------------------
# check_execute_streamed on host memory, with SLICE_BYTES small enough that the batch spans four slices
# ---------------------------------------------------------------------------------------------------------------------------
STREAM_N, STREAM_BATCH, STREAM_SEED = 256, 1000, 21


class StreamedPlan(NumpyPlan):
    """A numpy plan on host memory; `defect` names one kind of wrong result or stray write."""

    def execute_ptr(self, d_in, d_out):
        mem = A.memory()
        n, batch, rb = self.n, self.batch, self.n * self.dtype.itemsize
        x = mem.d2h(d_in, (batch, n), self.dtype)
        y = (np.fft.fft(x, axis=1) if self.direction < 0 else np.fft.ifft(x, axis=1)).astype(self.dtype)
        step = A._slice_rows(16 * n)
        if self.defect == "bin_last_slice":
            b = batch - 2
            y[b, 77] += 1e3 * A.bound("multipass", self.dtype, n) * np.sqrt(np.mean(np.abs(y[b]) ** 2))
        elif self.defect == "swap_across_slices":
            y[[step - 1, step]] = y[[step, step - 1]]
        elif self.defect == "wrapped_index":
            w = np.empty_like(y)
            w[:] = np.nan
            for b in range(batch):
                w[b % 512] = y[b]  # transform b written at row b mod 2^9: an index that wraps, scaled down from 2^31
            y = w if d_in != d_out else np.where(np.isnan(w), x, w)
        elif self.defect == "last_unwritten":
            y = y[:-1]
        mem.h2d(d_out, y)
        if self.defect == "guard" and d_in != d_out:
            mem.h2d(d_out - 4, np.zeros(1, np.uint32))  # the last word of the guard row before the output
        if self.defect == "input_later_slice" and d_in != d_out:
            mem.h2d(d_in + (2 * step + 5) * rb + 8, np.zeros(1, np.uint32))


@pytest.fixture
def small_slices(host_memory, monkeypatch):
    monkeypatch.setattr(A, "SLICE_BYTES", 16 * STREAM_N * 300)  # 300 rows per slice: 1000 rows in four slices


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_streamed_correct_plan_passes(small_slices, dt):
    assert -(-STREAM_BATCH // A._slice_rows(16 * STREAM_N)) >= 3
    for d in (-1, 1):
        seen = []
        e = A.check_execute_streamed(StreamedPlan(STREAM_N, STREAM_BATCH, d, dt), STREAM_N, STREAM_BATCH, dt, STREAM_SEED, "multipass",
                                     label="numpy plan", expect=lambda: seen.append(1), long_rows=2 if dt == np.complex128 else 0)
        assert 0 <= e <= A.bound("multipass", dt, STREAM_N) / 2
        assert len(seen) == 2  # after the out-of-place and the in-place sync


@pytest.mark.parametrize("defect,match", [
    ("bin_last_slice", "1 of 100 transforms over the bound.*worst transform 998 \\(bin 77"),
    ("swap_across_slices", "worst transform 29[9]"),
    ("wrapped_index", "300 of 300 transforms over the bound"),  # rows 0 .. 511 hold transforms 512 .. 999
    ("last_unwritten", "worst transform 999 .*non-finite 1"),
    ("guard", "wrote outside"),
    ("input_later_slice", "changed its input \\(transform 605\\)"),
])
def test_streamed_defects_flagged(small_slices, defect, match):
    plan = StreamedPlan(STREAM_N, STREAM_BATCH, -1, np.complex64, defect=defect)
    with pytest.raises(AssertionError, match=match):
        A.check_execute_streamed(plan, STREAM_N, STREAM_BATCH, np.complex64, STREAM_SEED, "multipass", label="defect " + defect)


def test_streamed_in_place_must_match_out_of_place(small_slices):
    class InPlaceDiffers(StreamedPlan):
        def execute_ptr(self, d_in, d_out):
            super().execute_ptr(d_in, d_out)
            if d_in == d_out:  # one last-bit change in the third slice: within the bound, but not the same bits
                mem = A.memory()
                w = mem.d2h(d_out + 700 * STREAM_N * 8, (1,), np.uint32)
                mem.h2d(d_out + 700 * STREAM_N * 8, w ^ np.uint32(1))

    with pytest.raises(AssertionError, match="in-place result differs from the out-of-place one at transform 700"):
        A.check_execute_streamed(InPlaceDiffers(STREAM_N, STREAM_BATCH, -1, np.complex64), STREAM_N, STREAM_BATCH, np.complex64,
                                 STREAM_SEED, "multipass")


def test_streamed_exact_flags_any_changed_word(small_slices):
    """exact=True (n = 1 plans): the output must be the input bit for bit."""
    class Identity(NumpyPlan):
        def execute_ptr(self, d_in, d_out):
            mem = A.memory()
            x = mem.d2h(d_in, (self.batch, 1), self.dtype)
            x[640, 0] = np.nextafter(x[640, 0].real, np.float32(np.inf)) + 1j * x[640, 0].imag
            mem.h2d(d_out, x)

    A.check_execute_streamed(NumpyPlan(1, 5000, -1, np.complex64), 1, 5000, np.complex64, 3, "multipass", exact=True)
    with pytest.raises(AssertionError, match="output differs from the input at transform 640"):
        A.check_execute_streamed(Identity(1, 5000, -1, np.complex64), 1, 5000, np.complex64, 3, "multipass", exact=True)


def test_block_rows_are_regenerable():
    n, dt = 64, np.complex64
    R = A.block_rows(n, dt)
    a = A.block_normal_rows(n, 0, 3 * R + 5, dt, seed=9)
    b = A.block_normal_rows(n, R - 2, R + 7, dt, seed=9)  # across a block boundary
    assert np.array_equal(a[R - 2:2 * R + 5], b)
    assert not np.array_equal(a[R - 1], a[R]) and not np.array_equal(a[0], a[1])
    assert not np.array_equal(a[:R], A.block_normal_rows(n, 0, R, dt, seed=10))
    c = A.block_normal_rows(4096, 0, 300, np.complex128, seed=2)
    assert np.array_equal(c[123:201], A.block_normal_rows(4096, 123, 78, np.complex128, seed=2))


# ---------------------------------------------------------------------------------------------------------------------------
# check_execute_io on host memory: executes whose input and output rows differ in width and type
# ---------------------------------------------------------------------------------------------------------------------------
IO_BATCH = 7
IO_SHAPES = {
    # name: (input dtype, w_in, output dtype, w_out, float64 reference of input rows)
    "truncated": (np.complex64, 40, np.complex64, 25, lambda x: np.fft.fft(x.astype(np.complex128), axis=1)[:, :25]),     # w_out < w_in, odd pitch
    "padded": (np.complex128, 25, np.complex128, 40, lambda x: np.fft.fft(x.astype(np.complex128), n=40, axis=1)),        # w_out > w_in
    "real_out": (np.complex64, 32, np.float32, 17, lambda x: np.abs(np.fft.fft(x.astype(np.complex128), axis=1)[:, :17]) ** 2),  # 68-byte rows
}


class FakeIO:
    """run(in_ptr, in2_ptr, out_ptr) of a numpy "plan": out = ref(x) (+ ref(x2)), stored row by row; `defect` names one fault."""

    def __init__(self, shape, defect=None):
        self.dt_in, self.w_in, self.dt_out, self.w_out, self.ref = IO_SHAPES[shape]
        self.dt_in, self.dt_out = np.dtype(self.dt_in), np.dtype(self.dt_out)
        self.defect, self.runs = defect, 0

    def ref2(self, x, x2):
        return self.ref(x) + self.ref(x2)

    def __call__(self, in_ptr, in2_ptr, out_ptr):
        mem = A.memory()
        self.runs += 1
        x = mem.d2h(in_ptr, (IO_BATCH, self.w_in), self.dt_in)
        y = self.ref(x)
        if in2_ptr is not None:
            y = y + self.ref(mem.d2h(in2_ptr, (IO_BATCH, self.w_in), self.dt_in))
        y = y.astype(self.dt_out)
        d = self.defect
        if d == "swap":
            y[[2, 5]] = y[[5, 2]]
        elif d == "neighbour_bin":
            y[3, 11] = y[4, 11]
        elif d == "tail_nan":
            y[4, self.w_out - 1] = np.nan
        rb = self.w_out * self.dt_out.itemsize
        for b in range(IO_BATCH):  # the store order of a kernel that walks the rows
            if d == "tail_unwritten" and b == 4:
                mem.h2d(out_ptr + b * rb, y[b, :-1])
                continue
            mem.h2d(out_ptr + b * rb, y[b])
            if d == "past_row":  # one element past the row: the next row's first element, which that row's own store then repairs
                mem.h2d(out_ptr + (b + 1) * rb, y[b, :1])
        if d == "guard":
            mem.h2d(out_ptr + IO_BATCH * rb, np.zeros(1, np.uint32))  # the first word of the trailing guard
        if d == "input2" and in2_ptr is not None:
            mem.h2d(in2_ptr + 5 * self.w_in * self.dt_in.itemsize + 8, np.zeros(1, np.uint32))
        if d == "inplace_differs" and in_ptr == out_ptr:
            w = mem.d2h(out_ptr + 3 * rb, (1,), np.uint32)
            mem.h2d(out_ptr + 3 * rb, w ^ np.uint32(1))


def _io_check(shape, defect=None, second=True, inplace=False):
    f = FakeIO(shape, defect)
    x = A.normal_rows(f.w_in, 0, IO_BATCH, f.dt_in, seed=31)
    x2 = A.normal_rows(f.w_in, 100, IO_BATCH, f.dt_in, seed=31) if second else None
    e = A.check_execute_io(f, x, f.w_out, f.dt_out, "multipass", f.ref2 if second else f.ref, x2=x2, n=40, inplace=inplace,
                           label="fake " + shape)
    return f, e


@pytest.mark.parametrize("shape", sorted(IO_SHAPES))
def test_io_correct_execute_passes(host_memory, shape):
    f, e = _io_check(shape, second=True)
    assert e.shape == (IO_BATCH,) and np.all(np.isfinite(e)) and f.runs == 1
    f, e = _io_check(shape, second=False, inplace=True)
    assert f.runs == 2 and np.max(e) <= A.bound("multipass", f.dt_out, 40)


def test_io_payload_is_aligned_like_a_plain_allocation(host_memory):
    """68-byte rows: the guards are 80 bytes, the payload starts 16-byte aligned and the trailing guard right behind it."""
    g = A.Guarded(5, 68, align16=True)
    assert g.guard_bytes == 80 and g.ptr % 16 == 0 and g.ptr - g.base == 80
    assert g.guards_intact()
    A.h2d(g.ptr + 5 * 68, np.zeros(1, np.uint32))
    assert not g.guards_intact()
    g.free()
    assert A.Guarded(5, 64).guard_bytes == 64 and A.Guarded(5, 8).guard_bytes == 8  # check_execute's buffers are as they were


@pytest.mark.parametrize("shape", sorted(IO_SHAPES))
@pytest.mark.parametrize("defect,match", [
    ("past_row", "wrote outside"),  # every stray element but the last row's is overwritten by the next row: the guard sees the last
    ("guard", "wrote outside"),
    ("tail_nan", "worst transform 4 .*non-finite 1"),
    ("tail_unwritten", "worst transform 4 .*non-finite 1"),
    ("swap", "2 of 7 transforms over the bound.*\\[2, 5\\]"),
    ("neighbour_bin", "1 of 7 transforms over the bound.*worst transform 3 \\(bin 11"),
    ("input2", "changed its second input"),
])
def test_io_defects_flagged(host_memory, shape, defect, match):
    with pytest.raises(AssertionError, match=match):
        _io_check(shape, defect)
    _io_check(shape, None)  # the same call without the defect passes


def test_io_in_place_must_match_out_of_place(host_memory):
    with pytest.raises(AssertionError, match="in-place result differs from the out-of-place one at row 3"):
        _io_check("truncated", "inplace_differs", second=False, inplace=True)


def test_row_errors_scaled_by_the_larger_of_rms_and_bin():
    """scale="rms_or_bin": a peak's own rounding error is measured against the peak, every other bin against the row's RMS."""
    rng = np.random.default_rng(4)
    X = rng.standard_normal((3, 256))
    X[:, 0] = 1000.0  # the lag 0 of a correlation
    rms = np.sqrt(np.mean(X ** 2, axis=1))
    y = X.copy()
    y[1, 0] *= 1 + 1e-6  # a relative error of 1e-6 on the peak
    e_old, k_old = A.row_errors(y, X)
    e_new, k_new = A.row_errors(y, X, scale="rms_or_bin")
    assert k_old[1] == 0 and np.isclose(e_old[1], 1e-3 / rms[1]) and np.isclose(e_new[1], 1e-6)
    y = X.copy()
    y[2, 77] += 1e-3  # the same absolute error on an ordinary bin: unchanged by the option, unless that bin is above the RMS
    e_new, k_new = A.row_errors(y, X, scale="rms_or_bin")
    assert k_new[2] == 77 and np.isclose(e_new[2], 1e-3 / max(rms[2], abs(X[2, 77])))
    y[0, 5] = np.nan
    assert np.isinf(A.row_errors(y, X, scale="rms_or_bin")[0][0])
    with pytest.raises(ValueError):
        A.row_errors(y, X, scale="max")


# ---------------------------------------------------------------------------------------------------------------------------
# the operator checks (tests/operator_ladder.py, accuracy.check_neighbours / check_scaling / check_zeros) see what random rows cannot
# ---------------------------------------------------------------------------------------------------------------------------
import operator_ladder as OL  # noqa: E402


class DefectPlan(NumpyPlan):
    """A numpy plan with one defect of the kind only the operator checks see."""

    def __init__(self, n, batch, direction, dtype, defect=None, j0=0, k0=0, delta=0.0):
        super().__init__(n, batch, direction, dtype, defect)
        self.j0, self.k0, self.delta = j0, k0, delta

    def execute_ptr(self, d_in, d_out):
        mem = A.memory()
        x = mem.d2h(d_in, (self.batch, self.n), self.dtype)
        with np.errstate(all="ignore"):
            y = (np.fft.fft(x, axis=1) if self.direction < 0 else np.fft.ifft(x, axis=1)).astype(self.dtype)
            if self.defect == "matrix_element":    # element (j0, k0) of the matrix is off by delta
                y[:, self.k0] += self.dtype.type(self.delta) * x[:, self.j0]
            elif self.defect == "zero_multiply":   # row b gets 0 * (row b + 1): a multiply where a select belongs
                y[:-1] += self.dtype.type(0) * x[1:]
            elif self.defect == "flush":
                y[np.abs(y) < 1e-30] = 0
            elif self.defect == "unscaled_row":    # the inverse forgets 1/n on one row
                y[self.j0] *= self.n
        mem.h2d(d_out, y)


def _run_of(plan):
    return lambda i, _, o: plan.execute_ptr(i, o)


def test_perturbed_matrix_element_passes_random_rows_and_fails_the_impulse(host_memory):
    """The gap: an element of the DFT matrix off by 4 x the bound reaches a random row as 4 x bound / sqrt(n) of its RMS."""
    n, dt, j0, k0 = 4096, np.complex64, 1234, 77
    delta = 4 * A.bound("multipass", dt, n)
    x = A.normal_rows(n, 0, 16, dt, seed=5)
    A.check_execute(DefectPlan(n, 16, -1, dt, "matrix_element", j0, k0, delta), x, "multipass", label="perturbed, random rows")
    js = OL.positions(n)
    imp = OL.impulses(n, js, dt)
    A.check_execute(NumpyPlan(n, len(js), -1, dt), imp, "multipass", ref=OL.ref_1d(n, -1), kind="impulse", label="numpy, impulses")
    with pytest.raises(A.AccuracyError, match="1 of 4096 transforms over the bound.*worst transform %d \\(bin %d" % (j0, k0)):
        A.check_execute(DefectPlan(n, len(js), -1, dt, "matrix_element", j0, k0, delta), imp, "multipass", ref=OL.ref_1d(n, -1),
                        kind="impulse", label="perturbed, impulses")


def test_zero_multiply_leak_passes_every_check_but_the_poisoned_neighbour(host_memory):
    n, batch, dt = 256, 9, np.complex64
    x = A.normal_rows(n, 0, batch, dt, seed=6)
    leak = DefectPlan(n, batch, -1, dt, "zero_multiply")
    A.check_execute(leak, x, "multipass", label="leak, random rows")
    A.check_scaling(_run_of(leak), x, label="leak")
    A.check_zeros(_run_of(leak), x, label="leak")
    for poison in A.POISONS:
        A.check_neighbours(_run_of(NumpyPlan(n, batch, -1, dt)), x, [0, 4, 8], poison, label="numpy")
    with pytest.raises(A.AccuracyError, match="2 untouched result rows changed with their neighbour: rows \\[3, 7\\]"):
        A.check_neighbours(_run_of(leak), x, [0, 4, 8], "nan", label="leak")
    with pytest.raises(A.AccuracyError, match="rows \\[3, 7\\]"):
        A.check_neighbours(_run_of(leak), x, [0, 4, 8], "inf0", label="leak")
    A.check_neighbours(_run_of(leak), x, [0, 4, 8], "huge", label="leak")  # 0 * a finite value is still 0


def test_all_nan_transform_must_come_back_non_finite(host_memory):
    n, batch, dt = 64, 5, np.complex128

    class Drops(NumpyPlan):
        def execute_ptr(self, d_in, d_out):
            mem = A.memory()
            x = mem.d2h(d_in, (self.batch, self.n), self.dtype)
            y = np.fft.fft(np.nan_to_num(x), axis=1)
            mem.h2d(d_out, y)

    x = A.normal_rows(n, 0, batch, dt, seed=7)
    with pytest.raises(A.AccuracyError, match="result row 2 of an all-NaN transform has 64 finite bins"):
        A.check_neighbours(_run_of(Drops(n, batch, -1, dt)), x, [2], "nan")


def test_flush_to_zero_fails_the_scaling_property(host_memory):
    n, batch, dt = 256, 5, np.complex128
    x = A.normal_rows(n, 0, batch, dt, seed=8)
    A.check_scaling(_run_of(NumpyPlan(n, batch, -1, dt)), x, label="numpy")
    A.check_execute(DefectPlan(n, batch, -1, dt, "flush"), x, "multipass", label="flush, random rows")
    with pytest.raises(A.AccuracyError, match="execute\\(2\\^-200 x\\) differs from 2\\^-200 execute\\(x\\) in 5 rows"):
        A.check_scaling(_run_of(DefectPlan(n, batch, -1, dt, "flush")), x, label="flush")


def test_unscaled_inverse_row_fails_the_impulse_check(host_memory):
    n, dt = 256, np.complex128
    js = OL.positions(n)
    imp = OL.impulses(n, js, dt)
    OL.closed_form_checked(OL.ref_1d(n, 1), OL.ref_1d(n, 1, np.longdouble), imp, "multipass", dt, n)
    A.check_execute(NumpyPlan(n, n, 1, dt), imp, "multipass", ref=OL.ref_1d(n, 1), kind="impulse", label="numpy inverse")
    with pytest.raises(A.AccuracyError, match="1 of 256 transforms over the bound.*worst transform 99 "):
        A.check_execute(DefectPlan(n, n, 1, dt, "unscaled_row", j0=99), imp, "multipass", ref=OL.ref_1d(n, 1), kind="impulse")


def test_positions_and_closed_form():
    assert np.array_equal(OL.positions(4096), np.arange(4096))
    js = OL.positions(1 << 20)
    assert {0, 1, (1 << 20) - 1, 1 << 19, 1 << 7, (1 << 7) - 1, (1 << 20) - (1 << 7)} <= set(js.tolist()) and len(js) <= 75
    assert len(OL.positions(1 << 21)) == len({0, 1} | {x for t in range(22) for x in ((1 << t) % (1 << 21), (1 << t) - 1, (1 << 21) - (1 << t))} - {1 << 21})
    assert {4200 // 56, 4200 // 56 - 1} <= set(OL.positions(4200, [75, 56]).tolist())
    for n in (2, 3, 8, 30, 1009, 4096):  # the closed form against numpy's FFT of the impulses, both directions, and c2r / 2D
        imp = OL.impulses(n, np.arange(n), np.complex128)
        for d in (-1, 1):
            ref = np.fft.fft(imp, axis=1) if d < 0 else np.fft.ifft(imp, axis=1)
            assert np.max(np.abs(OL.ref_1d(n, d)(imp) - ref)) * (1 if d < 0 else n) < 1e-12
        half = OL.impulses(n // 2 + 1, np.arange(n // 2 + 1), np.complex128)
        assert np.max(np.abs(OL.ref_c2r(n)(half) - np.fft.irfft(half, n, axis=1))) * n < 1e-12
    imp = OL.impulses(12 * 32, np.arange(12 * 32), np.complex128)
    assert np.max(np.abs(OL.ref_2d(12, 32, -1)(imp) - np.fft.fft2(imp.reshape(-1, 12, 32)).reshape(384, -1))) < 1e-12
