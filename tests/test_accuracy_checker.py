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
    for fam in A.BOUND_K:
        if fam != "bluestein":
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
