"""The cases at which the 3D transform plan (csrc/fft_plans_ext.h Plan3D; csrc/fft_kernels_plane.h plane_fft_kernel) is checked against
numpy, on the GPU (tests/test_gpu_fft3d.py) and in the CPU emulation (tests/test_emulated_fft3d.py), with the inputs, the reference and
the checkers both files share.  Test infrastructure only.

A backend is a function
    run_plan(depth, rows, cols, n_volumes, inverse, dtype, in_ptr, out_ptr, no_fusion=False, lds_budget=0) -> (rc, info)
that builds ONE plan (dtype: the complex dtype), executes, waits and destroys the plan: rc 0 / -1 plan refused / -2 execute refused;
info = dict(fused, n_passes).  lds_budget exists in the emulation only.

Reference: numpy.fft.fftn / ifftn over the last three axes in float64.
Error: per volume max |y - ref| / RMS(ref), in units of u log2(depth rows cols) (u = 2^-24 / 2^-53; a single point counts log2 as 1).
Bound: K = 8, the ladders' constant for one transform.  Worst measured: profiles/fft3d_accuracy_report.json.
"""
import numpy as np

import accuracy as A
import filter_ladder as FL

C64, C128 = np.dtype(np.complex64), np.dtype(np.complex128)
BOTH = (C64, C128)
BOUND_K = 8


class Case:
    """V volumes of depth x rows x cols; fused: True / False the path the plan must report, None: only recorded."""

    def __init__(self, depth, rows, cols, V=3, fused=True, no_fusion=False, why=""):
        self.depth, self.rows, self.cols, self.V, self.fused, self.no_fusion, self.why = depth, rows, cols, V, fused, no_fusion, why
        self.name = "%dx%dx%d%s" % (depth, rows, cols, "-no-fusion" if no_fusion else "")

    def __repr__(self):
        return self.name

    @property
    def n(self):
        return self.depth * self.rows * self.cols


FUSED = [
    Case(2, 8, 8, why="the smallest plane; an fp32 row is exactly 64 bytes"),
    Case(8, 8, 16, why="rows != cols"), Case(4, 16, 8, why="rows != cols, the other way round"),
    Case(8, 64, 64, why="the largest plane every device must take: several LDS exchanges in both steps, two strips in fp64"),
    Case(1, 16, 16, why="the plane kernel alone"),
    Case(3, 16, 16, why="plane kernel plus the transpose route along depth"),
    Case(1024, 8, 8, V=1, why="more planes than workgroups, several planes per tile, the long-depth column rule"),
    Case(2, 128, 128, V=1, fused=None, why="the path is recorded, not demanded (MI355X: the composition, see Plan3D::take_unprefetched)"),
]
COMPOSITION = [
    Case(1, 1, 1, fused=False), Case(2, 3, 4, fused=False), Case(5, 6, 7, fused=False),
    Case(8, 8, 4, fused=False, why="cols below the plane minimum"),
    Case(4, 12, 16, fused=False), Case(8, 16, 12, fused=False),
    Case(8, 16, 16, fused=False, no_fusion=True, why="the composition at a shape the plane kernel takes"),
]
OPERATOR = [Case(4, 16, 16), Case(4, 12, 16, fused=False)]  # one fused, one composition shape


def volumes(case, dtype, seed=11):
    rng = np.random.default_rng((seed, case.depth, case.rows, case.cols))
    s = (case.V, case.depth, case.rows, case.cols)
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(dtype)


def reference(x, inverse):
    return (np.fft.ifftn if inverse else np.fft.fftn)(x.astype(np.complex128), axes=(-3, -2, -1))


def errors(y, ref):
    return FL.errors(y.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1))


def unit(dtype, case):
    return A.U[np.dtype(dtype)] * max(1.0, np.log2(case.n))


def run_once(run_plan, case, dtype, x, inverse, in_place=False, lds_budget=0):
    """One plan on guarded, NaN-gapped buffers (one row of the Flat per volume).  Returns (y [V][depth][rows][cols], info); asserts rc, the
    guards and -- out of place -- the input."""
    dt = np.dtype(dtype)
    fi = FL.Flat(case.V, case.n, case.n, dt)
    fo = fi if in_place else FL.Flat(case.V, case.n, case.n, dt)
    try:
        flat = np.ascontiguousarray(x.reshape(case.V, case.n))
        if not in_place:
            fo.put(None)
        fi.put(flat)
        rc, info = run_plan(case.depth, case.rows, case.cols, case.V, inverse, dt, fi.ptr, fo.ptr, no_fusion=case.no_fusion, lds_budget=lds_budget)
        assert rc == 0, (case, rc)
        y, ok = fo.get()
        assert ok, "%s: the execute wrote outside its volumes" % case
        if not in_place:
            back, ok = fi.get()
            assert ok and np.array_equal(back.view(np.uint8), flat.view(np.uint8)), "%s: the execute changed its input" % case
        return y.reshape(x.shape), info
    finally:
        fi.free()
        if fo is not fi:
            fo.free()


def check(run_plan, case, dtype, inverse, in_place=False, lds_budget=0, want_fused="case", report=True):
    """Every value of every volume within BOUND_K u log2(depth rows cols) of numpy's; prints before it asserts."""
    dt = np.dtype(dtype)
    x = volumes(case, dt)
    y, info = run_once(run_plan, case, dt, x, inverse, in_place, lds_budget)
    e = errors(y, reference(x, inverse)) / unit(dt, case)
    label = "%s %s %s%s%s" % (case, "ifftn" if inverse else "fftn", dt.name, " in place" if in_place else "", " lds %d" % lds_budget if lds_budget else "")
    print("%s: fused %d, launches %d, worst e / (u log2 n) = %.3f (volume %d)" % (label, info["fused"], info["n_passes"], float(np.max(e)), int(np.argmax(e))))
    if report:
        A._note("fft3d_fused" if info["fused"] else "fft3d_composition", dt, case.n, None, np.max(e), unit=1.0)
    want = case.fused if want_fused == "case" else want_fused
    if want is not None:
        assert info["fused"] == (1 if want else 0), (label, info)
    assert float(np.max(e)) <= BOUND_K, "%s: %.3f u log2 n > %d" % (label, float(np.max(e)), BOUND_K)
    return y, info


def check_case(run_plan, case, dtype):
    """forward and inverse, out of place and in place"""
    for inverse in (False, True):
        for in_place in (False, True):
            check(run_plan, case, dtype, inverse, in_place)


def check_impulse(run_plan, case, dtype):
    """A unit impulse at an interior (d0, r0, c0) of volume 1 (the others hold zeros) against the closed-form product of three
    exponentials; the zero volumes give exact zeros."""
    dt = np.dtype(dtype)
    d0, r0, c0 = case.depth - 2, case.rows // 2 + 1, case.cols // 3 + 1
    x = np.zeros((case.V, case.depth, case.rows, case.cols), dtype=dt)
    x[1, d0, r0, c0] = 1.0
    kd, kr, kc = np.meshgrid(np.arange(case.depth), np.arange(case.rows), np.arange(case.cols), indexing="ij")
    ref = np.zeros(x.shape, dtype=np.complex128)
    ref[1] = (np.exp(-2j * np.pi * (kd * d0 % case.depth) / case.depth) * np.exp(-2j * np.pi * (kr * r0 % case.rows) / case.rows)
              * np.exp(-2j * np.pi * (kc * c0 % case.cols) / case.cols))
    y, info = run_once(run_plan, case, dt, x, False)
    assert info["fused"] == (1 if case.fused else 0), info
    e = float(errors(y[1:2], ref[1:2])[0]) / unit(dt, case)
    print("impulse %s %s: %.3f u log2 n" % (case, dt.name, e))
    assert e <= BOUND_K
    assert np.all(y[0] == 0) and np.all(y[2] == 0), "zeros in, something else out"


def check_linear_operator(run_plan, case, dtype, inverse):
    """Input times 2 gives output times 2, bit-exact; zeros give zeros; a volume of NaN leaves its neighbours bit-identical."""
    dt = np.dtype(dtype)
    x = volumes(case, dt)
    y, info = run_once(run_plan, case, dt, x, inverse)
    assert info["fused"] == (1 if case.fused else 0), info
    y2, _ = run_once(run_plan, case, dt, x * dt.type(2), inverse)
    assert np.array_equal(y2, y * dt.type(2)), "scaling by 2 is not exact (%s)" % case
    yz, _ = run_once(run_plan, case, dt, np.zeros_like(x), inverse)
    assert np.all(yz == 0), "zeros in, something else out (%s)" % case
    xp = x.copy()
    xp[1] = np.nan
    yp, _ = run_once(run_plan, case, dt, xp, inverse)
    for v in (0, 2):
        assert np.array_equal(yp[v].view(np.uint8), y[v].view(np.uint8)), "volume %d changed next to a volume of NaN (%s)" % (v, case)
    assert np.all(np.isnan(yp[1].real) | np.isnan(yp[1].imag))
