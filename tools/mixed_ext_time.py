"""Timing of the 2D and real plans on the mixed-radix engine against chirp-z, one library per process:

    python tools/mixed_ext_time.py LABEL LIBRARY.so ALGO [REPEATS]

ALGO is 0 (AUTO: chirp-z for these sizes under the default policy; uses only entry points an earlier commit's library has, so
that one can be loaded as the baseline) or 7 (FFT_GPU_ALGO_MIXED_RADIX through the _algo entry points).  Sizes: 2D 1080 x 1920
and 1000 x 1000, r2c / c2r of n = 1000, 44100, 10^6, fp32 and fp64.
For every case: one plan of about 1 GiB per execute, one warm-up execute, then REPEATS timings of two executes each through
fft_gpu_execute_timed (HIP events on the plan's stream); prints median, fastest and slowest repeat.  Run the libraries
interleaved from a job script, each step under its own timeout."""
import ctypes as C
import sys

import numpy as np

BYTES = 1 << 30
MAIN_2D = ((1080, 1920), (1000, 1000))
MAIN_REAL = (1000, 44100, 10 ** 6)


def main():
    label, path, algo = sys.argv[1], sys.argv[2], int(sys.argv[3])
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.fft_gpu_init.argtypes = [i]
    for name, args in (("fft_gpu_plan_2d_ex_hip", [i] * 5), ("fft_gpu_plan_r2c_1d_hip", [i] * 3), ("fft_gpu_plan_c2r_1d_hip", [i] * 3)) + \
            ((("fft_gpu_plan_2d_algo_hip", [i] * 6), ("fft_gpu_plan_r2c_1d_algo_hip", [i] * 4), ("fft_gpu_plan_c2r_1d_algo_hip", [i] * 4)) if algo else ()):
        getattr(lib, name).restype = vp
        getattr(lib, name).argtypes = args
    lib.fft_gpu_alloc_bytes_hip.restype = vp
    lib.fft_gpu_alloc_bytes_hip.argtypes = [C.c_size_t]
    lib.fft_gpu_memory_ptr.restype = vp
    lib.fft_gpu_memory_ptr.argtypes = [vp]
    lib.fft_gpu_execute_timed.argtypes = [vp, vp, vp, i, C.POINTER(C.c_float)]
    lib.fft_gpu_destroy_plan.argtypes = [vp]
    lib.fft_gpu_free.argtypes = [vp]
    lib.fft_gpu_copy_h2d_bytes_hip.argtypes = [vp, vp, C.c_size_t]
    if lib.fft_gpu_init(-1) != 0:
        raise SystemExit("no device")
    noise = np.random.default_rng(1).standard_normal(1 << 22)

    def plan_2d(rows, cols, nm, prec):
        return lib.fft_gpu_plan_2d_algo_hip(rows, cols, nm, -1, prec, algo) if algo else lib.fft_gpu_plan_2d_ex_hip(rows, cols, nm, -1, prec)

    def plan_real(n, batch, prec, r2c):
        if algo:
            return (lib.fft_gpu_plan_r2c_1d_algo_hip if r2c else lib.fft_gpu_plan_c2r_1d_algo_hip)(n, batch, prec, algo)
        return (lib.fft_gpu_plan_r2c_1d_hip if r2c else lib.fft_gpu_plan_c2r_1d_hip)(n, batch, prec)

    def time_plan(what, plan, in_bytes, out_bytes, prec, points):
        if not plan:
            raise SystemExit("plan failed: " + what)
        a, b = lib.fft_gpu_alloc_bytes_hip(in_bytes), lib.fft_gpu_alloc_bytes_hip(out_bytes)
        if not (a and b):
            raise SystemExit("allocation failed: " + what)
        x = np.resize(noise.astype(np.float32) if prec else noise, in_bytes // (4 if prec else 8))
        lib.fft_gpu_copy_h2d_bytes_hip(a, x.ctypes.data, x.nbytes)
        ms = C.c_float()
        da, db = lib.fft_gpu_memory_ptr(a), lib.fft_gpu_memory_ptr(b)
        assert lib.fft_gpu_execute_timed(plan, da, db, 1, C.byref(ms)) == 0
        ts = []
        for _ in range(reps):
            assert lib.fft_gpu_execute_timed(plan, da, db, 2, C.byref(ms)) == 0
            ts.append(ms.value / 2)
        t = float(np.median(ts))
        print("%-10s algo=%d %s %-22s ms median %8.3f min %8.3f max %8.3f  %7.1f Gpoint/s" %
              (label, algo, "fp32" if prec else "fp64", what, t, min(ts), max(ts), points / t / 1e6), flush=True)
        lib.fft_gpu_destroy_plan(plan)
        lib.fft_gpu_free(a)
        lib.fft_gpu_free(b)

    for prec, esz in ((1, 8), (0, 16)):
        for rows, cols in MAIN_2D:
            nm = max(1, BYTES // (rows * cols * esz))
            nbytes = rows * cols * nm * esz
            time_plan("2d %dx%d x%d" % (rows, cols, nm), plan_2d(rows, cols, nm, prec), nbytes, nbytes, prec, rows * cols * nm)
        for n in MAIN_REAL:
            batch = max(1, BYTES // (n * esz // 2))
            rb, cb = n * batch * (esz // 2), (n // 2 + 1) * batch * esz
            time_plan("r2c n=%d x%d" % (n, batch), plan_real(n, batch, prec, True), rb, cb, prec, n * batch)
            time_plan("c2r n=%d x%d" % (n, batch), plan_real(n, batch, prec, False), cb, rb, prec, n * batch)


if __name__ == "__main__":
    main()
