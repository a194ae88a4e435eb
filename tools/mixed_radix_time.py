"""Timing of the mixed-radix plan against chirp-z, one library per process:

    python tools/mixed_radix_time.py LABEL LIBRARY.so ALGO [REPEATS]

ALGO is 0 (AUTO: chirp-z for these lengths under the default policy) or 7 (FFT_GPU_ALGO_MIXED_RADIX).  For every size and
precision: one plan of about 1 GiB per execute, one warm-up execute, then REPEATS timings of two executes each through
fft_gpu_execute_timed (HIP events on the plan's stream); prints the median and the spread of the repeats, Gpoint/s and the
algorithmic TB/s (2 * n * sizeof per transform).  Plain ctypes on the few entry points used, so that a library built from an
earlier commit can be loaded as the baseline.  Run the two libraries interleaved from a job script, each step under its own
timeout."""
import ctypes as C
import sys

import numpy as np

SIZES = (1000, 1080, 1920, 3000, 3600, 4000, 44100, 100000, 10 ** 6, 2073600)
BYTES = 1 << 30


def main():
    label, path, algo = sys.argv[1], sys.argv[2], int(sys.argv[3])
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.fft_gpu_init.argtypes = [i]
    lib.fft_gpu_plan_1d_ex.restype = vp
    lib.fft_gpu_plan_1d_ex.argtypes = [i, i, i, i, i]
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
    for prec, esz in ((1, 8), (0, 16)):
        for n in SIZES:
            batch = max(1, BYTES // (n * esz))
            nbytes = n * batch * esz
            a, b = lib.fft_gpu_alloc_bytes_hip(nbytes), lib.fft_gpu_alloc_bytes_hip(nbytes)
            plan = lib.fft_gpu_plan_1d_ex(n, batch, -1, prec, algo)
            if not (a and b and plan):
                raise SystemExit("allocation or plan failed at n=%d" % n)
            x = np.random.default_rng(n).standard_normal(nbytes // 8 if prec else nbytes // 16 * 2, dtype=np.float32 if prec else np.float64)
            lib.fft_gpu_copy_h2d_bytes_hip(a, x.ctypes.data, x.nbytes)
            ms = C.c_float()
            da, db = lib.fft_gpu_memory_ptr(a), lib.fft_gpu_memory_ptr(b)
            assert lib.fft_gpu_execute_timed(plan, da, db, 1, C.byref(ms)) == 0
            ts = []
            for _ in range(reps):
                assert lib.fft_gpu_execute_timed(plan, da, db, 2, C.byref(ms)) == 0
                ts.append(ms.value / 2)
            t = float(np.median(ts))
            print("%-8s algo=%d %s n=%-8d batch=%-8d ms median %8.3f min %8.3f max %8.3f  %7.1f Gpoint/s  %5.2f TB/s" %
                  (label, algo, "fp32" if prec else "fp64", n, batch, t, min(ts), max(ts), n * batch / t / 1e6, 2.0 * nbytes / t / 1e9), flush=True)
            lib.fft_gpu_destroy_plan(plan)
            lib.fft_gpu_free(a)
            lib.fft_gpu_free(b)


if __name__ == "__main__":
    main()
