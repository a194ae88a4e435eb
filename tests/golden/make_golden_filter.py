#!/usr/bin/env python3
"""Golden vectors for the FIR design front end from the REAL reference's design_fir_filter (applications/fft_filtering.c:135-161),
compiled into a temporary directory OUTSIDE the repository (its main() renamed) and called through ctypes.  Build container only.
The output, tests/golden/reference_filter_vectors.npz, is DATA: the parameter sets and the taps the reference computed for them.

    python tests/golden/make_golden_filter.py <path of the reference tree>
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    sys.exit(__doc__)
REF = sys.argv[1]

# (taps, type, cutoff_low, cutoff_high, sample_rate, transition_width); type: the reference's filter_type_t
SETS = [(31, 0, 1000.0, 0.0, 8000.0, 0.0), (31, 0, 1000.0, 0.0, 8000.0, 400.0), (64, 0, 2000.0, 0.0, 48000.0, 1500.0),
        (31, 1, 0.0, 2500.0, 8000.0, 0.0), (64, 1, 0.0, 6000.0, 48000.0, 2000.0), (31, 2, 800.0, 2400.0, 8000.0, 0.0),
        (64, 2, 3000.0, 9000.0, 48000.0, 0.0), (64, 3, 3000.0, 9000.0, 48000.0, 0.0)]


class Params(C.Structure):
    _fields_ = [("type", C.c_int), ("cutoff_low", C.c_double), ("cutoff_high", C.c_double), ("sample_rate", C.c_double),
                ("transition_width", C.c_double)]


def main():
    out = {"sets": np.array(SETS, dtype=np.float64)}
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "libref_filter.so")
        subprocess.run(["gcc", "-w", "-O2", "-std=gnu99", "-fPIC", "-shared", "-Dmain=fft_filtering_demo_main", "-DLIB_BUILD", "-I" + os.path.join(REF, "include"),
                        os.path.join(REF, "applications", "fft_filtering.c"), os.path.join(REF, "algorithms", "core", "radix2_dit.c"), "-o", so, "-lm"],
                       check=True)
        lib = C.CDLL(so)
        lib.design_fir_filter.argtypes = [C.c_int, C.POINTER(Params)]
        lib.design_fir_filter.restype = C.POINTER(C.c_double)
        for i, (taps, kind, lo, hi, fs, tw) in enumerate(SETS):
            p = Params(kind, lo, hi, fs, tw)
            h = lib.design_fir_filter(taps, C.byref(p))
            out["taps_%d" % i] = np.array([h[2 * k] + 1j * h[2 * k + 1] for k in range(taps)], dtype=np.complex128)
    np.savez(os.path.join(HERE, "reference_filter_vectors.npz"), **out)
    print("wrote", len(SETS), "tap sets")


if __name__ == "__main__":
    main()
