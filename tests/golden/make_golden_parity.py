#!/usr/bin/env python3
"""SHA-256 digests (oracle_lib.digest) of the REAL reference's whole outputs where tests/golden/reference_vectors.npz keeps
only samples, so that the oracle's bit parity with the reference is checked on every host and also where oracle/_ref
cannot be built:
- tests/test_oracle.py::test_golden_large_sampled: the forward transforms of its inputs (a norm over the whole output, as
  reference_vectors.npz stores it, depends on the host's BLAS in the last bit; the output itself does not);
- tests/test_oracle.py::test_against_real_reference_when_present: every input and output, and in full the one output
  that test compares numerically.
Build container only (needs `make -C oracle ref`).  The outputs are DATA.

    python tests/golden/make_golden_parity.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402


def main():
    assert O.ref_available(), "build oracle/_ref first: make -C oracle ref"
    out = {}
    for n in (65536, 1 << 18):
        for name, x in (("tone", O.gen_two_tone(n, 3, 1)[0]), ("lcg", O.gen_lcg(n, 3, 1)[0])):
            out["n%d_%s_fwd" % (n, name)] = O.digest(O.ref_fft(x, -1, "dit"))

    rng = np.random.default_rng(3)  # the test's inputs, drawn in the test's order
    for n in (32, 2048, 1 << 16):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        out["in_%d" % n] = O.digest(x)
        for algo in ("dit", "dif", "radix4", "split_radix"):
            for d in (-1, 1):
                out["%s_%d_%+d" % (algo, n, d)] = O.digest(O.ref_fft(x, d, algo))
    for n in (9, 100, 641):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        out["in_%d" % n] = O.digest(x)
        for d in (-1, 1):
            out["bluestein_%d_%+d" % (n, d)] = O.digest(O.ref_fft(x, d, "bluestein"))
    x = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    out["in_7"] = O.digest(x)
    out["bluestein_7_-1"] = O.ref_fft(x, -1, "bluestein")  # wrong in the reference (bit_reverse bug at m = 16): kept whole

    dst = os.path.join(HERE, "reference_parity.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
