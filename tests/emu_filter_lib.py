"""ctypes loader for the CPU emulation of the overlap-save FIR filter plan (tests/emu/emu_filter.cpp): a library of its own, built
lazily under a file lock the way emu_lib.lib() builds its library.  Test infra only."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_lib as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fft-implementation-in-c_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(EMU_DIR, "libfft_emu_filter.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_filter.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _lib.emu_filter.restype = C.c_int
    return _lib


def filter(x_ptr, y_ptr, h, signal_len, n_signals, n, mode, x_pitch, y_pitch, prec, lds_budget=0, no_fusion=False, no_chain=False,
           x2_ptr=None, y2_ptr=None):
    """One plan, one execute of x into y (and a second, of x2 -- or x again -- into y2) on raw host pointers.  h: the complex taps in
    the plan's precision.  Returns (rc, info): rc 0, -1 the plan was refused, -2 the execute was; info as documented in emu_filter.cpp."""
    info = (C.c_int * 8)()
    h = np.ascontiguousarray(h)
    rc = lib().emu_filter(x_ptr, y_ptr, x2_ptr, y2_ptr, h.size, h.ctypes.data if h.size else None, signal_len, n_signals, n, mode, x_pitch, y_pitch,
                          prec, lds_budget, (1 if no_fusion else 0) | (2 if no_chain else 0), info)
    return rc, list(info)
