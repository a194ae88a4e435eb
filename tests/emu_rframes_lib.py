"""ctypes loader for the CPU emulation of the frames plans on REAL signals (tests/emu/emu_rframes.cpp): a library of its own, built
lazily under a file lock the way emu_frames_lib.lib() builds its library.  Test infra only."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_lib as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fft-implementation-in-c_amd", "csrc")
_lib = None
_FRAMES_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(EMU_DIR, "libfft_emu_rframes.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_rframes.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        for f in (_lib.emu_rframes, _lib.emu_frames):
            f.argtypes = _FRAMES_ARGS
            f.restype = C.c_int
    return _lib


def _call(f, x_ptr, out_ptr, n, hop, signal_len, n_signals, signal_pitch, window, w_host, kind, prec, lds_budget, no_fusion, fs, out2_ptr):
    info = (C.c_int * 8)()
    w = None if w_host is None else np.ascontiguousarray(w_host)
    rc = f(x_ptr, out_ptr, out2_ptr, n, hop, signal_len, n_signals, signal_pitch, window, None if w is None else w.ctypes.data,
           kind, prec, lds_budget, 1 if no_fusion else 0, fs, info)
    return rc, list(info)


def rframes(x_ptr, out_ptr, n, hop, signal_len, n_signals, signal_pitch, window, w_host, kind, prec, lds_budget=0, no_fusion=False, fs=1.0,
            out2_ptr=None):
    """One REAL frames plan, one execute into out_ptr (and a second into out2_ptr) on raw host pointers; x_ptr: real samples,
    signal_pitch in reals.  Returns (rc, info): rc 0, -1 the plan was refused, -2 the execute was; info as documented in
    emu_rframes.cpp."""
    return _call(lib().emu_rframes, x_ptr, out_ptr, n, hop, signal_len, n_signals, signal_pitch, window, w_host, kind, prec, lds_budget,
                 no_fusion, fs, out2_ptr)


def cframes(x_ptr, out_ptr, n, hop, signal_len, n_signals, signal_pitch, window, w_host, kind, prec, lds_budget=0, no_fusion=False, fs=1.0,
            out2_ptr=None):
    """The COMPLEX frames plan (emu_frames.cpp's emu_frames) in the same library: what the real plan's rows are compared with."""
    return _call(lib().emu_frames, x_ptr, out_ptr, n, hop, signal_len, n_signals, signal_pitch, window, w_host, kind, prec, lds_budget,
                 no_fusion, fs, out2_ptr)
