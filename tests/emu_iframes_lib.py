"""ctypes loader for the CPU emulation of the inverse STFT plan (tests/emu/emu_iframes.cpp): a library of its own, built lazily
under a file lock the way emu_rframes_lib.lib() builds its library.  Test infra only."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_lib as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fft-implementation-in-c_amd", "csrc")
_lib = None
_IFRAMES_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                 C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
_FRAMES_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(EMU_DIR, "libfft_emu_iframes.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_iframes.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_iframes.argtypes = _IFRAMES_ARGS
        _lib.emu_iframes.restype = C.c_int
        _lib.emu_rframes.argtypes = _FRAMES_ARGS
        _lib.emu_rframes.restype = C.c_int
    return _lib


def iframes(X_ptr, y_ptr, n, hop, n_frames, n_signals, signal_pitch, window, w_host, prec, lds_budget=0, no_fusion=False, y2_ptr=None):
    """One inverse frames plan, one execute into y_ptr (and a second into y2_ptr) on raw host pointers.  Returns (rc, info): rc 0,
    -1 the plan was refused, -2 the execute was; info as documented in emu_iframes.cpp."""
    info = (C.c_int * 8)()
    w = None if w_host is None else np.ascontiguousarray(w_host)
    rc = lib().emu_iframes(X_ptr, y_ptr, y2_ptr, n, hop, n_frames, n_signals, signal_pitch, window, None if w is None else w.ctypes.data,
                           prec, lds_budget, 1 if no_fusion else 0, info)
    return rc, list(info)


def rstft(x_ptr, out_ptr, n, hop, signal_len, n_signals, window, w_host, prec):
    """The STFT of the REAL frames plan (emu_rframes.cpp's emu_rframes) in the same library: the forward leg of the round trip."""
    info = (C.c_int * 8)()
    w = None if w_host is None else np.ascontiguousarray(w_host)
    return lib().emu_rframes(x_ptr, out_ptr, None, n, hop, signal_len, n_signals, signal_len, window, None if w is None else w.ctypes.data,
                             0, prec, 0, 0, 1.0, info)
