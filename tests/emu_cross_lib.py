"""ctypes loader for the CPU emulation of the cross frames plan (tests/emu/emu_cross.cpp): a library of its own, built lazily under a
file lock the way emu_iframes_lib.lib() builds its library.  Test infra only."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_lib as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fft-implementation-in-c_amd", "csrc")
_lib = None
_CROSS_ARGS = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
               C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_longlong)]
_FRAMES_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]
INFO = ("passes", "fused", "nw", "launches", "C", "chunks", "part_bytes", "rows_bytes")


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(EMU_DIR, "libfft_emu_cross.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_cross.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_cross.argtypes = _CROSS_ARGS
        _lib.emu_cross.restype = C.c_int
        _lib.emu_cross_chunk_len.argtypes = [C.c_int, C.c_int, C.c_int]
        _lib.emu_cross_chunk_len.restype = C.c_int
        for f in (_lib.emu_rframes, _lib.emu_frames):
            f.argtypes = _FRAMES_ARGS
            f.restype = C.c_int
    return _lib


def cross(x_ptr, x_pitch, y_ptr, y_pitch, out_ptr, n, hop, signal_len, n_signals, window, w_host, kind, real_input, prec, lds_budget=0,
          no_fusion=False, max_grid=0, block=0, fs=1.0, out2_ptr=None):
    """One cross frames plan, one execute into out_ptr (and a second into out2_ptr) on raw host pointers.  Returns (rc, info): rc 0,
    -1 the plan was refused, -2 the execute was; info: a dict of INFO, as documented in emu_cross.cpp."""
    info = (C.c_longlong * 8)()
    w = None if w_host is None else np.ascontiguousarray(w_host)
    rc = lib().emu_cross(x_ptr, x_pitch, y_ptr, y_pitch, out_ptr, out2_ptr, n, hop, signal_len, n_signals, window, None if w is None else w.ctypes.data,
                         kind, 1 if real_input else 0, prec, lds_budget, 1 if no_fusion else 0, max_grid, block, fs, info)
    return rc, dict(zip(INFO, (int(v) for v in info)))


def chunk_len(nw, n_signals, hb):
    """The plan-time chunk rule alone."""
    return lib().emu_cross_chunk_len(nw, n_signals, hb)


def welch(x_ptr, out_ptr, n, hop, signal_len, n_signals, signal_pitch, window, w_host, real_input, prec, fs):
    """The WELCH rows of the (real or complex) frames plan in the same library: what the cross plan's Pxx is compared with."""
    info = (C.c_int * 8)()
    w = None if w_host is None else np.ascontiguousarray(w_host)
    f = lib().emu_rframes if real_input else lib().emu_frames
    return f(x_ptr, out_ptr, None, n, hop, signal_len, n_signals, signal_pitch, window, None if w is None else w.ctypes.data, 2, prec, 0, 0, fs, info)
