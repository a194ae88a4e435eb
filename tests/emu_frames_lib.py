"""ctypes loader for the CPU emulation of the plans on overlapping frames (tests/emu/emu_frames.cpp): a library of its own, built
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
        so = os.path.join(EMU_DIR, "libfft_emu_frames.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_frames.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]
        _lib.emu_frames.restype = C.c_int
        _lib.emu_fused.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_double, C.POINTER(C.c_int)]
        _lib.emu_fused.restype = C.c_int
    return _lib


def frames(x_ptr, out_ptr, n, hop, signal_len, n_signals, signal_pitch, window, w_host, kind, prec, lds_budget=0, no_fusion=False, fs=1.0,
           out2_ptr=None):
    """One plan, one execute into out_ptr (and a second into out2_ptr) on raw host pointers.  Returns (rc, info): rc 0, -1 the plan
    was refused, -2 the execute was; info as documented in emu_frames.cpp."""
    info = (C.c_int * 8)()
    w = None if w_host is None else np.ascontiguousarray(w_host)
    rc = lib().emu_frames(x_ptr, out_ptr, out2_ptr, n, hop, signal_len, n_signals, signal_pitch, window, None if w is None else w.ctypes.data,
                          kind, prec, lds_budget, 1 if no_fusion else 0, fs, info)
    return rc, list(info)


def psd(x, fs):
    """FUSED_PSD of the rows of x ([batch][n] complex) in the same library: the plan ladder case (i) compares Welch with."""
    x = np.ascontiguousarray(x)
    batch, n = x.shape
    prec = 1 if x.dtype == np.complex64 else 0
    out = np.full((batch, n // 2 + 1), np.nan, dtype=np.float32 if prec else np.float64)
    info = (C.c_int * 8)()
    if lib().emu_fused(4, x.ctypes.data, None, None, n, 0, out.ctypes.data, batch, prec, 0, 0, fs, info) != 0:
        raise RuntimeError("emu_fused psd failed")
    return out
