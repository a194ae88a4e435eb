"""ctypes loader for the CPU emulation of the 2D convolution plan (tests/emu/emu_conv2d.cpp): a library of its own, built lazily under
a file lock the way emu_filter_lib.lib() builds its library.  Test infra only."""
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
        so = os.path.join(EMU_DIR, "libfft_emu_conv2d.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_conv2d.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_conv2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _lib.emu_conv2d.restype = C.c_int
        _lib.emu_colround.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _lib.emu_colround.restype = C.c_int
    return _lib


def conv2d(x_ptr, y_ptr, k, rows, cols, n_matrices, mode, x_pitch, y_pitch, prec, lds_budget=0, no_fusion=False, min_seg=0, x2_ptr=None, y2_ptr=None):
    """One plan, one execute of x into y (and a second, of x2 -- or x again -- into y2) on raw host pointers.  k: the [krows, kcols]
    kernel (SPECTRUM: H) in the plan's precision.  Returns (rc, info): rc 0, -1 the plan was refused, -2 the execute was; info as
    documented in emu_conv2d.cpp (info[0]: which path ran)."""
    info = (C.c_int * 8)()
    k = np.ascontiguousarray(k)
    kr, kc = (k.shape if k.ndim == 2 else (0, 0))
    rc = lib().emu_conv2d(x_ptr, y_ptr, x2_ptr, y2_ptr, rows, cols, kr, kc, k.ctypes.data if k.size else None, n_matrices, mode, x_pitch, y_pitch, prec,
                          lds_budget, 1 if no_fusion else 0, min_seg, info)
    return rc, list(info)


def colround(x, H, rows_out, prec, lds_budget=0):
    """The column round alone on numpy arrays: x [nm, rows_in, Q], H [P, Q] -> ([nm, rows_out, Q], columns per tile, tiles per matrix)."""
    x, H = np.ascontiguousarray(x), np.ascontiguousarray(H)
    nm, rows_in, Q = x.shape
    P = H.shape[0]
    out = np.full((nm, rows_out, Q), np.nan, dtype=x.dtype)
    info = (C.c_int * 4)()
    rc = lib().emu_colround(x.ctypes.data, H.ctypes.data, out.ctypes.data, int(np.log2(P)), Q, rows_in, rows_out, nm, prec, lds_budget, info)
    assert rc == 0, rc
    return out, info[0], info[1]
