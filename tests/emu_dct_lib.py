"""ctypes loader for the CPU emulation of the cosine / sine transform plans (tests/emu/emu_dct.cpp): a library of its own, built lazily
under a file lock the way emu_real2d_lib.lib() builds its library.  Test infra only."""
import ctypes as C
import os
import subprocess

import emu_lib as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fft-implementation-in-c_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(EMU_DIR, "libfft_emu_dct.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_dct.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_dct.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _lib.emu_dct.restype = C.c_int
        _lib.emu_dct2d.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(C.c_int)]
        _lib.emu_dct2d.restype = C.c_int
    return _lib


def dct(in_ptr, in_pitch, out_ptr, out_pitch, n, batch, type, norm, prec, no_fusion=False):
    """One plan, one execute on raw host pointers.  Returns (rc, fused): rc 0, -1 the plan was refused, -2 the execute was."""
    info = (C.c_int * 4)()
    rc = lib().emu_dct(in_ptr, in_pitch, out_ptr, out_pitch, n, batch, type, norm, prec, 1 if no_fusion else 0, info)
    return rc, info[0]


def dct2d(in_ptr, in_pitch, out_ptr, out_pitch, rows, cols, n_matrices, type, norm, prec, no_fusion=False):
    info = (C.c_int * 4)()
    rc = lib().emu_dct2d(in_ptr, in_pitch, out_ptr, out_pitch, rows, cols, n_matrices, type, norm, prec, 1 if no_fusion else 0, info)
    return rc, info[0]
