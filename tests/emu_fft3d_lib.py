"""ctypes loader for the CPU emulation of the 3D transform plan (tests/emu/emu_fft3d.cpp): a library of its own, built lazily under a
file lock the way emu_real2d_lib.lib() builds its library.  Test infra only."""
import ctypes as C
import os
import subprocess

import emu_lib as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fft-implementation-in-c_amd", "csrc")
_lib = None

INFO = ("fused", "n_passes", "launches", "tile_planes", "threads", "prefetch", "row_strips", "col_strips", "depth_route", "workspace")


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(EMU_DIR, "libfft_emu_fft3d.so")
        if E._needs_build(so):
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if E._needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_fft3d.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_fft3d.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _lib.emu_fft3d.restype = C.c_int
    return _lib


def fft3d(in_ptr, out_ptr, depth, rows, cols, n_volumes, inverse, prec, lds_budget=0, no_fusion=False, unprefetched=False):
    """One plan, one execute on raw host pointers.  Returns (rc, info): rc 0, -1 the plan was refused, -2 the execute was; info: a dict
    of the fields emu_fft3d.cpp documents.  unprefetched: let the plan take tiles of more than two strips per step."""
    info = (C.c_int * 12)()
    rc = lib().emu_fft3d(in_ptr, out_ptr, depth, rows, cols, n_volumes, 1 if inverse else 0, prec, lds_budget, (1 if no_fusion else 0) | (2 if unprefetched else 0), info)
    return rc, dict(zip(INFO, list(info)))
