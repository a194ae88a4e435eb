"""ctypes loader for the CPU emulation of the HIP kernels (tests/emu).  Test infra only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fft-implementation-in-c_amd", "csrc")
_lib = None


def _needs_build(so):
    if not os.path.exists(so):
        return True
    t = os.path.getmtime(so)
    srcs = [os.path.join(EMU_DIR, f) for f in os.listdir(EMU_DIR) if f.endswith((".cpp", ".h"))]
    srcs += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    return any(os.path.getmtime(s) > t for s in srcs)


def lib():
    global _lib
    if _lib is None:
        so = os.environ.get("FFT_EMU_SO", os.path.join(EMU_DIR, "libfft_emu.so"))  # FFT_EMU_SO: a sanitizer build
        if "FFT_EMU_SO" not in os.environ and _needs_build(so):
            # several processes may get here at once (the ranks of a gloo test): one builds, under a lock, into a temporary
            # file that is renamed into place; the others wait for the lock and find the library fresh
            import fcntl
            with open(so + ".lock", "w") as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                if _needs_build(so):
                    tmp = "%s.%d.tmp" % (so, os.getpid())
                    subprocess.run(["g++", "-O1", "-std=c++17", "-DFFT_EMU", "-DFFT_EXPERIMENTS", "-fPIC", "-shared", "-pthread", "-I" + CSRC,
                                    os.path.join(EMU_DIR, "emu_fft.cpp"), "-o", tmp], check=True)
                    os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_fft.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_int)]
        _lib.emu_fft.restype = C.c_int
        _lib.emu_fft_team.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_int)]
        _lib.emu_fft_team.restype = C.c_int
        _lib.emu_bitrev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    return _lib


def emu_fft(x, direction=-1, algo=0, lds_budget=0, inplace=False):
    """x: [batch, n] complex64/complex128.  Returns (result, info)."""
    x = np.ascontiguousarray(x)
    prec = 1 if x.dtype == np.complex64 else 0
    batch, n = x.shape
    info = (C.c_int * 8)()
    if inplace:
        out = x.copy()
        rc = lib().emu_fft(out.ctypes.data, out.ctypes.data, n, batch, direction, prec, algo, lds_budget, info)
    else:
        out = np.full_like(x, np.nan)
        rc = lib().emu_fft(x.ctypes.data, out.ctypes.data, n, batch, direction, prec, algo, lds_budget, info)
    if rc != 0:
        raise RuntimeError("emu_fft failed")
    return out, list(info)


def emu_fft_team(x, direction=-1, log2seats=2, n_xcc=2, threads=16, lds_budget=0, inplace=False, skew=False, tiles=4):
    """The team kernel (fft_team.h) with a small geometry: n_xcc "XCDs" of 2^log2seats workgroups of `threads` threads,
    all running concurrently.  The planner cuts each "XCD" into teams of n / (tiles * tile elements) workgroups
    (tiles = 4 as on the device; 1 or 2 force the few-tiles variants of the kernel).  info[0] = 100*tiles + passes
    when the team kernel was planned.  skew=True makes workgroup 0 report the wrong XCD: the kernel must give up and
    the two-pass fallback run."""
    os.environ["FFT_HIP_TEAM"] = "2"  # every size, any batch (the default only plans it where it measured faster)
    os.environ["FFT_HIP_TEAM_TILES"] = str(tiles)
    x = np.ascontiguousarray(x)
    prec = 1 if x.dtype == np.complex64 else 0
    batch, n = x.shape
    info = (C.c_int * 8)()
    mode = (log2seats + 1) | (n_xcc << 4) | (threads << 8) | ((1 << 20) if skew else 0)
    if inplace:
        out = x.copy()
        rc = lib().emu_fft_team(out.ctypes.data, out.ctypes.data, n, batch, direction, prec, lds_budget, mode, info)
    else:
        out = np.full_like(x, np.nan)
        rc = lib().emu_fft_team(x.ctypes.data, out.ctypes.data, n, batch, direction, prec, lds_budget, mode, info)
    if rc != 0:
        raise RuntimeError("emu_fft_team failed")
    return out, list(info)


SENTINEL = np.uint32(0x7F8A5A5A)  # the NaN payload of accuracy.SENTINEL: no kernel writes it


class GuardedArray:
    """[rows][width] values of dtype between two guards of SENTINEL words, in one numpy allocation.  `inner` is the view the
    emulation gets a pointer to: a write before its first or past its last element lands in a guard, not in the heap.  Each guard
    is the smallest multiple of 16 bytes >= one row and the allocation is 16-byte aligned, so `inner` starts where a plain
    allocation would put it (the kernels' 16-byte accesses rely on that), whatever the row size; the trailing guard starts right
    behind the last value."""

    def __init__(self, rows, width, dtype, fill=np.nan):
        dt = np.dtype(dtype)
        words = rows * width * dt.itemsize // 4
        self.gw = -(-(width * dt.itemsize) // 16) * 4  # guard words
        store = np.empty(words + 2 * self.gw + 4, dtype=np.uint32)
        off = ((-store.ctypes.data) % 16) // 4
        self.raw = store[off:off + words + 2 * self.gw]
        self.raw[...] = SENTINEL
        self.inner = self.raw[self.gw:self.gw + words].view(dt).reshape(rows, width)
        assert self.inner.ctypes.data % 16 == 0
        if fill is not None:
            self.inner[...] = fill

    def intact(self):
        return bool(np.all(self.raw[:self.gw] == SENTINEL) and np.all(self.raw[-self.gw:] == SENTINEL))


def _output(rows, width, dtype, guard):
    """(array the emulation writes, the GuardedArray around it or None)"""
    if guard:
        g = GuardedArray(rows, width, dtype)
        return g.inner, g
    return np.full((rows, width), np.nan, dtype=dtype), None


def _after(g, what, inputs):
    """Guarded variants: both guard rows intact, every input array unchanged."""
    if g is None:
        return
    assert g.intact(), "%s wrote outside its output" % what
    for a, copy in inputs:
        assert a is None or np.array_equal(a.view(np.uint8), copy.view(np.uint8)), "%s changed an input" % what


def emu_fft2d(x, direction=-1, lds_budget=0, inplace=False, guard=False):
    """x: [matrices, rows, cols] (or [rows, cols]) complex.  Returns (result, info); info[0] = 1 direct column pass, 2 transpose
    path, 3 two strided passes, 0 rows only.  guard=True: the output (in place: the buffer) sits between two sentinel rows that
    must be intact afterwards, and the input of an out-of-place run must be unchanged."""
    x = np.ascontiguousarray(x)
    x3 = x.reshape((-1,) + x.shape[-2:])
    nm, rows, cols = x3.shape
    prec = 1 if x.dtype == np.complex64 else 0
    info = (C.c_int * 8)()
    out, g = _output(nm, rows * cols, x.dtype, guard)
    if inplace:
        out[...] = x3.reshape(nm, -1)
    src = out if inplace else x3
    keep = x3.copy() if guard else None
    lib().emu_fft2d.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_int)]
    if lib().emu_fft2d(src.ctypes.data, out.ctypes.data, rows, cols, nm, direction, prec, lds_budget, info) != 0:
        raise RuntimeError("emu_fft2d failed")
    _after(g, "emu_fft2d", [(x3, keep)])
    return out.reshape(x.shape), list(info)


def _emu_real(src, out, n, batch, r2c, prec):
    lib().emu_real.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4
    if lib().emu_real(src.ctypes.data, out.ctypes.data, n, batch, r2c, prec) != 0:
        raise RuntimeError("emu_real failed")


def emu_r2c(x, guard=False, inplace=False):
    """x: [batch, n] float32/float64 -> [batch, n//2 + 1] complex.  inplace: through one buffer of batch * (n//2 + 1) complex
    values that holds the packed real rows at its start."""
    x = np.ascontiguousarray(x)
    batch, n = x.shape
    prec = 1 if x.dtype == np.float32 else 0
    out, g = _output(batch, n // 2 + 1, np.complex64 if prec else np.complex128, guard)
    keep = x.copy() if guard else None
    if inplace:
        out.reshape(-1).view(x.dtype)[:batch * n] = x.reshape(-1)
    _emu_real(out if inplace else x, out, n, batch, 1, prec)
    _after(g, "emu_r2c", [(x, keep)])
    return out


def emu_c2r(X, n, guard=False, inplace=False):
    """X: [batch, n//2 + 1] complex -> [batch, n] real (scaled by 1/n).  inplace: the real rows land packed at the start of a
    buffer that held X."""
    X = np.ascontiguousarray(X)
    batch = X.shape[0]
    prec = 1 if X.dtype == np.complex64 else 0
    rdt = np.float32 if prec else np.float64
    keep = X.copy() if guard else None
    if inplace:
        buf, g = _output(batch, n // 2 + 1, X.dtype, guard)
        buf[...] = X
        _emu_real(buf, buf, n, batch, 0, prec)
        _after(g, "emu_c2r in place", [])
        return buf.reshape(-1).view(rdt)[:batch * n].reshape(batch, n).copy()
    out, g = _output(batch, n, rdt, guard)
    _emu_real(X, out, n, batch, 0, prec)
    _after(g, "emu_c2r", [(X, keep)])
    return out


FUSED = {"conv": 0, "circ": 1, "autocorr": 2, "xcorr": 3, "psd": 4}


def emu_fused(kind, x, y=None, h=None, lds_budget=0, no_fusion=False, fs=1.0, guard=False):
    """x: [batch, nx] complex; h: [nh] kernel (conv / circ); y: [batch, nx] (xcorr).  Returns (result, info);
    info = [passes, fused?, log2 m, launch group].  guard=True: see emu_fft2d."""
    x = np.ascontiguousarray(x)
    batch, nx = x.shape
    prec = 1 if x.dtype == np.complex64 else 0
    k = FUSED[kind]
    nh = 0 if h is None else len(h)
    if h is not None:
        h = np.ascontiguousarray(h.astype(x.dtype))
    if y is not None:
        y = np.ascontiguousarray(y.astype(x.dtype))
    if kind == "conv":
        out, g = _output(batch, nx + nh - 1, x.dtype, guard)
    elif kind == "psd":
        out, g = _output(batch, nx // 2 + 1, np.float32 if prec else np.float64, guard)
    else:
        out, g = _output(batch, nx, x.dtype, guard)
    keep = [(a, a.copy()) for a in (x, y, h) if a is not None] if guard else []
    info = (C.c_int * 8)()
    f = lib().emu_fused
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                  C.POINTER(C.c_int)]
    rc = f(k, x.ctypes.data, None if y is None else y.ctypes.data, None if h is None else h.ctypes.data, nx, nh, out.ctypes.data, batch, prec,
           lds_budget, 1 if no_fusion else 0, fs, info)
    if rc != 0:
        raise RuntimeError("emu_fused failed")
    _after(g, "emu_fused " + kind, keep)
    return out, list(info)


def emu_fft2d_guarded(*a, **k):
    return emu_fft2d(*a, guard=True, **k)


def emu_r2c_guarded(*a, **k):
    return emu_r2c(*a, guard=True, **k)


def emu_c2r_guarded(*a, **k):
    return emu_c2r(*a, guard=True, **k)


def emu_fused_guarded(*a, **k):
    return emu_fused(*a, guard=True, **k)
