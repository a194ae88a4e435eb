"""What the plan handle answers for one small plan of every kind, built through the C API and never executed: every field of
fft_gpu_plan_info_hip, every getter (the ones of other kinds answer -1), the return code of every plan option, the path after
FFT_GPU_OPT_NO_FUSION / FFT_GPU_OPT_NO_CHAIN, the team status before any execute, and the refusal of fft_gpu_execute_ptr_hip by the
kinds that have an execute entry point of their own.

    python tools/plan_handle_table.py > tests/golden/plan_handle_table.json

The two large 1D plans are there for a team kernel in the plan (built, never launched): n = 2^20 has one in fp32 (team_kernel = 3)
and none in fp64, n = 2^19 has one in both (fp64: team_kernel = 2).

tests/test_gpu_plan_handle.py builds the same table and compares it with that file, field by field: a change of the handle's
dispatch that loses a plan kind somewhere shows there."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fft-implementation-in-c_amd"))

import fftlib  # noqa: E402

GETTERS = ("fused_out_len", "frames_count", "iframes_len", "iframes_unrecoverable", "cross_chunk", "filter_out_len", "filter_block",
           "conv2d_out_rows", "conv2d_out_cols", "conv2d_padded_rows", "conv2d_padded_cols", "real2d_bins")
# option -> the value set for the recorded return code (the ones that switch something off: the plan info after them is recorded too)
OPTIONS = (("no_fusion", fftlib.OPT_NO_FUSION, 1), ("no_chain", fftlib.OPT_NO_CHAIN, 1), ("team_force_fallback", fftlib.OPT_TEAM_FORCE_FALLBACK, 1),
           ("team_no_replay", fftlib.OPT_TEAM_NO_REPLAY, 1), ("team_enable", fftlib.OPT_TEAM_ENABLE, 0))
FWD = fftlib.FFT_FORWARD


def plans(lib, prec):
    """(name, refuses fft_gpu_execute_ptr_hip, constructor) of every plan of the table, in the element type of `prec`"""
    cdt = np.complex64 if prec == fftlib.PREC_F32 else np.complex128
    keep = []  # the host arrays live until the constructors have run

    def host(count, dt):
        a = ((np.arange(count) % 7) - 3).astype(dt)
        keep.append(a)
        return a.ctypes.data

    out = []
    for name, n, batch, algo in (("1d n=8 batch=2 auto", 8, 2, fftlib.ALGO_AUTO), ("1d n=8 bluestein", 8, 1, fftlib.ALGO_BLUESTEIN),
                                 ("1d n=11", 11, 1, fftlib.ALGO_AUTO), ("1d n=12 mixed_radix", 12, 1, fftlib.ALGO_MIXED_RADIX),
                                 ("1d n=2^19", 1 << 19, 1, fftlib.ALGO_AUTO), ("1d n=2^20", 1 << 20, 1, fftlib.ALGO_AUTO)):
        out.append((name, False, lambda n=n, batch=batch, algo=algo: lib.fft_gpu_plan_1d_ex_hip(n, batch, FWD, prec, algo)))
    for name, rows, cols, algo in (("2d 8x16", 8, 16, fftlib.ALGO_AUTO), ("2d 6x10", 6, 10, fftlib.ALGO_AUTO),
                                   ("2d 12x20 mixed_radix", 12, 20, fftlib.ALGO_MIXED_RADIX), ("2d 1x8", 1, 8, fftlib.ALGO_AUTO)):
        out.append((name, False, lambda rows=rows, cols=cols, algo=algo: lib.fft_gpu_plan_2d_algo_hip(rows, cols, 1, FWD, prec, algo)))
    for n in (16, 15):
        out.append(("r2c n=%d" % n, False, lambda n=n: lib.fft_gpu_plan_r2c_1d_hip(n, 1, prec)))
        out.append(("c2r n=%d" % n, False, lambda n=n: lib.fft_gpu_plan_c2r_1d_hip(n, 1, prec)))
    for kind, k in sorted(fftlib.FUSED_KINDS.items(), key=lambda kv: kv[1]):
        out.append(("fused %s nx=16 nh=3" % kind, True, lambda k=k: lib.fft_gpu_plan_fused_hip(k, 16, 3, host(3, cdt), 1, prec)))
    for real in (False, True):
        for o, ov in sorted(fftlib.FRAMES_OUT.items(), key=lambda kv: kv[1]):
            make = lib.fft_gpu_plan_frames_real_hip if real else lib.fft_gpu_plan_frames_hip
            out.append(("frames %s %s" % ("real" if real else "complex", o), True,
                        lambda make=make, ov=ov: make(16, 8, 64, 2, fftlib.WINDOWS["hann"], None, ov, prec)))
    out.append(("iframes", True, lambda: lib.fft_gpu_plan_iframes_real_hip(16, 8, 7, 2, fftlib.WINDOWS["hann"], None, prec)))
    for real in (False, True):
        for o, ov in sorted(fftlib.CROSS_OUT.items(), key=lambda kv: kv[1]):
            make = lib.fft_gpu_plan_cross_frames_real_hip if real else lib.fft_gpu_plan_cross_frames_hip
            out.append(("cross %s %s" % ("real" if real else "complex", o), True,
                        lambda make=make, ov=ov: make(16, 8, 64, 2, fftlib.WINDOWS["hann"], None, ov, prec)))
    for n in (0, 32):
        out.append(("filter taps=5 n=%d" % n, True, lambda n=n: lib.fft_gpu_plan_filter_hip(5, host(5, cdt), 100, 2, n, fftlib.FILTER_OUT["full"], prec)))
    for mode, mv in sorted(fftlib.CONV2D_MODES.items(), key=lambda kv: kv[1]):
        k = 8 if mode == "spectrum" else 3
        out.append(("conv2d %s" % mode, True, lambda k=k, mv=mv: lib.fft_gpu_plan_conv2d_hip(8, 8, k, k, host(k * k, cdt), 1, mv, prec)))
    for rows, cols in ((8, 16), (6, 10)):
        out.append(("rfft2 %dx%d" % (rows, cols), True, lambda rows=rows, cols=cols: lib.fft_gpu_plan_r2c_2d_hip(rows, cols, 1, prec)))
        out.append(("irfft2 %dx%d" % (rows, cols), True, lambda rows=rows, cols=cols: lib.fft_gpu_plan_c2r_2d_hip(rows, cols, 1, prec)))
    return out


def info_of(lib, handle):
    pi = fftlib.PlanInfo()
    rc = lib.fft_gpu_plan_info_hip(handle, C.byref(pi))
    d = {name: (list(getattr(pi, name)) if name == "factors" else int(getattr(pi, name))) for name, _ in fftlib.PlanInfo._fields_}
    d["rc"] = rc
    return d


def streams_created(lib):
    allocs, streams = C.c_longlong(), C.c_longlong()
    lib.fft_gpu_debug_counters_hip(C.byref(allocs), C.byref(streams))
    return streams.value


def record(lib, handle, refuses, d_a, d_b):
    row = {"info": info_of(lib, handle)}
    row["getters"] = {g: getattr(lib, "fft_gpu_%s_hip" % g)(handle) for g in GETTERS}
    row["team_status"] = lib.fft_gpu_plan_team_status_hip(handle)
    if refuses:
        row["execute_ptr"] = lib.fft_gpu_execute_ptr_hip(handle, d_a, d_b)
    row["options"] = {}
    for name, opt, value in OPTIONS:
        row["options"][name] = lib.fft_gpu_plan_set_option_hip(handle, opt, value)
        after = info_of(lib, handle)
        if name in ("no_fusion", "no_chain"):
            row["after_" + name] = {"fused": after["fused"], "n_passes": after["n_passes"]}
            lib.fft_gpu_plan_set_option_hip(handle, opt, 0)
        if name == "team_enable":
            row["after_team_enable_0"] = {"team_kernel": after["team_kernel"], "team_tiles": after["team_tiles"]}
    return row


def build_table():
    lib = fftlib.init()
    fftlib.set_policy(team=1, min_batch=0, chunk_mb=0)
    smooth = fftlib.set_smooth_policy(-1)
    fftlib.set_smooth_policy(0)
    a, b = fftlib.DeviceBuffer(4096), fftlib.DeviceBuffer(4096)
    table = {"plans": {}}
    streams0 = streams_created(lib)
    try:
        for pname, prec in (("fp32", fftlib.PREC_F32), ("fp64", fftlib.PREC_F64)):
            for name, refuses, make in plans(lib, prec):
                handle = make()
                if not handle:
                    raise RuntimeError("could not build the plan '%s' (%s)" % (name, pname))
                try:
                    table["plans"]["%s %s" % (pname, name)] = record(lib, handle, refuses, a.ptr, b.ptr)
                finally:
                    lib.fft_gpu_destroy_plan_hip(handle)
    finally:
        fftlib.set_smooth_policy(smooth)
        a.free()
        b.free()
    table["streams_created"] = streams_created(lib) - streams0
    return table


if __name__ == "__main__":
    json.dump(build_table(), sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")
