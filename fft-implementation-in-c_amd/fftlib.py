"""ctypes binding of the C-ABI product library (libfft_mi355x.so).

This is the same boundary a C caller links against (include/fft_gpu.h,
include/fft_auto.h, include/fft_hip.h).  There is no fallback of any kind: a
missing library raises, and every entry point fails (NULL / -1) without a GPU.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FFT_LIB_PATH") or os.path.join(HERE, "libfft_mi355x.so")  # FFT_LIB_PATH: tools A/B-ing two builds

FFT_FORWARD = -1
FFT_INVERSE = 1
FFT_GPU_AUTO = -1
FFT_GPU_HIP = 4
PREC_F64 = 0
PREC_F32 = 1
ALGO_AUTO, ALGO_RADIX2, ALGO_RADIX4, ALGO_SPLIT_RADIX, ALGO_RADIX2_GLOBAL, ALGO_BLUESTEIN, ALGO_RADIX2_SHFL, ALGO_MIXED_RADIX = range(8)
ALGO_NAMES = {"auto": 0, "radix2": 1, "radix4": 2, "split_radix": 3, "radix2_global": 4, "bluestein": 5, "radix2_shfl": 6, "mixed_radix": 7}
FFT_PREFER_GPU = 1 << 9
HIP_STREAM_LEGACY = 1  # hipStreamLegacy: the NULL / default stream named explicitly (fft_gpu_plan_set_stream: NULL = the plan's own)
DCT2, DCT3, DST2, DST3 = range(4)                          # fft_gpu_dct_t
DCT_NORM_NONE, DCT_NORM_INVERSE, DCT_NORM_ORTHO = range(3)  # fft_gpu_dct_norm_t


def _real_prec(dtype):
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("float32 or float64 expected")
    return PREC_F32 if dt == np.float32 else PREC_F64


class PlanInfo(C.Structure):
    _fields_ = [("n", C.c_int), ("batch", C.c_int), ("direction", C.c_int), ("precision", C.c_int),
                ("algo", C.c_int), ("device", C.c_int), ("bluestein_m", C.c_int), ("n_passes", C.c_int),
                ("factors", C.c_int * 4), ("chunk_batch", C.c_int), ("workspace_bytes", C.c_size_t),
                ("team_tiles", C.c_int), ("fused", C.c_int), ("team_kernel", C.c_int)]


# every symbol include/*.h declares, with its ctypes signature
_vp, _sz, _i = C.c_void_p, C.c_size_t, C.c_int
SIGNATURES = {
    # include/fft_gpu.h
    "fft_gpu_init": (_i, [_i]), "fft_gpu_cleanup": (None, []), "fft_gpu_available": (_i, []),
    "fft_gpu_get_backend": (_i, []), "fft_gpu_alloc": (_vp, [_sz]), "fft_gpu_free": (None, [_vp]),
    "fft_gpu_copy_h2d": (None, [_vp, _vp, _sz]), "fft_gpu_copy_d2h": (None, [_vp, _vp, _sz]),
    "fft_gpu_plan_1d": (_vp, [_i, _i, _i]), "fft_gpu_execute": (None, [_vp, _vp, _vp]),
    "fft_gpu_destroy_plan": (None, [_vp]), "fft_gpu_dft_1d": (_i, [_vp, _vp, _i, _i]),
    "fft_gpu_dft_1d_batch": (_i, [_vp, _vp, _i, _i, _i]), "fft_gpu_plan_2d": (_vp, [_i, _i, _i]),
    "fft_gpu_dft_2d": (_i, [_vp, _vp, _i, _i, _i]), "fft_gpu_dft_3d": (_i, [_vp, _vp, _i, _i, _i, _i]),
    "fft_gpu_plan_3d": (_vp, [_i, _i, _i, _i, _i, _i]), "fft_gpu_get_device_name": (C.c_char_p, []),
    "fft_gpu_get_memory_info": (None, [C.POINTER(_sz), C.POINTER(_sz)]), "fft_gpu_set_device": (_i, [_i]),
    # include/fft_hip.h part 1 (backend set)
    "fft_gpu_init_hip": (_i, []), "fft_gpu_cleanup_hip": (None, []), "fft_gpu_available_hip": (_i, []),
    "fft_gpu_alloc_hip": (_vp, [_sz]), "fft_gpu_free_hip": (None, [_vp]),
    "fft_gpu_copy_h2d_hip": (None, [_vp, _vp, _sz]), "fft_gpu_copy_d2h_hip": (None, [_vp, _vp, _sz]),
    "fft_gpu_plan_1d_hip": (_vp, [_i, _i, _i]), "fft_gpu_execute_hip": (None, [_vp, _vp, _vp, _i]),
    "fft_gpu_destroy_plan_hip": (None, [_vp]), "fft_gpu_get_device_name_hip": (C.c_char_p, []),
    "fft_gpu_get_memory_info_hip": (None, [C.POINTER(_sz), C.POINTER(_sz)]),
    "fft_gpu_dft_1d_hip": (_i, [_vp, _vp, _i, _i]),
    # include/fft_hip.h part 2 (additive, backend level)
    "fft_gpu_device_count_hip": (_i, []), "fft_gpu_set_device_hip": (_i, [_i]), "fft_gpu_get_device_hip": (_i, []),
    "fft_gpu_alloc_bytes_hip": (_vp, [_sz]), "fft_gpu_copy_h2d_bytes_hip": (_i, [_vp, _vp, _sz]),
    "fft_gpu_copy_d2h_bytes_hip": (_i, [_vp, _vp, _sz]), "fft_gpu_memory_ptr_hip": (_vp, [_vp]),
    "fft_gpu_memory_bytes_hip": (_sz, [_vp]), "fft_gpu_plan_1d_ex_hip": (_vp, [_i, _i, _i, _i, _i]),
    "fft_gpu_plan_info_hip": (_i, [_vp, C.POINTER(PlanInfo)]), "fft_gpu_plan_set_stream_hip": (_i, [_vp, _vp]),
    "fft_gpu_execute_ptr_hip": (_i, [_vp, _vp, _vp]), "fft_gpu_plan_sync_hip": (_i, [_vp]),
    "fft_gpu_plan_set_option_hip": (_i, [_vp, _i, _i]), "fft_gpu_set_policy_hip": (_i, [_i, _i, _i]),
    "fft_gpu_mixed_radix_passes_hip": (_i, [_i]), "fft_gpu_set_smooth_policy_hip": (_i, [_i]),
    "fft_gpu_plan_3d_hip": (_vp, [_i, _i, _i, _i, _i, _i]), "fft_gpu_plan_2d_hip": (_vp, [_i, _i, _i]), "fft_gpu_plan_2d_ex_hip": (_vp, [_i, _i, _i, _i, _i]),
    "fft_gpu_plan_r2c_1d_hip": (_vp, [_i, _i, _i]), "fft_gpu_plan_c2r_1d_hip": (_vp, [_i, _i, _i]),
    "fft_gpu_plan_2d_algo_hip": (_vp, [_i, _i, _i, _i, _i, _i]),
    "fft_gpu_plan_r2c_1d_algo_hip": (_vp, [_i, _i, _i, _i]), "fft_gpu_plan_c2r_1d_algo_hip": (_vp, [_i, _i, _i, _i]),
    "fft_gpu_plan_fused_hip": (_vp, [_i, _i, _i, _vp, _i, _i]), "fft_gpu_fused_out_len_hip": (_i, [_vp]),
    "fft_gpu_execute_fused_hip": (_i, [_vp, _vp, _vp, _vp, C.c_double]),
    "fft_gpu_plan_frames_hip": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]), "fft_gpu_frames_count_hip": (_i, [_vp]),
    "fft_gpu_plan_frames_real_hip": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]),
    "fft_gpu_execute_frames_hip": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_double]),
    "fft_gpu_plan_iframes_real_hip": (_vp, [_i, _i, _i, _i, _i, _vp, _i]), "fft_gpu_iframes_len_hip": (_i, [_vp]),
    "fft_gpu_iframes_unrecoverable_hip": (_i, [_vp]), "fft_gpu_execute_iframes_hip": (_i, [_vp, _vp, _vp, C.c_longlong]),
    "fft_gpu_plan_cross_frames_hip": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]),
    "fft_gpu_plan_cross_frames_real_hip": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]), "fft_gpu_cross_chunk_hip": (_i, [_vp]),
    "fft_gpu_execute_cross_frames_hip": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_double]),
    "fft_gpu_plan_filter_hip": (_vp, [_i, _vp, _i, _i, _i, _i, _i]), "fft_gpu_filter_out_len_hip": (_i, [_vp]),
    "fft_gpu_filter_block_hip": (_i, [_vp]), "fft_gpu_execute_filter_hip": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    "fft_gpu_plan_conv2d_hip": (_vp, [_i, _i, _i, _i, _vp, _i, _i, _i]), "fft_gpu_conv2d_out_rows_hip": (_i, [_vp]),
    "fft_gpu_conv2d_out_cols_hip": (_i, [_vp]), "fft_gpu_conv2d_padded_rows_hip": (_i, [_vp]), "fft_gpu_conv2d_padded_cols_hip": (_i, [_vp]),
    "fft_gpu_execute_conv2d_hip": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    "fft_gpu_plan_r2c_2d_hip": (_vp, [_i, _i, _i, _i]), "fft_gpu_plan_c2r_2d_hip": (_vp, [_i, _i, _i, _i]), "fft_gpu_real2d_bins_hip": (_i, [_vp]),
    "fft_gpu_execute_real2d_hip": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    "fft_gpu_plan_dct_hip": (_vp, [_i, _i, _i, _i, _i]), "fft_gpu_plan_dct_2d_hip": (_vp, [_i, _i, _i, _i, _i, _i]),
    "fft_gpu_execute_dct_hip": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    "fft_gpu_host_register_hip": (_i, [_vp, _sz]), "fft_gpu_host_unregister_hip": (_i, [_vp]),
    "fft_gpu_host_is_registered_hip": (_i, [_vp]), "fft_gpu_copy_bench_hip": (C.c_double, [_sz, _i]), "fft_gpu_stream_bench_hip": (C.c_double, [_sz, _i, _i]),
    "fft_gpu_debug_counters_hip": (None, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "fft_gpu_plan_measure_hip": (_i, [_vp, _i]),
    "fft_gpu_plan_team_status_hip": (_i, [_vp]), "fft_gpu_plan_team_trace_hip": (_i, [_vp, _vp, _i]),
    "fft_gpu_execute_timed_hip": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_float)]),
    "fft_gpu_dft_1d_batch_hip": (_i, [_vp, _vp, _i, _i, _i, _i]),
    "fft_gpu_profile_passes_hip": (_i, [_vp, _vp, _vp, C.POINTER(C.c_float), C.POINTER(C.c_int), _i]),
    "fft_gpu_bit_reverse_hip": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    # include/fft_hip.h part 2 (additive, public)
    "fft_gpu_device_count": (_i, []), "fft_gpu_alloc_f32": (_vp, [_sz]),
    "fft_gpu_copy_h2d_f32": (None, [_vp, _vp, _sz]), "fft_gpu_copy_d2h_f32": (None, [_vp, _vp, _sz]),
    "fft_gpu_memory_ptr": (_vp, [_vp]), "fft_gpu_plan_1d_f32": (_vp, [_i, _i, _i]),
    "fft_gpu_plan_1d_ex": (_vp, [_i, _i, _i, _i, _i]), "fft_gpu_plan_2d_algo": (_vp, [_i, _i, _i, _i, _i, _i]),
    "fft_gpu_plan_info": (_i, [_vp, C.POINTER(PlanInfo)]),
    "fft_gpu_plan_set_stream": (_i, [_vp, _vp]), "fft_gpu_execute_async": (_i, [_vp, _vp, _vp]),
    "fft_gpu_execute_ptr": (_i, [_vp, _vp, _vp]), "fft_gpu_plan_sync": (_i, [_vp]),
    "fft_gpu_execute_timed": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_float)]),
    "fft_gpu_dft_1d_f32": (_i, [_vp, _vp, _i, _i]), "fft_gpu_dft_1d_batch_f32": (_i, [_vp, _vp, _i, _i, _i]),
    "fft_gpu_bit_reverse": (_i, [_vp, _vp, _i, _i, _i]),
    "fft_gpu_plan_frames": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]), "fft_gpu_frames_count": (_i, [_vp]),
    "fft_gpu_plan_frames_real": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]),
    "fft_gpu_execute_frames": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_double]),
    "fft_gpu_plan_iframes_real": (_vp, [_i, _i, _i, _i, _i, _vp, _i]), "fft_gpu_iframes_len": (_i, [_vp]),
    "fft_gpu_iframes_unrecoverable": (_i, [_vp]), "fft_gpu_execute_iframes": (_i, [_vp, _vp, _vp, C.c_longlong]),
    "fft_gpu_plan_cross_frames": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]),
    "fft_gpu_plan_cross_frames_real": (_vp, [_i, _i, _i, _i, _i, _vp, _i, _i]), "fft_gpu_cross_chunk": (_i, [_vp]),
    "fft_gpu_execute_cross_frames": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_double]),
    # include/fft_gpu.h, behind its include of fft_hip.h
    "fft_gpu_plan_filter": (_vp, [_i, _vp, _i, _i, _i, _i, _i]), "fft_gpu_filter_out_len": (_i, [_vp]),
    "fft_gpu_filter_block": (_i, [_vp]), "fft_gpu_execute_filter": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    "fft_gpu_plan_conv2d": (_vp, [_i, _i, _i, _i, _vp, _i, _i, _i]), "fft_gpu_conv2d_out_rows": (_i, [_vp]),
    "fft_gpu_conv2d_out_cols": (_i, [_vp]), "fft_gpu_conv2d_padded_rows": (_i, [_vp]), "fft_gpu_conv2d_padded_cols": (_i, [_vp]),
    "fft_gpu_execute_conv2d": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    "fft_gpu_plan_r2c_2d": (_vp, [_i, _i, _i, _i]), "fft_gpu_plan_c2r_2d": (_vp, [_i, _i, _i, _i]), "fft_gpu_real2d_bins": (_i, [_vp]),
    "fft_gpu_execute_real2d": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    "fft_gpu_plan_dct": (_vp, [_i, _i, _i, _i, _i]), "fft_gpu_plan_dct_2d": (_vp, [_i, _i, _i, _i, _i, _i]),
    "fft_gpu_execute_dct": (_i, [_vp, _vp, C.c_longlong, _vp, C.c_longlong]),
    # include/fft_auto.h
    "fft_plan_dft_1d": (_vp, [_i, _vp, _vp, _i, C.c_uint]), "fft_execute": (None, [_vp]),
    "fft_execute_dft": (None, [_vp, _vp, _vp]), "fft_destroy_plan": (None, [_vp]),
    "fft_auto": (_i, [_vp, _vp, _i, _i]), "fft_plan_r2c_1d": (_vp, [_i, _vp, _vp, C.c_uint]),
    "fft_plan_c2r_1d": (_vp, [_i, _vp, _vp, C.c_uint]), "fft_plan_dft_2d": (_vp, [_i, _i, _vp, _vp, _i, C.c_uint]),
    "fft_export_wisdom_to_string": (_vp, []), "fft_import_wisdom_from_string": (_i, [C.c_char_p]),
    "fft_get_hardware_capabilities": (C.c_uint, []), "fft_plan_with_nthreads": (None, [_i]),
    "fft_alloc_complex": (_vp, [_sz]), "fft_alloc_real": (_vp, [_sz]), "fft_free": (None, [_vp]),
    "fft_version": (C.c_char_p, []), "fft_plan_measured_algo": (_i, [_vp]), "fft_plan_last_error": (_i, [_vp]), "fft_auto_cleanup": (None, []),
    # include/fft_apps.h, include/fft_utils.h
    "fft_convolution_gpu": (_i, [_vp, _i, _vp, _i, _vp]), "circular_convolution_gpu": (_i, [_vp, _vp, _i, _vp]),
    "compute_periodogram_gpu": (_vp, [_vp, _i, C.c_double]), "autocorrelation_fft_gpu": (_vp, [_vp, _i]),
    "cross_correlation_fft_gpu": (_vp, [_vp, _vp, _i]),
    "fft_welch_psd_gpu": (_vp, [_vp, _i, C.c_double, _i, _i]), "fft_welch_psd_real_gpu": (_vp, [_vp, _i, C.c_double, _i, _i]),
    "fft_coherence_real_gpu": (_vp, [_vp, _vp, _i, _i, _i]), "fft_csd_real_gpu": (_i, [_vp, _vp, _i, C.c_double, _i, _i, _vp]),
    "fft_fir_filter_gpu": (_i, [_vp, _i, _vp, _i, _vp]),
    "fft_design_fir_filter_gpu": (_vp, [_i, _i, C.c_double, C.c_double, C.c_double, C.c_double]),
    "fft_convolution_2d_gpu": (_i, [_vp, _i, _i, _vp, _i, _i, _vp]), "fft_filter_2d_gpu": (_i, [_vp, _i, _i, _vp, _vp]),
    "fft_rfft2_gpu": (_i, [_vp, _i, _i, _vp]), "fft_irfft2_gpu": (_i, [_vp, _i, _i, _vp]),
    "fft_dct_gpu": (_i, [_vp, _i, _i, _i, _vp]), "fft_dct_2d_gpu": (_i, [_vp, _i, _i, _i, _i, _vp]),
    "save_complex_array": (_i, [C.c_char_p, _vp, _i]), "load_complex_array": (_i, [C.c_char_p, C.POINTER(_vp), C.POINTER(_i)]),
    # include/fft_algorithms.h
    "radix2_dit_fft_gpu": (_i, [_vp, _i, _i]), "radix2_fft_gpu": (_i, [_vp, _i, _i]),
    "radix4_fft_gpu": (_i, [_vp, _i, _i]), "split_radix_fft_gpu": (_i, [_vp, _i, _i]),
    "bluestein_fft_gpu": (_i, [_vp, _i, _i]), "fft_mixed_radix_gpu": (_i, [_vp, _i, _i]),
}

# declared in include/fft_apps.h under the reference's own name, which none of the prefixes of SIGNATURES' names covers
EXTRA_SIGNATURES = {"compute_coherence_gpu": (_vp, [_vp, _vp, _i, _i])}

_lib = None


def load():
    """Load the product library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("HIP extension missing: %s (build it: make -C %s)" % (LIB_PATH, HERE))
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(EXTRA_SIGNATURES.items()):
            f = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = lib
    return _lib


def _prec_of(dtype):
    if dtype == np.complex64:
        return PREC_F32
    if dtype == np.complex128:
        return PREC_F64
    raise TypeError("complex64 or complex128 expected")


def init():
    lib = load()
    if lib.fft_gpu_init(FFT_GPU_AUTO) != 0:
        raise RuntimeError("fft_gpu_init failed: no usable MI355X/HIP device")
    return lib


EXP_LIB_PATH = os.path.join(HERE, "libfft_mi355x_exp.so")  # -DFFT_EXPERIMENTS build: kernel-variant switches, ablation bits
OPT_TEAM_FORCE_FALLBACK, OPT_TEAM_ENABLE, OPT_NO_FUSION, OPT_NO_CHAIN, OPT_TEAM_NO_REPLAY = 1, 2, 3, 4, 5


def set_device(index):
    """Make `index` the device new plans and buffers live on (fft_gpu_set_device; an 8-GPU process sets each in turn)."""
    if load().fft_gpu_set_device(int(index)) != 0:
        raise RuntimeError("fft_gpu_set_device(%d) failed" % index)


def get_device():
    """The device new plans and buffers currently live on (fft_gpu_get_device_hip)."""
    return load().fft_gpu_get_device_hip()


def set_smooth_policy(mode=-1):
    """Which plan ALGO_AUTO builds for 7-smooth lengths from now on: 0 chirp-z (default), 1 mixed radix; -1 only asks.  Returns the mode in force."""
    return load().fft_gpu_set_smooth_policy_hip(mode)


def mixed_radix_passes(n):
    """0: n is not a mixed-radix length; 1 / 2: passes of the mixed-radix plan (no device needed)."""
    return load().fft_gpu_mixed_radix_passes_hip(n)


def set_policy(team=-1, min_batch=-1, chunk_mb=-1):
    """Planner policy for plans created from now on (fft_gpu_set_policy_hip); -1 keeps a value."""
    load().fft_gpu_set_policy_hip(team, min_batch, chunk_mb)


class DeviceBuffer:
    """Device memory owned through fft_gpu_alloc_bytes_hip / fft_gpu_free."""

    def __init__(self, nbytes):
        self.lib = load()
        self.handle = self.lib.fft_gpu_alloc_bytes_hip(nbytes)
        if not self.handle:
            raise MemoryError("device allocation of %d bytes failed" % nbytes)
        self.nbytes = nbytes

    @property
    def ptr(self):
        return self.lib.fft_gpu_memory_ptr_hip(self.handle)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        if self.lib.fft_gpu_copy_h2d_bytes_hip(self.handle, arr.ctypes.data, arr.nbytes) != 0:
            raise RuntimeError("h2d failed")

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if self.lib.fft_gpu_copy_d2h_bytes_hip(out.ctypes.data, self.handle, out.nbytes) != 0:
            raise RuntimeError("d2h failed")
        return out

    def free(self):
        if self.handle:
            self.lib.fft_gpu_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Plan:
    def __init__(self, n, batch, direction=FFT_FORWARD, dtype=np.complex64, algo=ALGO_AUTO):
        self.lib = init()
        self.n, self.batch, self.direction, self.dtype = n, batch, direction, np.dtype(dtype)
        self.handle = self.lib.fft_gpu_plan_1d_ex(n, batch, direction, _prec_of(self.dtype), algo)
        if not self.handle:
            raise RuntimeError("fft_gpu_plan_1d_ex(n=%d, batch=%d) failed" % (n, batch))

    def info(self):
        pi = PlanInfo()
        self.lib.fft_gpu_plan_info(self.handle, C.byref(pi))
        return pi

    def execute(self, buf_in, buf_out=None):
        buf_out = buf_out or buf_in
        self.lib.fft_gpu_execute(self.handle, buf_in.handle, buf_out.handle)

    def execute_ptr(self, d_in, d_out):
        if self.lib.fft_gpu_execute_ptr(self.handle, d_in, d_out) != 0:
            raise RuntimeError("fft_gpu_execute_ptr failed")

    def sync(self):
        return self.lib.fft_gpu_plan_sync(self.handle)

    def set_option(self, option, value):
        if self.lib.fft_gpu_plan_set_option_hip(self.handle, option, value) != 0:
            raise RuntimeError("fft_gpu_plan_set_option_hip(%d) failed" % option)

    def team_status(self):
        """0 team kernel did the last execute, 1 its fallback did, 2 barrier timeout, -1 no team kernel / never launched."""
        return self.lib.fft_gpu_plan_team_status_hip(self.handle)

    def timed(self, d_in, d_out, iters):
        ms = C.c_float()
        if self.lib.fft_gpu_execute_timed(self.handle, d_in, d_out, iters, C.byref(ms)) != 0:
            raise RuntimeError("fft_gpu_execute_timed failed")
        return ms.value

    def profile_passes(self, d_in, d_out, max_passes=4):
        ms = (C.c_float * max_passes)()
        cnt = (C.c_int * max_passes)()
        if self.lib.fft_gpu_profile_passes_hip(self.handle, d_in, d_out, ms, cnt, max_passes) != 0:
            raise RuntimeError("fft_gpu_profile_passes_hip failed")
        return [(ms[i], cnt[i]) for i in range(max_passes) if cnt[i]]

    def set_stream(self, stream_ptr):
        self.lib.fft_gpu_plan_set_stream(self.handle, stream_ptr)

    def destroy(self):
        if self.handle:
            self.lib.fft_gpu_destroy_plan(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


FUSED_KINDS = {"conv": 0, "circ": 1, "autocorr": 2, "xcorr": 3, "psd": 4}
WINDOWS = {"rect": 0, "hann": 1, "hamming": 2, "blackman": 3, "user": 4}
FRAMES_OUT = {"stft": 0, "power": 1, "welch": 2}
CROSS_OUT = {"csd": 0, "coherence": 1, "transfer": 2, "all": 3}
FILTER_OUT = {"full": 0, "causal": 1, "same": 2}


class ExtPlan:
    """2D / r2c / c2r / fused plans (fft_hip.h): a thin owner of the handle; execute with raw device pointers."""

    def __init__(self, handle):
        self.lib = init()
        if not handle:
            raise RuntimeError("plan creation failed")
        self.handle = handle

    @classmethod
    def fft2d(cls, rows, cols, n_matrices=1, direction=FFT_FORWARD, dtype=np.complex128, algo=ALGO_AUTO):
        """algo (here and in r2c / c2r): ALGO_AUTO or ALGO_MIXED_RADIX (7-smooth lengths on the mixed-radix engine)."""
        return cls(init().fft_gpu_plan_2d_algo_hip(rows, cols, n_matrices, direction, _prec_of(np.dtype(dtype)), algo))

    @classmethod
    def plan3d(cls, depth, rows, cols, n_volumes=1, direction=FFT_FORWARD, dtype=np.complex128):
        """3D complex plan (fft_gpu_plan_3d_hip): n_volumes row-major [depth][rows][cols] volumes of dtype complex64 / complex128; execute
        and execute_ptr as a 2D plan's, in place allowed.  info(): fused = 1 where the plane kernel runs, n_passes = launches."""
        p = cls(init().fft_gpu_plan_3d_hip(depth, rows, cols, n_volumes, direction, _prec_of(np.dtype(dtype))))
        p.depth, p.rows, p.cols, p.n_volumes, p.dtype = depth, rows, cols, n_volumes, np.dtype(dtype)
        return p

    @classmethod
    def r2c(cls, n, batch=1, dtype=np.float64, algo=ALGO_AUTO):
        return cls(init().fft_gpu_plan_r2c_1d_algo_hip(n, batch, PREC_F32 if np.dtype(dtype) == np.float32 else PREC_F64, algo))

    @classmethod
    def c2r(cls, n, batch=1, dtype=np.float64, algo=ALGO_AUTO):
        return cls(init().fft_gpu_plan_c2r_1d_algo_hip(n, batch, PREC_F32 if np.dtype(dtype) == np.float32 else PREC_F64, algo))

    @classmethod
    def fused(cls, kind, nx, batch=1, h=None, dtype=np.complex128):
        dt = np.dtype(dtype)
        hh = None if h is None else np.ascontiguousarray(np.asarray(h).astype(dt))
        p = cls(init().fft_gpu_plan_fused_hip(FUSED_KINDS[kind], nx, 0 if hh is None else len(hh),
                                              None if hh is None else hh.ctypes.data, batch, _prec_of(dt)))
        p.out_len = p.lib.fft_gpu_fused_out_len_hip(p.handle)
        return p

    @classmethod
    def frames(cls, n, hop, signal_len, n_signals=1, window="hann", out="stft", dtype=np.complex128):
        """STFT / spectrogram ("power") / Welch plan on overlapping frames.  window: a name of WINDOWS, or n real values (USER).
        dtype float32 / float64: the plan for REAL signals (fft_gpu_plan_frames_real_hip), whose rows are one-sided."""
        dt = np.dtype(dtype)
        real = dt in (np.dtype(np.float32), np.dtype(np.float64))
        w = None
        if not isinstance(window, str):
            w = np.ascontiguousarray(np.asarray(window).astype(np.float32 if dt in (np.complex64, np.float32) else np.float64))
            if w.shape != (n,):
                raise ValueError("a user window has n values")
        lib = init()
        make = lib.fft_gpu_plan_frames_real_hip if real else lib.fft_gpu_plan_frames_hip
        prec = (PREC_F32 if dt == np.float32 else PREC_F64) if real else _prec_of(dt)
        p = cls(make(n, hop, signal_len, n_signals, WINDOWS["user" if w is not None else window],
                     None if w is None else w.ctypes.data, FRAMES_OUT[out], prec))
        p.n, p.n_signals, p.out, p.dtype, p.real = n, n_signals, out, dt, real
        p.nw = p.lib.fft_gpu_frames_count_hip(p.handle)
        return p

    def frames_out(self):
        """(shape, dtype) of a frames plan's result."""
        rdt = np.dtype(np.float32 if self.dtype in (np.complex64, np.float32) else np.float64)
        if self.out == "stft" and self.real:  # one-sided rows
            return (self.n_signals, self.nw, self.n // 2 + 1), np.dtype(np.complex64 if rdt == np.float32 else np.complex128)
        if self.out == "stft":
            return (self.n_signals, self.nw, self.n), self.dtype
        if self.out == "power":
            return (self.n_signals, self.nw, self.n // 2 + 1), rdt
        return (self.n_signals, self.n // 2 + 1), rdt

    @classmethod
    def iframes(cls, n, hop, n_frames, n_signals=1, window="hann", dtype=np.float64):
        """Inverse STFT plan (fft_gpu_plan_iframes_real_hip): [n_signals, n_frames, n//2 + 1] one-sided rows -> n_signals real signals
        of out_len = (n_frames - 1) * hop + n samples of dtype float32 / float64, by weighted overlap-add.  window: a name of WINDOWS,
        or n real values (USER).  unrecoverable: the samples per signal whose window envelope vanishes (written as 0)."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("an inverse frames plan writes float32 or float64 signals")
        w = None
        if not isinstance(window, str):
            w = np.ascontiguousarray(np.asarray(window).astype(dt))
            if w.shape != (n,):
                raise ValueError("a user window has n values")
        p = cls(init().fft_gpu_plan_iframes_real_hip(n, hop, n_frames, n_signals, WINDOWS["user" if w is not None else window],
                                                     None if w is None else w.ctypes.data, PREC_F32 if dt == np.float32 else PREC_F64))
        p.n, p.hop, p.nw, p.n_signals, p.dtype = n, hop, n_frames, n_signals, dt
        p.out_len = p.lib.fft_gpu_iframes_len_hip(p.handle)
        p.unrecoverable = p.lib.fft_gpu_iframes_unrecoverable_hip(p.handle)
        return p

    @classmethod
    def cross_frames(cls, n, hop, signal_len, n_signals=1, window="hann", out="csd", dtype=np.float64):
        """Cross-spectral density ("csd"), magnitude-squared coherence, H1 transfer estimate or all three spectra ("all") of n_signals
        PAIRS of signals on overlapping frames (fft_gpu_plan_cross_frames_real_hip for float32 / float64 signals,
        fft_gpu_plan_cross_frames_hip for complex64 / complex128).  window: a name of WINDOWS, or n real values (USER).
        chunk: the frames per chunk of the reduction."""
        dt = np.dtype(dtype)
        real = dt in (np.dtype(np.float32), np.dtype(np.float64))
        f32 = dt in (np.dtype(np.complex64), np.dtype(np.float32))
        w = None
        if not isinstance(window, str):
            w = np.ascontiguousarray(np.asarray(window).astype(np.float32 if f32 else np.float64))
            if w.shape != (n,):
                raise ValueError("a user window has n values")
        lib = init()
        make = lib.fft_gpu_plan_cross_frames_real_hip if real else lib.fft_gpu_plan_cross_frames_hip
        p = cls(make(n, hop, signal_len, n_signals, WINDOWS["user" if w is not None else window],
                     None if w is None else w.ctypes.data, CROSS_OUT[out], PREC_F32 if f32 else PREC_F64))
        p.n, p.n_signals, p.out, p.dtype, p.real = n, n_signals, out, dt, real
        p.nw = p.lib.fft_gpu_frames_count_hip(p.handle)
        p.chunk = p.lib.fft_gpu_cross_chunk_hip(p.handle)
        return p

    def cross_out(self):
        """(shape, dtype) of a cross frames plan's result."""
        f32 = self.dtype in (np.dtype(np.complex64), np.dtype(np.float32))
        hb = self.n // 2 + 1
        if self.out == "coherence":
            return (self.n_signals, hb), np.dtype(np.float32 if f32 else np.float64)
        if self.out == "all":
            return (self.n_signals, hb, 4), np.dtype(np.float32 if f32 else np.float64)
        return (self.n_signals, hb), np.dtype(np.complex64 if f32 else np.complex128)

    @classmethod
    def filter(cls, h, signal_len, n_signals=1, mode="full", n=0, dtype=np.complex128):
        """Overlap-save FIR filter plan (fft_gpu_plan_filter_hip): n_signals complex signals of signal_len samples, the taps h, the
        output of FILTER_OUT[mode] ("full": signal_len + len(h) - 1 samples, np.convolve; "causal": signal_len, lfilter(h, 1, x);
        "same": signal_len, np.convolve 'same').  n: the block length, a power of two > len(h) - 1; 0: the plan chooses.
        out_len, block: what the plan writes per signal and the block length it uses."""
        dt = np.dtype(dtype)
        taps = np.ascontiguousarray(np.asarray(h).astype(dt)).reshape(-1)
        p = cls(init().fft_gpu_plan_filter_hip(taps.size, taps.ctypes.data if taps.size else None, signal_len, n_signals, n, FILTER_OUT[mode], _prec_of(dt)))
        p.n_signals, p.signal_len, p.mode, p.dtype = n_signals, signal_len, mode, dt
        p.out_len = p.lib.fft_gpu_filter_out_len_hip(p.handle)
        p.block = p.lib.fft_gpu_filter_block_hip(p.handle)
        return p

    @classmethod
    def conv2d(cls, k, rows, cols, n_matrices=1, mode="full", dtype=np.complex128):
        """2D convolution plan (fft_gpu_plan_conv2d_hip): n_matrices row-major rows x cols complex images, the kernel k ([krows, kcols]),
        the output of CONV2D_MODES[mode] ("full", "same", "valid": scipy.signal.convolve2d's; "circular": the kernel wraps, sizes powers of
        two; "spectrum": k IS the rows x cols spectrum H in natural order, out = ifft2(fft2(x) * H)).  out_rows, out_cols: what the plan
        writes per matrix; padded: (P, Q)."""
        dt = np.dtype(dtype)
        kk = np.ascontiguousarray(np.asarray(k).astype(dt))
        if kk.ndim != 2:
            raise ValueError("the kernel is a 2D array")
        p = cls(init().fft_gpu_plan_conv2d_hip(rows, cols, kk.shape[0], kk.shape[1], kk.ctypes.data if kk.size else None, n_matrices, CONV2D_MODES[mode],
                                               _prec_of(dt)))
        p.n_matrices, p.rows, p.cols, p.mode, p.dtype = n_matrices, rows, cols, mode, dt
        p.out_rows, p.out_cols = p.lib.fft_gpu_conv2d_out_rows_hip(p.handle), p.lib.fft_gpu_conv2d_out_cols_hip(p.handle)
        p.padded = (p.lib.fft_gpu_conv2d_padded_rows_hip(p.handle), p.lib.fft_gpu_conv2d_padded_cols_hip(p.handle))
        return p

    @classmethod
    def real2d(cls, rows, cols, n_matrices=1, inverse=False, dtype=np.float64):
        """Real 2D transform plan (fft_gpu_plan_r2c_2d_hip / fft_gpu_plan_c2r_2d_hip): n_matrices row-major rows x cols real images of
        dtype float32 / float64 and their one-sided spectra of rows x bins complex values, bins = cols // 2 + 1; numpy's rfft2, or with
        inverse=True irfft2(X, s=(rows, cols)).  execute(d_in, d_out, in_pitch, out_pitch) runs it on device pointers."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("float32 or float64 expected")
        prec = PREC_F32 if dt == np.float32 else PREC_F64
        lib = init()
        p = cls((lib.fft_gpu_plan_c2r_2d_hip if inverse else lib.fft_gpu_plan_r2c_2d_hip)(rows, cols, n_matrices, prec))
        p.n_matrices, p.rows, p.cols, p.inverse, p.dtype = n_matrices, rows, cols, bool(inverse), dt
        p.cdtype = np.dtype(np.complex64 if dt == np.float32 else np.complex128)
        p.bins = p.lib.fft_gpu_real2d_bins_hip(p.handle)
        p.execute = p.execute_real2d
        return p

    @classmethod
    def dct(cls, n, batch=1, type=DCT2, norm=DCT_NORM_NONE, dtype=np.float64):
        """DCT / DST plan of type II or III (fft_gpu_plan_dct_hip): batch rows of n reals of dtype float32 / float64, type DCT2 / DCT3 /
        DST2 / DST3, norm DCT_NORM_NONE / _INVERSE / _ORTHO.  execute(d_in, d_out, in_pitch, out_pitch) runs it on device pointers
        (pitches in reals between rows, 0: dense; d_in == d_out is allowed)."""
        p = cls(init().fft_gpu_plan_dct_hip(n, batch, type, norm, _real_prec(dtype)))
        p.n, p.batch, p.type, p.norm, p.dtype = n, batch, type, norm, np.dtype(dtype)
        p.execute = p.execute_dct
        return p

    @classmethod
    def dct2d(cls, rows, cols, n_matrices=1, type=DCT2, norm=DCT_NORM_NONE, dtype=np.float64):
        """The same transform along both axes of n_matrices row-major rows x cols real images (fft_gpu_plan_dct_2d_hip).  execute as
        ExtPlan.dct's, pitches in reals between matrices."""
        p = cls(init().fft_gpu_plan_dct_2d_hip(rows, cols, n_matrices, type, norm, _real_prec(dtype)))
        p.rows, p.cols, p.n_matrices, p.type, p.norm, p.dtype = rows, cols, n_matrices, type, norm, np.dtype(dtype)
        p.execute = p.execute_dct
        return p

    def execute_dct(self, d_in, d_out, in_pitch=0, out_pitch=0):
        if self.lib.fft_gpu_execute_dct_hip(self.handle, d_in, in_pitch, d_out, out_pitch) != 0:
            raise RuntimeError("fft_gpu_execute_dct_hip failed")

    def execute_real2d(self, d_in, d_out, in_pitch=0, out_pitch=0):
        if self.lib.fft_gpu_execute_real2d_hip(self.handle, d_in, in_pitch, d_out, out_pitch) != 0:
            raise RuntimeError("fft_gpu_execute_real2d_hip failed")

    def execute_conv2d(self, d_x, d_y, x_pitch=0, y_pitch=0):
        if self.lib.fft_gpu_execute_conv2d_hip(self.handle, d_x, x_pitch, d_y, y_pitch) != 0:
            raise RuntimeError("fft_gpu_execute_conv2d_hip failed")

    def execute_filter(self, d_x, d_y, x_pitch=0, y_pitch=0):
        if self.lib.fft_gpu_execute_filter_hip(self.handle, d_x, x_pitch, d_y, y_pitch) != 0:
            raise RuntimeError("fft_gpu_execute_filter_hip failed")

    def execute_cross(self, d_x, d_y, d_out, x_pitch=0, y_pitch=0, sample_rate=1.0):
        if self.lib.fft_gpu_execute_cross_frames_hip(self.handle, d_x, x_pitch, d_y, y_pitch, d_out, sample_rate) != 0:
            raise RuntimeError("fft_gpu_execute_cross_frames_hip failed")

    def execute_iframes(self, d_X, d_y, signal_pitch=0):
        if self.lib.fft_gpu_execute_iframes_hip(self.handle, d_X, d_y, signal_pitch) != 0:
            raise RuntimeError("fft_gpu_execute_iframes_hip failed")

    def set_stream(self, stream_ptr):
        self.lib.fft_gpu_plan_set_stream(self.handle, stream_ptr)

    def execute_frames(self, d_x, d_out, signal_pitch=0, sample_rate=1.0):
        if self.lib.fft_gpu_execute_frames_hip(self.handle, d_x, signal_pitch, d_out, sample_rate) != 0:
            raise RuntimeError("fft_gpu_execute_frames_hip failed")

    def execute_ptr(self, d_in, d_out):
        if self.lib.fft_gpu_execute_ptr(self.handle, d_in, d_out) != 0:
            raise RuntimeError("fft_gpu_execute_ptr failed")

    def set_option(self, option, value):
        if self.lib.fft_gpu_plan_set_option_hip(self.handle, option, value) != 0:
            raise RuntimeError("fft_gpu_plan_set_option_hip(%d) failed" % option)

    def info(self):
        pi = PlanInfo()
        self.lib.fft_gpu_plan_info(self.handle, C.byref(pi))
        return pi

    def execute_fused(self, d_x, d_y, d_out, sample_rate=1.0):
        if self.lib.fft_gpu_execute_fused_hip(self.handle, d_x, d_y, d_out, sample_rate) != 0:
            raise RuntimeError("fft_gpu_execute_fused_hip failed")

    def sync(self):
        return self.lib.fft_gpu_plan_sync(self.handle)

    def timed(self, d_in, d_out, iters):
        ms = C.c_float()
        if self.lib.fft_gpu_execute_timed(self.handle, d_in, d_out, iters, C.byref(ms)) != 0:
            raise RuntimeError("fft_gpu_execute_timed failed")
        return ms.value

    def destroy(self):
        if self.handle:
            self.lib.fft_gpu_destroy_plan(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _roundtrip(plan, x, out_shape, out_dtype, y=None, fused=False, fs=1.0):
    a = DeviceBuffer(x.nbytes)
    a.upload(x)
    out = np.empty(out_shape, dtype=out_dtype)
    o = DeviceBuffer(max(out.nbytes, 16))
    b = None
    if y is not None:
        b = DeviceBuffer(y.nbytes)
        b.upload(y)
    if fused:
        plan.execute_fused(a.ptr, b.ptr if b else None, o.ptr, fs)
    else:
        plan.execute_ptr(a.ptr, o.ptr)
    if plan.sync() != 0:
        raise RuntimeError("execute failed")
    res = o.download(out_shape, out_dtype)
    for buf in (a, o, b):
        if buf:
            buf.free()
    return res


def fft2d(x, direction=FFT_FORWARD, algo=ALGO_AUTO):
    """x: [rows, cols] or [matrices, rows, cols] complex -> 2D transform of every matrix."""
    x = np.ascontiguousarray(x)
    x3 = x.reshape((-1,) + x.shape[-2:])
    plan = ExtPlan.fft2d(x3.shape[1], x3.shape[2], x3.shape[0], direction, x3.dtype, algo)
    y = _roundtrip(plan, x3, x3.shape, x3.dtype)
    plan.destroy()
    return y.reshape(x.shape)


def _fftn(x, direction, name):
    x = np.asarray(x)
    if x.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)) or x.ndim not in (3, 4) or x.size == 0:
        raise ValueError("%s takes a non-empty complex64 or complex128 array of 3 dimensions, or 4 with the batch first" % name)
    a = np.ascontiguousarray(x)
    x4 = a.reshape((-1,) + a.shape[-3:])
    plan = ExtPlan.plan3d(x4.shape[1], x4.shape[2], x4.shape[3], x4.shape[0], direction, x4.dtype)
    try:
        y = _roundtrip(plan, x4, x4.shape, x4.dtype)
    finally:
        plan.destroy()
    return y.reshape(x.shape)


def fftn(x):
    """numpy.fft.fftn over the last three axes of a 3-D complex array, or of a 4-D one whose leading axis is the batch, on the device
    (ExtPlan.plan3d); the complex dtype is kept."""
    return _fftn(x, FFT_FORWARD, "fftn")


def ifftn(x):
    """numpy.fft.ifftn over the last three axes: ifftn(fftn(x)) = x."""
    return _fftn(x, FFT_INVERSE, "ifftn")


def rfft(x, algo=ALGO_AUTO):
    """x: [batch, n] float32/float64 -> [batch, n//2 + 1] complex."""
    x = np.ascontiguousarray(x)
    batch, n = x.shape
    cdt = np.complex64 if x.dtype == np.float32 else np.complex128
    plan = ExtPlan.r2c(n, batch, x.dtype, algo)
    y = _roundtrip(plan, x, (batch, n // 2 + 1), cdt)
    plan.destroy()
    return y


def irfft(X, n, algo=ALGO_AUTO):
    """X: [batch, n//2 + 1] complex -> [batch, n] real, scaled by 1/n."""
    X = np.ascontiguousarray(X)
    rdt = np.float32 if X.dtype == np.complex64 else np.float64
    plan = ExtPlan.c2r(n, X.shape[0], rdt, algo)
    y = _roundtrip(plan, X, (X.shape[0], n), rdt)
    plan.destroy()
    return y


def fused(kind, x, y=None, h=None, fs=1.0):
    """Batched fused consumer on host arrays: x [batch, nx] complex (see fft_hip.h fft_gpu_fused_t)."""
    x = np.ascontiguousarray(x)
    batch, nx = x.shape
    plan = ExtPlan.fused(kind, nx, batch, h, x.dtype)
    if kind == "psd":
        odt = np.float32 if x.dtype == np.complex64 else np.float64
    else:
        odt = x.dtype
    yy = None if y is None else np.ascontiguousarray(np.asarray(y).astype(x.dtype))
    res = _roundtrip(plan, x, (batch, plan.out_len), odt, y=yy, fused=True, fs=fs)
    plan.destroy()
    return res


def _frames(x, n, hop, window, out, fs):
    x = np.ascontiguousarray(x)
    x2 = x.reshape(1, -1) if x.ndim == 1 else x
    plan = ExtPlan.frames(n, hop, x2.shape[1], x2.shape[0], window, out, x2.dtype)
    shape, odt = plan.frames_out()
    a, o = DeviceBuffer(x2.nbytes), DeviceBuffer(int(np.prod(shape)) * odt.itemsize)
    a.upload(x2)
    plan.execute_frames(a.ptr, o.ptr, 0, fs)
    if plan.sync() != 0:
        raise RuntimeError("execute failed")
    res = o.download(shape, odt)
    a.free()
    o.free()
    plan.destroy()
    return res[0] if x.ndim == 1 else res


def fir_filter(x, h, mode="full", n=0, plan=None):
    """x: [signals, len] (or [len]) complex64 / complex128, h: the FIR taps -> [signals, out_len]: every signal convolved with h by
    overlap-save on the device (ExtPlan.filter).  mode "full": np.convolve(x, h); "causal": its first len samples, y[t] = sum_j h[j]
    x[t - j]; "same": np.convolve(x, h, 'same').  n: the block length (0: the plan's choice).  plan: an ExtPlan.filter to reuse (h,
    mode and n are then the plan's).  Convenience: a float32 / float64 x with real h is widened to complex and the real part of the
    result is returned -- no packed real path exists."""
    x = np.asarray(x)
    real = x.dtype in (np.dtype(np.float32), np.dtype(np.float64))
    if real and np.iscomplexobj(h):
        raise ValueError("a real signal takes real taps")
    if real:
        x = x.astype(np.complex64 if x.dtype == np.float32 else np.complex128)
    if x.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise ValueError("fir_filter takes float32, float64, complex64 or complex128 signals")
    x = np.ascontiguousarray(x)
    x2 = x.reshape(1, -1) if x.ndim == 1 else x
    own = plan is None
    if own:
        plan = ExtPlan.filter(h, x2.shape[1], x2.shape[0], mode, n, x2.dtype)
    elif (plan.n_signals, plan.signal_len, plan.dtype) != (x2.shape[0], x2.shape[1], x2.dtype):
        raise ValueError("the plan was made for another shape or precision")
    shape = (x2.shape[0], plan.out_len)
    a, o = DeviceBuffer(x2.nbytes), DeviceBuffer(shape[0] * shape[1] * x2.dtype.itemsize)
    try:
        a.upload(x2)
        plan.execute_filter(a.ptr, o.ptr, 0, 0)
        if plan.sync() != 0:
            raise RuntimeError("execute failed")
        res = o.download(shape, x2.dtype)
    finally:
        a.free()
        o.free()
        if own:
            plan.destroy()
    if real:
        res = np.ascontiguousarray(res.real)
    return res[0] if x.ndim == 1 else res


def conv2d(x, k, mode="full", plan=None):
    """x: [matrices, rows, cols] (or [rows, cols]) complex64 / complex128 images, k: [krows, kcols] -> every image convolved with k on
    the device (ExtPlan.conv2d).  mode "full", "same", "valid": scipy.signal.convolve2d(x, k, mode); "circular": rows and cols powers of
    two, the kernel (no larger than the image) wraps.  plan: an ExtPlan.conv2d to reuse (k and mode are then the plan's).  Convenience: a
    float32 / float64 x with a real k is widened to complex and the real part of the result is returned."""
    x = np.asarray(x)
    real = x.dtype in (np.dtype(np.float32), np.dtype(np.float64))
    if real and k is not None and np.iscomplexobj(k):
        raise ValueError("a real image takes a real kernel")
    if real:
        x = x.astype(np.complex64 if x.dtype == np.float32 else np.complex128)
    if x.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)) or x.ndim not in (2, 3):
        raise ValueError("conv2d takes [rows, cols] or [matrices, rows, cols] float32, float64, complex64 or complex128 images")
    x = np.ascontiguousarray(x)
    x3 = x.reshape((1,) + x.shape) if x.ndim == 2 else x
    own = plan is None
    if own:
        plan = ExtPlan.conv2d(k, x3.shape[1], x3.shape[2], x3.shape[0], mode, x3.dtype)
    elif (plan.n_matrices, plan.rows, plan.cols, plan.dtype) != (x3.shape[0], x3.shape[1], x3.shape[2], x3.dtype):
        raise ValueError("the plan was made for another shape or precision")
    shape = (x3.shape[0], plan.out_rows, plan.out_cols)
    a, o = DeviceBuffer(x3.nbytes), DeviceBuffer(shape[0] * shape[1] * shape[2] * x3.dtype.itemsize)
    try:
        a.upload(x3)
        plan.execute_conv2d(a.ptr, o.ptr, 0, 0)
        if plan.sync() != 0:
            raise RuntimeError("execute failed")
        res = o.download(shape, x3.dtype)
    finally:
        a.free()
        o.free()
        if own:
            plan.destroy()
    if real:
        res = np.ascontiguousarray(res.real)
    return res[0] if x.ndim == 2 else res


def _real2d(a, rows, cols, inverse):
    """a: [matrices, ...] contiguous input of one real 2D plan -> its output, through device buffers"""
    M = a.shape[0]
    plan = ExtPlan.real2d(rows, cols, M, inverse, np.float32 if a.dtype in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    shape, odt = ((M, rows, cols), plan.dtype) if inverse else ((M, rows, plan.bins), plan.cdtype)
    d_in, d_out = DeviceBuffer(a.nbytes), DeviceBuffer(M * shape[1] * shape[2] * odt.itemsize)
    try:
        d_in.upload(a)
        plan.execute_real2d(d_in.ptr, d_out.ptr, 0, 0)
        if plan.sync() != 0:
            raise RuntimeError("execute failed")
        return d_out.download(shape, odt)
    finally:
        d_in.free()
        d_out.free()
        plan.destroy()


def rfft2(x):
    """x: [..., rows, cols] float32 / float64 images -> [..., rows, cols // 2 + 1] complex64 / complex128, numpy.fft.rfft2 over the last
    two axes on the device (ExtPlan.real2d)."""
    x = np.asarray(x)
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.float64)) or x.ndim < 2 or x.size == 0:
        raise ValueError("rfft2 takes non-empty [..., rows, cols] float32 or float64 images")
    rows, cols = x.shape[-2:]
    res = _real2d(np.ascontiguousarray(x).reshape(-1, rows, cols), rows, cols, False)
    return res.reshape(x.shape[:-1] + (cols // 2 + 1,))


def irfft2(X, cols):
    """X: [..., rows, cols // 2 + 1] complex64 / complex128 one-sided spectra -> [..., rows, cols] float32 / float64,
    numpy.fft.irfft2(X, s=(rows, cols)) over the last two axes on the device: scaled by 1 / (rows cols), irfft2(rfft2(x), cols) = x."""
    X = np.asarray(X)
    if X.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)) or X.ndim < 2 or X.size == 0 or cols < 1 or X.shape[-1] != cols // 2 + 1:
        raise ValueError("irfft2 takes non-empty [..., rows, cols // 2 + 1] complex64 or complex128 spectra")
    rows = X.shape[-2]
    res = _real2d(np.ascontiguousarray(X).reshape(-1, rows, X.shape[-1]), rows, cols, True)
    return res.reshape(X.shape[:-2] + (rows, cols))


def _dct_any(x, kind, type, norm, inverse, two_d, name):
    """scipy.fft's dct / idct / dst / idst / dctn / idctn for types 2 and 3 on the device.  kind: 0 cosine, 2 sine.  scipy's inverse of
    type t is the forward transform of the other type, scaled by 1 / (2N) per axis; norm="ortho" scales both the same way."""
    x = np.asarray(x)
    if type not in (2, 3):
        raise NotImplementedError("%s: types 2 and 3 only" % name)
    if norm not in (None, "backward", "ortho"):
        raise ValueError("%s: norm None, 'backward' or 'ortho'" % name)
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.float64)) or x.ndim < (2 if two_d else 1) or x.size == 0:
        raise ValueError("%s takes non-empty float32 or float64 arrays" % name)
    t = kind + ((3 - type) if inverse else (type - 2))  # DCT2 / DCT3 / DST2 / DST3
    nm = DCT_NORM_ORTHO if norm == "ortho" else DCT_NORM_INVERSE if inverse else DCT_NORM_NONE
    a = np.ascontiguousarray(x)
    if two_d:
        rows, cols = x.shape[-2:]
        plan = ExtPlan.dct2d(rows, cols, a.size // (rows * cols), t, nm, x.dtype)
    else:
        plan = ExtPlan.dct(x.shape[-1], a.size // x.shape[-1], t, nm, x.dtype)
    buf = DeviceBuffer(a.nbytes)
    try:
        buf.upload(a)
        plan.execute_dct(buf.ptr, buf.ptr, 0, 0)
        if plan.sync() != 0:
            raise RuntimeError("execute failed")
        return buf.download(x.shape, x.dtype)
    finally:
        buf.free()
        plan.destroy()


def dct(x, type=2, norm=None):
    """scipy.fft.dct over the last axis of a float32 / float64 array, types 2 and 3, on the device (ExtPlan.dct)."""
    return _dct_any(x, DCT2, type, norm, False, False, "dct")


def idct(x, type=2, norm=None):
    """scipy.fft.idct over the last axis: idct(dct(x, type), type) = x."""
    return _dct_any(x, DCT2, type, norm, True, False, "idct")


def dst(x, type=2, norm=None):
    """scipy.fft.dst over the last axis, types 2 and 3."""
    return _dct_any(x, DST2, type, norm, False, False, "dst")


def idst(x, type=2, norm=None):
    """scipy.fft.idst over the last axis."""
    return _dct_any(x, DST2, type, norm, True, False, "idst")


def dctn(x, type=2, norm=None):
    """scipy.fft.dctn over the last two axes (ExtPlan.dct2d)."""
    return _dct_any(x, DCT2, type, norm, False, True, "dctn")


def idctn(x, type=2, norm=None):
    """scipy.fft.idctn over the last two axes."""
    return _dct_any(x, DCT2, type, norm, True, True, "idctn")


def filter2d(x, H):
    """x: [matrices, rows, cols] (or [rows, cols]) complex images, rows and cols powers of two; H: [rows, cols] spectrum in natural
    (unshifted) order, DC at [0, 0] -> ifft2(fft2(x) * H) on the device (ExtPlan.conv2d in "spectrum" mode).  A mask written in the
    centred layout goes through np.fft.ifftshift first."""
    return conv2d(x, H, "spectrum")


CONV2D_MODES = {"full": 0, "same": 1, "valid": 2, "circular": 3, "spectrum": 4}
FIR_TYPES = {"lowpass": 0, "highpass": 1, "bandpass": 2, "bandstop": 3, "custom": 4}


def design_fir(taps, kind, cutoff_low=0.0, cutoff_high=0.0, fs=1.0, transition=0.0):
    """FIR taps by frequency sampling (fft_design_fir_filter_gpu: the reference's design_fir_filter, inverse transform on the
    device): kind a name of FIR_TYPES or its number, cutoffs, sample rate and transition width in Hz -> [taps] complex128."""
    lib = init()
    ptr = lib.fft_design_fir_filter_gpu(taps, FIR_TYPES[kind] if isinstance(kind, str) else int(kind), cutoff_low, cutoff_high, fs, transition)
    if not ptr:
        raise RuntimeError("fft_design_fir_filter_gpu failed")
    h = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(taps, 2)).copy().view(np.complex128).reshape(taps)
    lib.fft_free(ptr)
    return h


def stft(x, n, hop, window="hann"):
    """x: [signals, len] (or [len]) complex -> [signals, frames, n] complex: the transform of every windowed frame
    x[s, w * hop : w * hop + n], frames = (len - (n - hop)) // hop; window: a name of WINDOWS or n real values.
    A float32 / float64 x (here, in spectrogram and in welch) is read as real signals where it lies -- no complex copy -- and
    the rows are one-sided: [signals, frames, n//2 + 1]."""
    return _frames(x, n, hop, window, "stft", 1.0)


def istft(X, n, hop, window="hann"):
    """X: [signals, frames, n//2 + 1] (or [frames, n//2 + 1]) complex64 / complex128, the one-sided rows stft() returns for real
    signals -> [signals, out_len] float32 / float64, out_len = (frames - 1) * hop + n: the least-squares inverse by weighted
    overlap-add with the same window, istft(stft(x)) = x wherever the window envelope does not vanish (those samples are 0)."""
    X = np.ascontiguousarray(X)
    if X.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise ValueError("istft takes complex64 or complex128 rows")
    X3 = X.reshape((1,) + X.shape) if X.ndim == 2 else X
    if X3.ndim != 3 or X3.shape[2] != n // 2 + 1:
        raise ValueError("istft takes [signals, frames, n//2 + 1] rows")
    rdt = np.dtype(np.float32 if X.dtype == np.complex64 else np.float64)
    plan = ExtPlan.iframes(n, hop, X3.shape[1], X3.shape[0], window, rdt)
    shape = (X3.shape[0], plan.out_len)
    a, o = DeviceBuffer(X3.nbytes), DeviceBuffer(shape[0] * shape[1] * rdt.itemsize)
    a.upload(X3)
    plan.execute_iframes(a.ptr, o.ptr, 0)
    if plan.sync() != 0:
        raise RuntimeError("execute failed")
    res = o.download(shape, rdt)
    a.free()
    o.free()
    plan.destroy()
    return res[0] if X.ndim == 2 else res


def spectrogram(x, n, hop, window="hann", fs=1.0):
    """-> [signals, frames, n//2 + 1] real: the one-sided periodogram of every frame."""
    return _frames(x, n, hop, window, "power", fs)


def welch(x, n, hop, window="hann", fs=1.0):
    """-> [signals, n//2 + 1] real: Welch's PSD, the mean of the frames' periodograms."""
    return _frames(x, n, hop, window, "welch", fs)


def _cross(x, y, n, hop, window, out, fs):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        raise ValueError("x and y have one shape and one dtype")
    x2, y2 = (x.reshape(1, -1), y.reshape(1, -1)) if x.ndim == 1 else (x, y)
    plan = ExtPlan.cross_frames(n, hop, x2.shape[1], x2.shape[0], window, out, x2.dtype)
    shape, odt = plan.cross_out()
    a, b, o = DeviceBuffer(x2.nbytes), DeviceBuffer(y2.nbytes), DeviceBuffer(int(np.prod(shape)) * odt.itemsize)
    a.upload(x2)
    b.upload(y2)
    plan.execute_cross(a.ptr, b.ptr, o.ptr, 0, 0, fs)
    if plan.sync() != 0:
        raise RuntimeError("execute failed")
    res = o.download(shape, odt)
    for buf in (a, b, o):
        buf.free()
    plan.destroy()
    return res[0] if x.ndim == 1 else res


def csd(x, y, n, hop, window="hann", fs=1.0):
    """x, y: [signals, len] (or [len]) float32 / float64 (real signals, read where they lie) or complex64 / complex128
    -> [signals, n//2 + 1] complex: the cross-spectral density Pxy = c_k mean_w conj(X_w) Y_w over the frames of stft()
    (scipy.signal.csd's convention and scaling, without detrending)."""
    return _cross(x, y, n, hop, window, "csd", fs)


def coherence(x, y, n, hop, window="hann"):
    """-> [signals, n//2 + 1] real: the magnitude-squared coherence |Pxy|^2 / (Pxx Pyy); 0 where Pxx Pyy is 0."""
    return _cross(x, y, n, hop, window, "coherence", 1.0)


def transfer(x, y, n, hop, window="hann"):
    """-> [signals, n//2 + 1] complex: the H1 transfer estimate Pxy / Pxx from x to y; 0 where Pxx is 0."""
    return _cross(x, y, n, hop, window, "transfer", 1.0)


def fft(x, direction=FFT_FORWARD, algo=ALGO_AUTO, inplace=True):
    """Host-array convenience: x [batch, n] (or [n]) complex64/complex128 -> transform on the GPU."""
    x = np.ascontiguousarray(x)
    squeeze = x.ndim == 1
    x2 = x.reshape(1, -1) if squeeze else x.reshape(-1, x.shape[-1])
    batch, n = x2.shape
    plan = Plan(n, batch, direction, x2.dtype, algo)
    a = DeviceBuffer(x2.nbytes)
    a.upload(x2)
    if inplace:
        plan.execute(a, a)
        out = a.download(x2.shape, x2.dtype)
    else:
        b = DeviceBuffer(x2.nbytes)
        plan.execute(a, b)
        out = b.download(x2.shape, x2.dtype)
        b.free()
    a.free()
    plan.destroy()
    return out.reshape(x.shape)
