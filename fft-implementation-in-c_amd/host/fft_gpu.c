/*
 * fft_gpu.c -- backend dispatcher of the public fft_gpu_* API (plain C).
 *
 * Role of the reference's gpu/fft_gpu.c:49-394: keep `g_current_backend`,
 * forward each public call to the active backend's symbol set.  The only
 * backend compiled here is the hand-written HIP engine, gated by the build
 * macro FFT_HAVE_HIP (the reference gates on __CUDACC__/__APPLE__, which a
 * plain gcc build never defines -- SURVEY.md fact 5).  There is NO CPU
 * fallback: without a usable device every call fails loudly (-1 / NULL +
 * a line on stderr).
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../include/fft_gpu.h"

#ifndef FFT_HAVE_HIP
#error "this dispatcher is only meaningful with the HIP backend: build with -DFFT_HAVE_HIP"
#endif

static fft_gpu_backend_t g_current_backend = FFT_GPU_NONE;

static int backend_is_hip(const char* what) {
    if (g_current_backend == FFT_GPU_HIP) return 1;
    fprintf(stderr, "fft_gpu: %s called without an initialised GPU backend (call fft_gpu_init first)\n", what);
    return 0;
}

int fft_gpu_init(fft_gpu_backend_t backend) {
    if (backend == FFT_GPU_AUTO) {
        if (!fft_gpu_available_hip()) {
            fprintf(stderr, "fft_gpu: no GPU backend available (HIP device not found)\n");
            return -1;
        }
        backend = FFT_GPU_HIP;
    }
    switch (backend) {
        case FFT_GPU_HIP:
            if (fft_gpu_init_hip() != 0) return -1;
            g_current_backend = FFT_GPU_HIP;
            return 0;
        case FFT_GPU_CUDA:
            fprintf(stderr, "CUDA support not compiled in\n");
            return -1;
        case FFT_GPU_METAL:
            fprintf(stderr, "Metal support only available on macOS\n");
            return -1;
        default:
            return -1;
    }
}

void fft_gpu_cleanup(void) {
    if (g_current_backend == FFT_GPU_HIP) fft_gpu_cleanup_hip();
    g_current_backend = FFT_GPU_NONE;
}

int fft_gpu_available(void) { return fft_gpu_available_hip() ? 1 : 0; }

fft_gpu_backend_t fft_gpu_get_backend(void) { return g_current_backend; }

fft_gpu_memory_t fft_gpu_alloc(size_t size) {
    if (!backend_is_hip("fft_gpu_alloc")) return NULL;
    return fft_gpu_alloc_hip(size);
}

fft_gpu_memory_t fft_gpu_alloc_f32(size_t size) {
    if (!backend_is_hip("fft_gpu_alloc_f32")) return NULL;
    return fft_gpu_alloc_bytes_hip(size * sizeof(complex32_t));
}

void fft_gpu_free(fft_gpu_memory_t mem) {
    if (!mem) return;
    fft_gpu_free_hip(mem);
}

void fft_gpu_copy_h2d(fft_gpu_memory_t dst, const complex_t* src, size_t size) {
    if (!backend_is_hip("fft_gpu_copy_h2d")) return;
    fft_gpu_copy_h2d_hip(dst, src, size);
}

void fft_gpu_copy_d2h(complex_t* dst, fft_gpu_memory_t src, size_t size) {
    if (!backend_is_hip("fft_gpu_copy_d2h")) return;
    fft_gpu_copy_d2h_hip(dst, src, size);
}

void fft_gpu_copy_h2d_f32(fft_gpu_memory_t dst, const complex32_t* src, size_t n) {
    if (!backend_is_hip("fft_gpu_copy_h2d_f32")) return;
    (void)fft_gpu_copy_h2d_bytes_hip(dst, src, n * sizeof(complex32_t));
}

void fft_gpu_copy_d2h_f32(complex32_t* dst, fft_gpu_memory_t src, size_t n) {
    if (!backend_is_hip("fft_gpu_copy_d2h_f32")) return;
    (void)fft_gpu_copy_d2h_bytes_hip(dst, src, n * sizeof(complex32_t));
}

void* fft_gpu_memory_ptr(fft_gpu_memory_t mem) { return fft_gpu_memory_ptr_hip(mem); }

fft_gpu_plan_t fft_gpu_plan_1d(int n, int batch, fft_direction direction) {
    if (!backend_is_hip("fft_gpu_plan_1d")) return NULL;
    return fft_gpu_plan_1d_hip(n, batch, direction);
}

fft_gpu_plan_t fft_gpu_plan_1d_f32(int n, int batch, fft_direction direction) {
    if (!backend_is_hip("fft_gpu_plan_1d_f32")) return NULL;
    return fft_gpu_plan_1d_ex_hip(n, batch, direction, FFT_PREC_F32, FFT_GPU_ALGO_AUTO);
}

fft_gpu_plan_t fft_gpu_plan_1d_ex(int n, int batch, fft_direction direction, fft_precision_t prec, fft_gpu_algo_t algo) {
    if (!backend_is_hip("fft_gpu_plan_1d_ex")) return NULL;
    return fft_gpu_plan_1d_ex_hip(n, batch, direction, prec, algo);
}

int fft_gpu_plan_info(fft_gpu_plan_t plan, fft_gpu_plan_info_t* info) { return fft_gpu_plan_info_hip(plan, info); }

int fft_gpu_plan_set_stream(fft_gpu_plan_t plan, void* hip_stream) { return fft_gpu_plan_set_stream_hip(plan, hip_stream); }

void fft_gpu_execute(fft_gpu_plan_t plan, fft_gpu_memory_t in, fft_gpu_memory_t out) {
    if (!plan) return;
    if (!backend_is_hip("fft_gpu_execute")) return;
    /* the plan carries its direction; the trailing argument only mirrors the backend signature */
    fft_gpu_execute_hip(plan, in, out, FFT_FORWARD);
}

int fft_gpu_execute_async(fft_gpu_plan_t plan, fft_gpu_memory_t in, fft_gpu_memory_t out) {
    if (!plan || !in || !out || !backend_is_hip("fft_gpu_execute_async")) return -1;
    return fft_gpu_execute_ptr_hip(plan, fft_gpu_memory_ptr_hip(in), fft_gpu_memory_ptr_hip(out));
}

int fft_gpu_execute_ptr(fft_gpu_plan_t plan, const void* d_in, void* d_out) {
    if (!backend_is_hip("fft_gpu_execute_ptr")) return -1;
    return fft_gpu_execute_ptr_hip(plan, d_in, d_out);
}

int fft_gpu_plan_sync(fft_gpu_plan_t plan) { return fft_gpu_plan_sync_hip(plan); }

int fft_gpu_execute_timed(fft_gpu_plan_t plan, const void* d_in, void* d_out, int iters, float* elapsed_ms) {
    if (!backend_is_hip("fft_gpu_execute_timed")) return -1;
    return fft_gpu_execute_timed_hip(plan, d_in, d_out, iters, elapsed_ms);
}

void fft_gpu_destroy_plan(fft_gpu_plan_t plan) {
    if (!plan) return;
    fft_gpu_destroy_plan_hip(plan);
}

const char* fft_gpu_get_device_name(void) {
    if (g_current_backend == FFT_GPU_HIP) return fft_gpu_get_device_name_hip();
    return "No GPU";
}

void fft_gpu_get_memory_info(size_t* total, size_t* available) {
    if (!total || !available) return;
    *total = 0;
    *available = 0;
    if (g_current_backend == FFT_GPU_HIP) fft_gpu_get_memory_info_hip(total, available);
}

static int lazy_init(void) {
    if (g_current_backend == FFT_GPU_HIP) return 0;
    return fft_gpu_init(FFT_GPU_AUTO);
}

int fft_gpu_dft_1d(complex_t* in, complex_t* out, int n, fft_direction direction) {
    if (!in || !out || n <= 0 || lazy_init() != 0) return -1;
    return fft_gpu_dft_1d_hip(in, out, n, direction);
}

int fft_gpu_dft_1d_batch(complex_t* in, complex_t* out, int n, int batch, fft_direction direction) {
    if (!in || !out || n <= 0 || batch <= 0 || lazy_init() != 0) return -1;
    return fft_gpu_dft_1d_batch_hip(in, out, n, batch, direction, FFT_PREC_F64);
}

int fft_gpu_dft_1d_f32(complex32_t* in, complex32_t* out, int n, fft_direction direction) {
    if (!in || !out || n <= 0 || lazy_init() != 0) return -1;
    return fft_gpu_dft_1d_batch_hip(in, out, n, 1, direction, FFT_PREC_F32);
}

int fft_gpu_dft_1d_batch_f32(complex32_t* in, complex32_t* out, int n, int batch, fft_direction direction) {
    if (!in || !out || n <= 0 || batch <= 0 || lazy_init() != 0) return -1;
    return fft_gpu_dft_1d_batch_hip(in, out, n, batch, direction, FFT_PREC_F32);
}

int fft_gpu_bit_reverse(fft_gpu_memory_t in, fft_gpu_memory_t out, int n, int batch, fft_precision_t prec) {
    if (!in || !out || !backend_is_hip("fft_gpu_bit_reverse")) return -1;
    return fft_gpu_bit_reverse_hip(fft_gpu_memory_ptr_hip(in), fft_gpu_memory_ptr_hip(out), n, batch, prec, NULL);
}

/* STFT / spectrogram / Welch plans on overlapping frames */
fft_gpu_plan_t fft_gpu_plan_frames(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                   fft_gpu_frames_out_t out, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_frames")) return NULL;
    return fft_gpu_plan_frames_hip(n, hop, signal_len, n_signals, window, w_host, out, prec);
}

fft_gpu_plan_t fft_gpu_plan_frames_real(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                        fft_gpu_frames_out_t out, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_frames_real")) return NULL;
    return fft_gpu_plan_frames_real_hip(n, hop, signal_len, n_signals, window, w_host, out, prec);
}

int fft_gpu_frames_count(fft_gpu_plan_t plan) { return fft_gpu_frames_count_hip(plan); }

int fft_gpu_execute_frames(fft_gpu_plan_t plan, const void* d_x, long long signal_pitch, void* d_out, double sample_rate) {
    if (!backend_is_hip("fft_gpu_execute_frames")) return -1;
    return fft_gpu_execute_frames_hip(plan, d_x, signal_pitch, d_out, sample_rate);
}

/* inverse STFT plans: one-sided rows back to real signals by overlap-add */
fft_gpu_plan_t fft_gpu_plan_iframes_real(int n, int hop, int n_frames, int n_signals, fft_gpu_window_t window, const void* w_host,
                                         fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_iframes_real")) return NULL;
    return fft_gpu_plan_iframes_real_hip(n, hop, n_frames, n_signals, window, w_host, prec);
}

int fft_gpu_iframes_len(fft_gpu_plan_t plan) { return fft_gpu_iframes_len_hip(plan); }

int fft_gpu_iframes_unrecoverable(fft_gpu_plan_t plan) { return fft_gpu_iframes_unrecoverable_hip(plan); }

int fft_gpu_execute_iframes(fft_gpu_plan_t plan, const void* d_X, void* d_y, long long signal_pitch) {
    if (!backend_is_hip("fft_gpu_execute_iframes")) return -1;
    return fft_gpu_execute_iframes_hip(plan, d_X, d_y, signal_pitch);
}

/* cross frames plans: cross-spectral density, coherence and transfer estimate of signal pairs */
fft_gpu_plan_t fft_gpu_plan_cross_frames(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                         fft_gpu_cross_out_t out, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_cross_frames")) return NULL;
    return fft_gpu_plan_cross_frames_hip(n, hop, signal_len, n_signals, window, w_host, out, prec);
}

fft_gpu_plan_t fft_gpu_plan_cross_frames_real(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                              fft_gpu_cross_out_t out, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_cross_frames_real")) return NULL;
    return fft_gpu_plan_cross_frames_real_hip(n, hop, signal_len, n_signals, window, w_host, out, prec);
}

int fft_gpu_cross_chunk(fft_gpu_plan_t plan) { return fft_gpu_cross_chunk_hip(plan); }

int fft_gpu_execute_cross_frames(fft_gpu_plan_t plan, const void* d_x, long long x_pitch, const void* d_y, long long y_pitch, void* d_out,
                                 double sample_rate) {
    if (!backend_is_hip("fft_gpu_execute_cross_frames")) return -1;
    return fft_gpu_execute_cross_frames_hip(plan, d_x, x_pitch, d_y, y_pitch, d_out, sample_rate);
}

/* filter plans: overlap-save FIR filtering of long signals */
fft_gpu_plan_t fft_gpu_plan_filter(int n_taps, const void* h_host, int signal_len, int n_signals, int n, fft_gpu_filter_out_t out,
                                   fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_filter")) return NULL;
    return fft_gpu_plan_filter_hip(n_taps, h_host, signal_len, n_signals, n, out, prec);
}

int fft_gpu_filter_out_len(fft_gpu_plan_t plan) { return fft_gpu_filter_out_len_hip(plan); }

int fft_gpu_filter_block(fft_gpu_plan_t plan) { return fft_gpu_filter_block_hip(plan); }

int fft_gpu_execute_filter(fft_gpu_plan_t plan, const void* d_x, long long x_pitch, void* d_y, long long y_pitch) {
    if (!backend_is_hip("fft_gpu_execute_filter")) return -1;
    return fft_gpu_execute_filter_hip(plan, d_x, x_pitch, d_y, y_pitch);
}

/* 2D convolution plans: convolution and spectrum filtering of images */
fft_gpu_plan_t fft_gpu_plan_conv2d(int rows, int cols, int krows, int kcols, const void* k_host, int n_matrices, fft_gpu_conv2d_t mode,
                                   fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_conv2d")) return NULL;
    return fft_gpu_plan_conv2d_hip(rows, cols, krows, kcols, k_host, n_matrices, mode, prec);
}

int fft_gpu_conv2d_out_rows(fft_gpu_plan_t plan) { return fft_gpu_conv2d_out_rows_hip(plan); }

int fft_gpu_conv2d_out_cols(fft_gpu_plan_t plan) { return fft_gpu_conv2d_out_cols_hip(plan); }

int fft_gpu_conv2d_padded_rows(fft_gpu_plan_t plan) { return fft_gpu_conv2d_padded_rows_hip(plan); }

int fft_gpu_conv2d_padded_cols(fft_gpu_plan_t plan) { return fft_gpu_conv2d_padded_cols_hip(plan); }

int fft_gpu_execute_conv2d(fft_gpu_plan_t plan, const void* d_x, long long x_pitch, void* d_y, long long y_pitch) {
    if (!backend_is_hip("fft_gpu_execute_conv2d")) return -1;
    return fft_gpu_execute_conv2d_hip(plan, d_x, x_pitch, d_y, y_pitch);
}

/* real 2D plans, rfft2 / irfft2 (fft_hip.h) */
fft_gpu_plan_t fft_gpu_plan_r2c_2d(int rows, int cols, int n_matrices, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_r2c_2d")) return NULL;
    return fft_gpu_plan_r2c_2d_hip(rows, cols, n_matrices, prec);
}

fft_gpu_plan_t fft_gpu_plan_c2r_2d(int rows, int cols, int n_matrices, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_c2r_2d")) return NULL;
    return fft_gpu_plan_c2r_2d_hip(rows, cols, n_matrices, prec);
}

int fft_gpu_real2d_bins(fft_gpu_plan_t plan) { return fft_gpu_real2d_bins_hip(plan); }

int fft_gpu_execute_real2d(fft_gpu_plan_t plan, const void* d_in, long long in_pitch, void* d_out, long long out_pitch) {
    if (!backend_is_hip("fft_gpu_execute_real2d")) return -1;
    return fft_gpu_execute_real2d_hip(plan, d_in, in_pitch, d_out, out_pitch);
}

/* DCT / DST plans of types II and III (fft_hip.h) */
fft_gpu_plan_t fft_gpu_plan_dct(int n, int batch, fft_gpu_dct_t type, fft_gpu_dct_norm_t norm, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_dct")) return NULL;
    return fft_gpu_plan_dct_hip(n, batch, type, norm, prec);
}

fft_gpu_plan_t fft_gpu_plan_dct_2d(int rows, int cols, int n_matrices, fft_gpu_dct_t type, fft_gpu_dct_norm_t norm, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_dct_2d")) return NULL;
    return fft_gpu_plan_dct_2d_hip(rows, cols, n_matrices, type, norm, prec);
}

int fft_gpu_execute_dct(fft_gpu_plan_t plan, const void* d_in, long long in_pitch, void* d_out, long long out_pitch) {
    if (!backend_is_hip("fft_gpu_execute_dct")) return -1;
    return fft_gpu_execute_dct_hip(plan, d_in, in_pitch, d_out, out_pitch);
}

/* 3D complex plans (fft_hip.h) */
fft_gpu_plan_t fft_gpu_plan_3d(int depth, int rows, int cols, int n_volumes, fft_direction direction, fft_precision_t prec) {
    if (!backend_is_hip("fft_gpu_plan_3d")) return NULL;
    return fft_gpu_plan_3d_hip(depth, rows, cols, n_volumes, direction, prec);
}

int fft_gpu_device_count(void) { return fft_gpu_device_count_hip(); }

/* a stub in the reference (gpu/fft_gpu.c:359-363); real here: later allocations and plans go to `device` */
int fft_gpu_set_device(int device) { return fft_gpu_set_device_hip(device); }

/* 2D: real here (stubs returning NULL / -1 in the reference, gpu/fft_gpu.c:377-394) */
fft_gpu_plan_t fft_gpu_plan_2d(int rows, int cols, fft_direction direction) {
    if (!backend_is_hip("fft_gpu_plan_2d")) return NULL;
    return fft_gpu_plan_2d_hip(rows, cols, direction);
}

fft_gpu_plan_t fft_gpu_plan_2d_algo(int rows, int cols, int n_matrices, fft_direction direction, fft_precision_t prec, fft_gpu_algo_t algo) {
    if (!backend_is_hip("fft_gpu_plan_2d_algo")) return NULL;
    return fft_gpu_plan_2d_algo_hip(rows, cols, n_matrices, direction, prec, algo);
}

/* host arrays, row-major; one matrix (7-smooth sizes follow fft_gpu_set_smooth_policy_hip, like every AUTO plan) */
int fft_gpu_dft_2d(complex_t* in, complex_t* out, int rows, int cols, fft_direction direction) {
    if (!in || !out || rows <= 0 || cols <= 0 || lazy_init() != 0) return -1;
    const size_t n = (size_t)rows * (size_t)cols;
    fft_gpu_plan_t plan = fft_gpu_plan_2d_hip(rows, cols, direction);
    fft_gpu_memory_t buf = plan ? fft_gpu_alloc_hip(n) : NULL;
    int rc = -1;
    if (plan && buf) {
        fft_gpu_copy_h2d_hip(buf, in, n);
        if (fft_gpu_execute_ptr_hip(plan, fft_gpu_memory_ptr_hip(buf), fft_gpu_memory_ptr_hip(buf)) == 0 && fft_gpu_plan_sync_hip(plan) == 0) {
            fft_gpu_copy_d2h_hip(out, buf, n);
            rc = 0;
        }
    }
    fft_gpu_free_hip(buf);
    fft_gpu_destroy_plan_hip(plan);
    return rc;
}

/* host arrays, row-major, cols fastest; one volume */
int fft_gpu_dft_3d(complex_t* in, complex_t* out, int depth, int rows, int cols, fft_direction direction) {
    if (!in || !out || depth <= 0 || rows <= 0 || cols <= 0 || (long long)depth * rows * cols > (1ll << 30)) return -1;
    if (lazy_init() != 0) {
        fprintf(stderr, "fft_gpu_dft_3d: no GPU device\n");
        return -1;
    }
    const size_t n = (size_t)depth * (size_t)rows * (size_t)cols;
    fft_gpu_plan_t plan = fft_gpu_plan_3d_hip(depth, rows, cols, 1, direction, FFT_PREC_F64);
    fft_gpu_memory_t buf = plan ? fft_gpu_alloc_hip(n) : NULL;
    int rc = -1;
    if (plan && buf) {
        fft_gpu_copy_h2d_hip(buf, in, n);
        if (fft_gpu_execute_ptr_hip(plan, fft_gpu_memory_ptr_hip(buf), fft_gpu_memory_ptr_hip(buf)) == 0 && fft_gpu_plan_sync_hip(plan) == 0) {
            fft_gpu_copy_d2h_hip(out, buf, n);
            rc = 0;
        }
    }
    fft_gpu_free_hip(buf);
    fft_gpu_destroy_plan_hip(plan);
    return rc;
}
