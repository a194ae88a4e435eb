/*
 * fft_apps.c -- host-array front ends of the fused consumers (include/fft_apps.h): the reference's
 * applications/convolution.c:34-96 and applications/power_spectrum.c:58-86, 133-190 as one fused device plan each, and
 * applications/fft_filtering.c's FIR design with FIR filtering of a long signal as one overlap-save filter plan, and the 2D
 * convolution applications/convolution.c:99-109 leaves as a placeholder with image_fft.c's spectrum masking as one 2D convolution plan.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/fft_apps.h"
#include "../../include/fft_gpu.h"
#include "../../include/fft_hip.h"

static int ensure_gpu(void) {
    if (fft_gpu_get_backend() == FFT_GPU_HIP) return 0;
    return fft_gpu_init(FFT_GPU_AUTO);
}

/* plan, upload, execute, download: x (nx) [, y (nx)] -> out (out_bytes) */
static int run_fused(fft_gpu_fused_t kind, const complex_t* x, const complex_t* y, int nx, const complex_t* h, int nh, void* out, size_t out_bytes,
                     double sample_rate) {
    if (!x || nx <= 0 || !out || ensure_gpu() != 0) return -1;
    int rc = -1;
    fft_gpu_plan_t plan = fft_gpu_plan_fused_hip(kind, nx, nh, h, 1, FFT_PREC_F64);
    fft_gpu_memory_t dx = plan ? fft_gpu_alloc((size_t)nx) : NULL;
    fft_gpu_memory_t dy = (plan && y) ? fft_gpu_alloc((size_t)nx) : NULL;
    fft_gpu_memory_t dout = plan ? fft_gpu_alloc_bytes_hip(out_bytes) : NULL;
    if (plan && dx && dout && (!y || dy)) {
        fft_gpu_copy_h2d(dx, x, (size_t)nx);
        if (y) fft_gpu_copy_h2d(dy, y, (size_t)nx);
        if (fft_gpu_execute_fused_hip(plan, fft_gpu_memory_ptr(dx), y ? fft_gpu_memory_ptr(dy) : NULL, fft_gpu_memory_ptr(dout), sample_rate) == 0 &&
            fft_gpu_plan_sync(plan) == 0 && fft_gpu_copy_d2h_bytes_hip(out, dout, out_bytes) == 0)
            rc = 0;
    }
    fft_gpu_free(dx);
    fft_gpu_free(dy);
    fft_gpu_free(dout);
    fft_gpu_destroy_plan(plan);
    return rc;
}

int fft_convolution_gpu(const complex_t* x, int nx, const complex_t* h, int nh, complex_t* y) {
    if (!h || nh <= 0) return -1;
    return run_fused(FFT_GPU_FUSED_CONV_LINEAR, x, NULL, nx, h, nh, y, (size_t)(nx + nh - 1) * sizeof(complex_t), 1.0);
}

int circular_convolution_gpu(const complex_t* x, const complex_t* h, int n, complex_t* y) {
    if (!h) return -1;
    if (!is_power_of_two(n)) {
        fprintf(stderr, "Error: Size %d is not a power of two\n", n);
        return -1;
    }
    return run_fused(FFT_GPU_FUSED_CONV_CIRCULAR, x, NULL, n, h, n, y, (size_t)n * sizeof(complex_t), 1.0);
}

double* compute_periodogram_gpu(const complex_t* signal, int n, double sample_rate) {
    if (n <= 0 || !is_power_of_two(n)) {
        fprintf(stderr, "Error: Size %d is not a power of two\n", n);
        return NULL;
    }
    double* psd = (double*)malloc(((size_t)n / 2 + 1) * sizeof(double));
    if (!psd) return NULL;
    if (run_fused(FFT_GPU_FUSED_PSD, signal, NULL, n, NULL, 0, psd, ((size_t)n / 2 + 1) * sizeof(double), sample_rate) != 0) {
        free(psd);
        return NULL;
    }
    return psd;
}

complex_t* autocorrelation_fft_gpu(const complex_t* signal, int n) {
    complex_t* acf = n > 0 ? allocate_complex_array(n) : NULL;
    if (!acf) return NULL;
    if (run_fused(FFT_GPU_FUSED_AUTOCORR, signal, NULL, n, NULL, 0, acf, (size_t)n * sizeof(complex_t), 1.0) != 0) {
        free_complex_array(acf);
        return NULL;
    }
    return acf;
}

complex_t* cross_correlation_fft_gpu(const complex_t* x, const complex_t* y, int n) {
    complex_t* ccf = (n > 0 && y) ? allocate_complex_array(n) : NULL;
    if (!ccf) return NULL;
    if (run_fused(FFT_GPU_FUSED_XCORR, x, y, n, NULL, 0, ccf, (size_t)n * sizeof(complex_t), 1.0) != 0) {
        free_complex_array(ccf);
        return NULL;
    }
    return ccf;
}

double* fft_welch_psd_gpu(const complex_t* signal, int signal_len, double sample_rate, int window_size, int overlap) {
    if (!signal || window_size < 2 || !is_power_of_two(window_size) || overlap < 0 || overlap >= window_size || signal_len < window_size) {
        fprintf(stderr, "Error: Welch PSD needs a power-of-two window_size >= 2, 0 <= overlap < window_size <= signal_len\n");
        return NULL;
    }
    if (ensure_gpu() != 0) return NULL;
    const size_t bins = (size_t)window_size / 2 + 1;
    double* psd = (double*)malloc(bins * sizeof(double));
    if (!psd) return NULL;
    int rc = -1;
    fft_gpu_plan_t plan = fft_gpu_plan_frames_hip(window_size, window_size - overlap, signal_len, 1, FFT_GPU_WINDOW_HANN, NULL, FFT_GPU_FRAMES_WELCH,
                                                  FFT_PREC_F64);
    fft_gpu_memory_t dx = plan ? fft_gpu_alloc((size_t)signal_len) : NULL;
    fft_gpu_memory_t dout = plan ? fft_gpu_alloc_bytes_hip(bins * sizeof(double)) : NULL;
    if (plan && dx && dout) {
        fft_gpu_copy_h2d(dx, signal, (size_t)signal_len);
        if (fft_gpu_execute_frames_hip(plan, fft_gpu_memory_ptr(dx), 0, fft_gpu_memory_ptr(dout), sample_rate) == 0 && fft_gpu_plan_sync(plan) == 0 &&
            fft_gpu_copy_d2h_bytes_hip(psd, dout, bins * sizeof(double)) == 0)
            rc = 0;
    }
    fft_gpu_free(dx);
    fft_gpu_free(dout);
    fft_gpu_destroy_plan(plan);
    if (rc != 0) {
        free(psd);
        return NULL;
    }
    return psd;
}

double* fft_welch_psd_real_gpu(const double* signal, int signal_len, double sample_rate, int window_size, int overlap) {
    if (!signal || window_size < 4 || !is_power_of_two(window_size) || overlap < 0 || overlap >= window_size || signal_len < window_size) {
        fprintf(stderr, "Error: real Welch PSD needs a power-of-two window_size >= 4, 0 <= overlap < window_size <= signal_len\n");
        return NULL;
    }
    if (ensure_gpu() != 0) return NULL;
    const size_t bins = (size_t)window_size / 2 + 1;
    double* psd = (double*)malloc(bins * sizeof(double));
    if (!psd) return NULL;
    int rc = -1;
    fft_gpu_plan_t plan = fft_gpu_plan_frames_real_hip(window_size, window_size - overlap, signal_len, 1, FFT_GPU_WINDOW_HANN, NULL, FFT_GPU_FRAMES_WELCH,
                                                       FFT_PREC_F64);
    fft_gpu_memory_t dx = plan ? fft_gpu_alloc_bytes_hip((size_t)signal_len * sizeof(double)) : NULL;
    fft_gpu_memory_t dout = plan ? fft_gpu_alloc_bytes_hip(bins * sizeof(double)) : NULL;
    if (plan && dx && dout) {
        if (fft_gpu_copy_h2d_bytes_hip(dx, signal, (size_t)signal_len * sizeof(double)) == 0 &&
            fft_gpu_execute_frames_hip(plan, fft_gpu_memory_ptr(dx), 0, fft_gpu_memory_ptr(dout), sample_rate) == 0 && fft_gpu_plan_sync(plan) == 0 &&
            fft_gpu_copy_d2h_bytes_hip(psd, dout, bins * sizeof(double)) == 0)
            rc = 0;
    }
    fft_gpu_free(dx);
    fft_gpu_free(dout);
    fft_gpu_destroy_plan(plan);
    if (rc != 0) {
        free(psd);
        return NULL;
    }
    return psd;
}

/* plan, upload both signals, execute, download: one pair through a cross frames plan (elem_bytes: 8 real, 16 complex samples) */
static int run_cross(int real_input, const void* x, const void* y, int n, double sample_rate, int window_size, int overlap, fft_gpu_cross_out_t kind,
                     void* out, size_t out_bytes) {
    if (!x || !y || !out || window_size < (real_input ? 4 : 2) || !is_power_of_two(window_size) || overlap < 0 || overlap >= window_size ||
        n < window_size) {
        fprintf(stderr, "Error: cross spectra need a power-of-two window_size >= %d, 0 <= overlap < window_size <= n\n", real_input ? 4 : 2);
        return -1;
    }
    if (ensure_gpu() != 0) return -1;
    const size_t in_bytes = (size_t)n * (real_input ? sizeof(double) : sizeof(complex_t));
    int rc = -1;
    fft_gpu_plan_t plan = real_input ? fft_gpu_plan_cross_frames_real_hip(window_size, window_size - overlap, n, 1, FFT_GPU_WINDOW_HANN, NULL, kind, FFT_PREC_F64)
                                     : fft_gpu_plan_cross_frames_hip(window_size, window_size - overlap, n, 1, FFT_GPU_WINDOW_HANN, NULL, kind, FFT_PREC_F64);
    fft_gpu_memory_t dx = plan ? fft_gpu_alloc_bytes_hip(in_bytes) : NULL;
    fft_gpu_memory_t dy = plan ? fft_gpu_alloc_bytes_hip(in_bytes) : NULL;
    fft_gpu_memory_t dout = plan ? fft_gpu_alloc_bytes_hip(out_bytes) : NULL;
    if (plan && dx && dy && dout) {
        if (fft_gpu_copy_h2d_bytes_hip(dx, x, in_bytes) == 0 && fft_gpu_copy_h2d_bytes_hip(dy, y, in_bytes) == 0 &&
            fft_gpu_execute_cross_frames_hip(plan, fft_gpu_memory_ptr(dx), 0, fft_gpu_memory_ptr(dy), 0, fft_gpu_memory_ptr(dout), sample_rate) == 0 &&
            fft_gpu_plan_sync(plan) == 0 && fft_gpu_copy_d2h_bytes_hip(out, dout, out_bytes) == 0)
            rc = 0;
    }
    fft_gpu_free(dx);
    fft_gpu_free(dy);
    fft_gpu_free(dout);
    fft_gpu_destroy_plan(plan);
    return rc;
}

static double* coherence_of(int real_input, const void* x, const void* y, int n, int window_size, int overlap) {
    if (window_size < 2) return NULL;
    const size_t bytes = ((size_t)window_size / 2 + 1) * sizeof(double);
    double* coh = (double*)malloc(bytes);
    if (!coh) return NULL;
    if (run_cross(real_input, x, y, n, 1.0, window_size, overlap, FFT_GPU_CROSS_COHERENCE, coh, bytes) != 0) {
        free(coh);
        return NULL;
    }
    return coh;
}

double* compute_coherence_gpu(const complex_t* x, const complex_t* y, int n, int window_size) {
    return coherence_of(0, x, y, n, window_size, window_size / 2);
}

double* fft_coherence_real_gpu(const double* x, const double* y, int n, int window_size, int overlap) {
    return coherence_of(1, x, y, n, window_size, overlap);
}

int fft_csd_real_gpu(const double* x, const double* y, int n, double sample_rate, int window_size, int overlap, complex_t* pxy) {
    if (window_size < 4) return -1;
    return run_cross(1, x, y, n, sample_rate, window_size, overlap, FFT_GPU_CROSS_CSD, pxy, ((size_t)window_size / 2 + 1) * sizeof(complex_t));
}

/* y = x * h through ONE overlap-save filter plan (fft_gpu_plan_filter_hip, FULL output): any nx, the block length is the plan's */
int fft_fir_filter_gpu(const complex_t* x, int nx, const complex_t* h, int nh, complex_t* y) {
    if (!x || !h || !y || nx <= 0 || nh <= 0 || ensure_gpu() != 0) return -1;
    const size_t ny = (size_t)nx + (size_t)nh - 1;
    int rc = -1;
    fft_gpu_plan_t plan = fft_gpu_plan_filter_hip(nh, h, nx, 1, 0, FFT_GPU_FILTER_FULL, FFT_PREC_F64);
    fft_gpu_memory_t dx = plan ? fft_gpu_alloc((size_t)nx) : NULL;
    fft_gpu_memory_t dy = plan ? fft_gpu_alloc(ny) : NULL;
    if (plan && dx && dy) {
        if (fft_gpu_copy_h2d_bytes_hip(dx, x, (size_t)nx * sizeof(complex_t)) == 0 &&
            fft_gpu_execute_filter_hip(plan, fft_gpu_memory_ptr(dx), 0, fft_gpu_memory_ptr(dy), 0) == 0 && fft_gpu_plan_sync(plan) == 0 &&
            fft_gpu_copy_d2h_bytes_hip(y, dy, ny * sizeof(complex_t)) == 0)
            rc = 0;
    }
    fft_gpu_free(dx);
    fft_gpu_free(dy);
    fft_gpu_destroy_plan(plan);
    return rc;
}

/* magnitude of the sampled response at frequency f (Hz, signed): the ideal response of the filter type, then -- low-pass and high-pass
 * only, as in the reference -- the raised-cosine transition of width tw centred on the cutoff */
static double fir_response(int type, double f, double lo, double hi, double tw) {
    const double a = fabs(f);
    double mag;
    switch (type) {
        case 0: mag = a <= lo ? 1.0 : 0.0; break;
        case 1: mag = a >= hi ? 1.0 : 0.0; break;
        case 2: mag = (a >= lo && a <= hi) ? 1.0 : 0.0; break;
        case 3: mag = (a < lo || a > hi) ? 1.0 : 0.0; break;
        default: mag = 1.0; break;
    }
    if (type == 0 && a > lo - tw / 2 && a < lo + tw / 2) mag = 0.5 * (1.0 + cos(PI * ((a - (lo - tw / 2)) / tw)));
    if (type == 1 && a > hi - tw / 2 && a < hi + tw / 2) mag = 0.5 * (1.0 - cos(PI * ((a - (hi - tw / 2)) / tw)));
    return mag;
}

complex_t* fft_design_fir_filter_gpu(int taps, int type, double cutoff_low, double cutoff_high, double sample_rate, double transition_width) {
    if (taps < 2 || taps > (1 << 26) || type < 0 || type > 4 || !(sample_rate > 0.0)) {
        fprintf(stderr, "Error: FIR design needs 2 <= taps <= 2^26, a filter type 0 ... 4 and a positive sample rate\n");
        return NULL;
    }
    if (ensure_gpu() != 0) return NULL;
    const int n = next_power_of_two(taps * 4);
    complex_t* H = allocate_complex_array(n);
    complex_t* h = allocate_complex_array(taps);
    int rc = -1;
    if (H && h) {
        const double bin = sample_rate / n;
        for (int k = 0; k < n; k++) H[k] = fir_response(type, (k > n / 2 ? k - n : k) * bin, cutoff_low, cutoff_high, transition_width);
        fft_gpu_plan_t plan = fft_gpu_plan_1d(n, 1, FFT_INVERSE);
        fft_gpu_memory_t d = plan ? fft_gpu_alloc((size_t)n) : NULL;
        if (plan && d) {
            if (fft_gpu_copy_h2d_bytes_hip(d, H, (size_t)n * sizeof(complex_t)) == 0 &&
                fft_gpu_execute_ptr(plan, fft_gpu_memory_ptr(d), fft_gpu_memory_ptr(d)) == 0 && fft_gpu_plan_sync(plan) == 0 &&
                fft_gpu_copy_d2h_bytes_hip(H, d, (size_t)n * sizeof(complex_t)) == 0)
                rc = 0;
        }
        fft_gpu_free(d);
        fft_gpu_destroy_plan(plan);
    }
    if (rc == 0) {
        const int shift = taps / 2;
        for (int i = 0; i < taps; i++) h[i] = H[(i - shift + n) % n] * (0.54 - 0.46 * cos(TWO_PI * i / (taps - 1)));
    }
    if (H) free_complex_array(H);
    if (rc != 0) {
        if (h) free_complex_array(h);
        return NULL;
    }
    return h;
}

/* one 2D convolution plan on host arrays: x (rows x cols, row-major) -> y (out_rows x out_cols) */
static int run_conv2d(const complex_t* x, int rows, int cols, const complex_t* k, int krows, int kcols, fft_gpu_conv2d_t mode, complex_t* y) {
    if (ensure_gpu() != 0) return -1;
    int rc = -1;
    fft_gpu_plan_t plan = fft_gpu_plan_conv2d_hip(rows, cols, krows, kcols, k, 1, mode, FFT_PREC_F64);
    const size_t nx = (size_t)rows * (size_t)cols;
    const size_t ny = plan ? (size_t)fft_gpu_conv2d_out_rows_hip(plan) * (size_t)fft_gpu_conv2d_out_cols_hip(plan) : 0;
    fft_gpu_memory_t dx = plan ? fft_gpu_alloc(nx) : NULL;
    fft_gpu_memory_t dy = plan ? fft_gpu_alloc(ny) : NULL;
    if (plan && dx && dy) {
        if (fft_gpu_copy_h2d_bytes_hip(dx, x, nx * sizeof(complex_t)) == 0 &&
            fft_gpu_execute_conv2d_hip(plan, fft_gpu_memory_ptr(dx), 0, fft_gpu_memory_ptr(dy), 0) == 0 && fft_gpu_plan_sync(plan) == 0 &&
            fft_gpu_copy_d2h_bytes_hip(y, dy, ny * sizeof(complex_t)) == 0)
            rc = 0;
    }
    fft_gpu_free(dx);
    fft_gpu_free(dy);
    fft_gpu_destroy_plan(plan);
    return rc;
}

int fft_convolution_2d_gpu(complex_t** image, int rows, int cols, complex_t** kernel, int krows, int kcols, complex_t** result) {
    if (!image || !kernel || !result || rows <= 0 || cols <= 0 || krows <= 0 || kcols <= 0) return -1;
    const long long orows = (long long)rows + krows - 1, ocols = (long long)cols + kcols - 1;
    if (orows * ocols > (1ll << 30)) return -1;
    complex_t* x = allocate_complex_array(rows * cols);
    complex_t* k = allocate_complex_array(krows * kcols);
    complex_t* y = allocate_complex_array((int)(orows * ocols));
    int rc = -1;
    if (x && k && y) {
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++) x[(size_t)i * cols + j] = image[i][j];
        for (int i = 0; i < krows; i++)
            for (int j = 0; j < kcols; j++) k[(size_t)i * kcols + j] = kernel[i][j];
        rc = run_conv2d(x, rows, cols, k, krows, kcols, FFT_GPU_CONV2D_FULL, y);
        if (rc == 0)
            for (long long i = 0; i < orows; i++)
                for (long long j = 0; j < ocols; j++) result[i][j] = y[i * ocols + j];
    }
    if (x) free_complex_array(x);
    if (k) free_complex_array(k);
    if (y) free_complex_array(y);
    return rc;
}

int fft_filter_2d_gpu(const complex_t* image, int rows, int cols, const complex_t* H_centred, complex_t* out) {
    if (!image || !H_centred || !out || rows <= 0 || cols <= 0 || !is_power_of_two(rows) || !is_power_of_two(cols)) return -1;
    if ((long long)rows * cols > (1ll << 30)) return -1;
    complex_t* H = allocate_complex_array(rows * cols);
    if (!H) return -1;
    /* fft_shift_2d puts bin (u, v) at [(u + rows/2) mod rows][(v + cols/2) mod cols]: undo it */
    for (int u = 0; u < rows; u++)
        for (int v = 0; v < cols; v++) H[(size_t)u * cols + v] = H_centred[(size_t)((u + rows / 2) % rows) * cols + (size_t)((v + cols / 2) % cols)];
    const int rc = run_conv2d(image, rows, cols, H, rows, cols, FFT_GPU_CONV2D_SPECTRUM, out);
    free_complex_array(H);
    return rc;
}

/* one real 2D plan on host arrays: `in` (in_bytes) -> `out` (out_bytes) */
static int run_real2d(const void* in, size_t in_bytes, void* out, size_t out_bytes, int rows, int cols, int r2c) {
    if (ensure_gpu() != 0) return -1;
    int rc = -1;
    fft_gpu_plan_t plan = r2c ? fft_gpu_plan_r2c_2d_hip(rows, cols, 1, FFT_PREC_F64) : fft_gpu_plan_c2r_2d_hip(rows, cols, 1, FFT_PREC_F64);
    fft_gpu_memory_t din = plan ? fft_gpu_alloc_bytes_hip(in_bytes) : NULL;
    fft_gpu_memory_t dout = plan ? fft_gpu_alloc_bytes_hip(out_bytes) : NULL;
    if (plan && din && dout) {
        if (fft_gpu_copy_h2d_bytes_hip(din, in, in_bytes) == 0 &&
            fft_gpu_execute_real2d_hip(plan, fft_gpu_memory_ptr(din), 0, fft_gpu_memory_ptr(dout), 0) == 0 && fft_gpu_plan_sync(plan) == 0 &&
            fft_gpu_copy_d2h_bytes_hip(out, dout, out_bytes) == 0)
            rc = 0;
    }
    fft_gpu_free(din);
    fft_gpu_free(dout);
    fft_gpu_destroy_plan(plan);
    return rc;
}

int fft_rfft2_gpu(const double* image, int rows, int cols, complex_t* out) {
    if (!image || !out || rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 30)) return -1;
    const size_t nr = (size_t)rows * (size_t)cols, ns = (size_t)rows * (size_t)(cols / 2 + 1);
    return run_real2d(image, nr * sizeof(double), out, ns * sizeof(complex_t), rows, cols, 1);
}

int fft_irfft2_gpu(const complex_t* spec, int rows, int cols, double* image) {
    if (!spec || !image || rows <= 0 || cols <= 0 || (long long)rows * cols > (1ll << 30)) return -1;
    const size_t nr = (size_t)rows * (size_t)cols, ns = (size_t)rows * (size_t)(cols / 2 + 1);
    return run_real2d(spec, ns * sizeof(complex_t), image, nr * sizeof(double), rows, cols, 0);
}

/* one DCT / DST plan (rows = 0: 1D of length cols) on host arrays of doubles, in place in one device buffer */
static int run_dct(const double* in, double* out, int rows, int cols, int type, int norm) {
    if (!in || !out || cols <= 0 || rows < 0 || type < 0 || type > 3 || norm < 0 || norm > 2 || (long long)(rows ? rows : 1) * cols > (1ll << 30)) return -1;
    if (ensure_gpu() != 0) return -1;
    int rc = -1;
    const size_t bytes = (size_t)(rows ? rows : 1) * (size_t)cols * sizeof(double);
    fft_gpu_plan_t plan = rows ? fft_gpu_plan_dct_2d_hip(rows, cols, 1, (fft_gpu_dct_t)type, (fft_gpu_dct_norm_t)norm, FFT_PREC_F64)
                               : fft_gpu_plan_dct_hip(cols, 1, (fft_gpu_dct_t)type, (fft_gpu_dct_norm_t)norm, FFT_PREC_F64);
    fft_gpu_memory_t buf = plan ? fft_gpu_alloc_bytes_hip(bytes) : NULL;
    if (plan && buf) {
        if (fft_gpu_copy_h2d_bytes_hip(buf, in, bytes) == 0 &&
            fft_gpu_execute_dct_hip(plan, fft_gpu_memory_ptr(buf), 0, fft_gpu_memory_ptr(buf), 0) == 0 && fft_gpu_plan_sync(plan) == 0 &&
            fft_gpu_copy_d2h_bytes_hip(out, buf, bytes) == 0)
            rc = 0;
    }
    fft_gpu_free(buf);
    fft_gpu_destroy_plan(plan);
    return rc;
}

int fft_dct_gpu(const double* x, int n, int type, int norm, double* out) { return run_dct(x, out, 0, n, type, norm); }

int fft_dct_2d_gpu(const double* image, int rows, int cols, int type, int norm, double* out) {
    if (rows <= 0) return -1;
    return run_dct(image, out, rows, cols, type, norm);
}
