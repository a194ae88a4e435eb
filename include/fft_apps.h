/*
 * fft_apps.h -- the reference's FFT consumers, device-backed (additive; the reference keeps these functions inside
 * its applications/ demo programs, they are not part of its library).
 *
 * Same names, argument order and results as
 *   fft_convolution, circular_convolution      applications/convolution.c:34-96
 *   compute_periodogram, autocorrelation_fft,
 *   cross_correlation_fft                      applications/power_spectrum.c:58-86, 133-190
 *   welch_psd (here fft_welch_psd_gpu)         applications/power_spectrum.c:87-130
 *   design_fir_filter (fft_design_fir_filter_gpu) applications/fft_filtering.c:135-161
 * with a `_gpu` suffix, host arrays in and out, and int 0 / -1 (or NULL) instead of exit().  Each is ONE fused plan on the
 * device (fft_hip.h: fft_gpu_plan_fused_hip): forward transform, element-wise step and inverse transform, with the zero
 * padding, the spectral product and the truncation riding on the FFT passes.  Batched, device-resident use goes through
 * fft_gpu_plan_fused_hip / fft_gpu_execute_fused_hip directly.
 */
#ifndef FFT_APPS_H
#define FFT_APPS_H

#include "fft_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y[0 .. nx + nh - 2] = x * h (linear convolution); y has room for nx + nh - 1 values */
int fft_convolution_gpu(const complex_t* x, int nx, const complex_t* h, int nh, complex_t* y);
/* y = x (*) h, all of length n (a power of two, as in the reference) */
int circular_convolution_gpu(const complex_t* x, const complex_t* h, int n, complex_t* y);
/* one-sided Hann periodogram: a malloc'd array of n/2 + 1 doubles (n a power of two), freed by the caller; NULL on failure */
double* compute_periodogram_gpu(const complex_t* signal, int n, double sample_rate);
/* first n lags; a malloc'd (allocate_complex_array) array freed by the caller; NULL on failure */
complex_t* autocorrelation_fft_gpu(const complex_t* signal, int n);
complex_t* cross_correlation_fft_gpu(const complex_t* x, const complex_t* y, int n);
/* Welch's averaged Hann periodogram (welch_psd, applications/power_spectrum.c:87-130, its params struct flattened): windows of
 * window_size samples (a power of two) every window_size - overlap samples, 0 <= overlap < window_size <= signal_len; a malloc'd
 * array of window_size/2 + 1 doubles freed by the caller; NULL on failure.  ONE frames plan (fft_gpu_plan_frames_hip): the windows
 * are read in place on the device, nothing is copied per window. */
double* fft_welch_psd_gpu(const complex_t* signal, int signal_len, double sample_rate, int window_size, int overlap);
/* The same for a REAL signal (window_size a power of two >= 4): ONE real frames plan (fft_gpu_plan_frames_real_hip) reads the doubles
 * in place on the device, no complex copy of the signal is made anywhere. */
double* fft_welch_psd_real_gpu(const double* signal, int signal_len, double sample_rate, int window_size, int overlap);
/* Magnitude-squared coherence of two signals of n samples (compute_coherence, applications/power_spectrum.c:195-224: its signature,
 * its Hann window, overlap window_size / 2 and rate 1 -- and the coherence itself, |Pxy|^2 / (Pxx Pyy), where the reference writes a
 * placeholder of 1.0 for want of a cross spectrum; 0 where Pxx Pyy is not > 0, its own rule).  window_size a power of two >= 2,
 * <= n.  A malloc'd array of window_size/2 + 1 doubles freed by the caller; NULL on failure.  ONE cross frames plan
 * (fft_gpu_plan_cross_frames_hip). */
double* compute_coherence_gpu(const complex_t* x, const complex_t* y, int n, int window_size);
/* The same for REAL signals with a free overlap, 0 <= overlap < window_size (a power of two >= 4) <= n: ONE real cross frames plan
 * (fft_gpu_plan_cross_frames_real_hip), no complex copy of the signals. */
double* fft_coherence_real_gpu(const double* x, const double* y, int n, int window_size, int overlap);
/* Cross-spectral density Pxy = c_k mean_w conj(X_w) Y_w of two real signals (scipy's csd convention): pxy has room for
 * window_size/2 + 1 values.  0 / -1. */
int fft_csd_real_gpu(const double* x, const double* y, int n, double sample_rate, int window_size, int overlap, complex_t* pxy);
/* FIR filtering of a long signal: y[0 .. nx + nh - 2] = x * h, the results of fft_convolution_gpu, through ONE overlap-save filter
 * plan (fft_gpu_plan_filter_hip: blocks of a few thousand samples, one kernel launch) for any nx.  0 / -1. */
int fft_fir_filter_gpu(const complex_t* x, int nx, const complex_t* h, int nh, complex_t* y);
/* FIR design by frequency sampling (design_fir_filter, applications/fft_filtering.c:135-161, its params struct flattened): the
 * response of `type` (the reference's filter_type_t: 0 low-pass, 1 high-pass, 2 band-pass, 3 band-stop, 4 all-pass) sampled at
 * next_power_of_two(4 taps) points, with a raised-cosine transition of transition_width Hz for low-pass and high-pass only, its
 * inverse transform (on the device) shifted by taps / 2 and Hamming-windowed with the taps - 1 denominator.  taps >= 2.  A malloc'd
 * (allocate_complex_array) array of taps values freed by the caller; NULL on failure and without a device. */
complex_t* fft_design_fir_filter_gpu(int taps, int type, double cutoff_low, double cutoff_high, double sample_rate, double transition_width);
/* 2D linear convolution, the reference's fft_convolution_2d (applications/convolution.c:99-109, a placeholder there) with its signature:
 * image and kernel as arrays of row pointers, result rows of (cols + kcols - 1) values, (rows + krows - 1) of them, allocated by the
 * caller.  ONE 2D convolution plan (fft_gpu_plan_conv2d_hip, FULL).  0 / -1, -1 without a device. */
int fft_convolution_2d_gpu(complex_t** image, int rows, int cols, complex_t** kernel, int krows, int kcols, complex_t** result);
/* Frequency-domain filtering of a row-major rows x cols image (powers of two) with a mask in the CENTRED layout of the reference's
 * fft_shift_2d, DC at [rows/2][cols/2] -- what image_fft.c's ideal low-pass, Gaussian and edge-detection masks are written in
 * (applications/image_fft.c:147-235): out = IFFT2(FFT2(image) . unshift(H_centred)).  The mask is unshifted on the host and the plan runs
 * in SPECTRUM mode.  The result carries ONE 1 / (rows cols), like the 2D plans; the reference's fft_2d divides twice
 * (image_fft.c:64-71), so its filtered images are smaller by that factor.  0 / -1, -1 without a device. */
int fft_filter_2d_gpu(const complex_t* image, int rows, int cols, const complex_t* H_centred, complex_t* out);
/* 2D transform of a REAL row-major rows x cols image and its inverse, numpy's rfft2 / irfft2 (applications/image_fft.c:35-60 widens the
 * real pixels to complex by hand): out holds rows x (cols/2 + 1) bins, unscaled; fft_irfft2_gpu reads such a spectrum and writes the
 * rows x cols image, scaled by 1 / (rows cols), so that fft_irfft2_gpu(fft_rfft2_gpu(x)) = x.  Host pointers; ONE real 2D plan each
 * (fft_gpu_plan_r2c_2d_hip / fft_gpu_plan_c2r_2d_hip).  0 / -1, -1 without a device. */
int fft_rfft2_gpu(const double* image, int rows, int cols, complex_t* out);
int fft_irfft2_gpu(const complex_t* spec, int rows, int cols, double* image);
/* Cosine / sine transform of n doubles, and of a row-major rows x cols image along both axes (the transform behind image compression that
 * applications/image_fft.c points at): type = fft_gpu_dct_t (DCT-II, DCT-III, DST-II, DST-III), norm = fft_gpu_dct_norm_t, scipy.fft's
 * conventions (fft_hip.h).  Host pointers; ONE plan each (fft_gpu_plan_dct_hip / fft_gpu_plan_dct_2d_hip).  0 / -1, -1 without a device. */
int fft_dct_gpu(const double* x, int n, int type, int norm, double* out);
int fft_dct_2d_gpu(const double* image, int rows, int cols, int type, int norm, double* out);

#ifdef __cplusplus
}
#endif

#endif /* FFT_APPS_H */
