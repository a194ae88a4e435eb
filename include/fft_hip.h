/*
 * fft_hip.h -- C ABI of the MI355X (gfx950) HIP FFT backend, and the
 * additive public entry points built on it.
 *
 * Part 1 is the drop-in boundary: the 13 backend functions the reference's
 * dispatcher expects of a backend -- the `extern` block of gpu/fft_gpu.c:32-46
 * (CUDA flavour; the functions being replaced live in gpu/fft_cuda.cu:53-252).
 * Plain C types only; opaque handles; no torch / HIP types in signatures
 * (streams travel as void*).  INTEGRATION.md shows the three-line patch that
 * binds the reference's own fft_gpu.c to these symbols.
 *
 * Part 2 is additive (nothing in the reference has these): fp32, batches with
 * 64-bit offsets, raw device pointers, streams, multi-device, algorithm
 * selection, the stand-alone bit-reversal permutation, HIP-event timing.
 */
#ifndef FFT_HIP_H
#define FFT_HIP_H

#include <stdint.h>
#include "fft_common.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef FFT_GPU_H
typedef struct fft_gpu_memory* fft_gpu_memory_t;
typedef struct fft_gpu_plan* fft_gpu_plan_t;
#endif

/* ------------------------------------------------------------------ part 1
 * Backend symbol set (replaces fft_gpu_*_cuda, gpu/fft_cuda.cu).          */
int fft_gpu_init_hip(void);               /* replaces fft_gpu_init_cuda        fft_cuda.cu:53-83   */
void fft_gpu_cleanup_hip(void);           /* replaces fft_gpu_cleanup_cuda     fft_cuda.cu:86-91   */
int fft_gpu_available_hip(void);          /* replaces fft_gpu_available_cuda   fft_cuda.cu:94-100  */
fft_gpu_memory_t fft_gpu_alloc_hip(size_t n_complex);                 /* fft_cuda.cu:103-115 */
void fft_gpu_free_hip(fft_gpu_memory_t mem);                          /* fft_cuda.cu:118-123 */
void fft_gpu_copy_h2d_hip(fft_gpu_memory_t dst, const complex_t* src, size_t n_complex); /* :126-129 */
void fft_gpu_copy_d2h_hip(complex_t* dst, fft_gpu_memory_t src, size_t n_complex);       /* :132-135 */
fft_gpu_plan_t fft_gpu_plan_1d_hip(int n, int batch, fft_direction dir);                 /* :138-163 */
/* `dir` is accepted for signature compatibility and IGNORED: the reference's
 * dispatcher hard-codes FFT_FORWARD there (gpu/fft_gpu.c:252); the plan's own
 * direction is used. */
void fft_gpu_execute_hip(fft_gpu_plan_t plan, fft_gpu_memory_t in, fft_gpu_memory_t out, fft_direction dir); /* :166-185 */
void fft_gpu_destroy_plan_hip(fft_gpu_plan_t plan);                   /* fft_cuda.cu:188-193 */
const char* fft_gpu_get_device_name_hip(void);                        /* fft_cuda.cu:196-206 */
void fft_gpu_get_memory_info_hip(size_t* total, size_t* available);   /* fft_cuda.cu:209-211 */
int fft_gpu_dft_1d_hip(complex_t* in, complex_t* out, int n, fft_direction dir); /* fft_cuda.cu:214-252 */

/* ------------------------------------------------------------------ part 2 */
typedef enum {
    FFT_PREC_F64 = 0, /* complex_t   : interleaved double (the reference's only type) */
    FFT_PREC_F32 = 1  /* complex32_t : interleaved float  (additive)                  */
} fft_precision_t;

/* Which butterfly family the power-of-two engine uses.  All compute the same
 * DFT (as radix4_fft / split_radix_fft / radix2_dit_fft do in the reference:
 * algorithms/core/radix4.c:98-125, split_radix.c:23-55 are radix-2 loops). */
typedef enum {
    FFT_GPU_ALGO_AUTO = 0,          /* fastest known schedule for the size               */
    FFT_GPU_ALGO_RADIX2 = 1,        /* LDS Stockham, radix-2 passes only                 */
    FFT_GPU_ALGO_RADIX4 = 2,        /* LDS Stockham, radix-4 passes (+ one radix-2)      */
    FFT_GPU_ALGO_SPLIT_RADIX = 3,   /* LDS Stockham, radix-8/16 passes with split-radix (L-shaped) codelets */
    FFT_GPU_ALGO_RADIX2_GLOBAL = 4, /* reference-shaped: bit-reversal permutation kernel + log2(n)
                                       in-place radix-2 DIT stage kernels in HBM (radix2_dit.c:70-112) */
    FFT_GPU_ALGO_BLUESTEIN = 5,     /* chirp-z even when n is a power of two (bluestein.c:79-155); every non-power-of-two
                                       n uses it whatever algo says, except a 7-smooth n planned with
                                       FFT_GPU_ALGO_MIXED_RADIX (or with AUTO under fft_gpu_set_smooth_policy_hip(1)) */
    FFT_GPU_ALGO_RADIX2_SHFL = 6,   /* reference-shaped radix-2 DIT held by one wavefront per transform: LDS
                                       bit-reversal permutation, in-register stages, __shfl_xor for the
                                       cross-lane strides (n = 128..1024; other n: FFT_GPU_ALGO_RADIX2) */
    FFT_GPU_ALGO_MIXED_RADIX = 7    /* direct Stockham mixed-radix (radix 2, 3, 4, 5, 7, 8 through LDS) for the 7-smooth
                                       n = 2^a 3^b 5^c 7^d <= 2^23: one pass up to 4096, two above; a power of two gets
                                       the plan AUTO builds, any other n chirp-z */
} fft_gpu_algo_t;

typedef struct {
    int n;              /* transform length */
    int batch;          /* transforms per execute */
    int direction;      /* -1 / +1 */
    int precision;      /* fft_precision_t */
    int algo;           /* fft_gpu_algo_t actually used */
    int device;         /* HIP device ordinal the plan lives on */
    int bluestein_m;    /* 0 for power-of-two n, else the padded length */
    int n_passes;       /* HBM round trips of the power-of-two engine (1, 2 or 3; log2n+1 for RADIX2_GLOBAL) */
    int factors[4];     /* length of the LDS-resident sub-transform of each pass */
    int chunk_batch;    /* transforms processed per launch group (Infinity-Cache blocking) */
    size_t workspace_bytes;
    int team_tiles;     /* 0: multi-pass schedule only.  1/2/4: the plan runs the one-round-trip team kernel (a whole
                           transform per XCD, this many 64 KiB tiles per workgroup); the multi-pass schedule
                           described by n_passes/factors is queued behind it as its fallback */
    int fused;          /* Bluestein and fused-consumer plans: 0 the element-wise steps run as kernels of their own, 1 they
                           ride on the first load / last store of the transforms, 2 and the forward transform's last pass and
                           the inverse's first pass are ONE kernel (2 * n_passes - 1 launches per group of chunk_batch), 3 the padded
                           transform fits one LDS tile and forward transform, product and inverse transform are ONE kernel */
    int team_kernel;    /* which one-round-trip kernel team_tiles refers to: 0 none, 1 team_fft_kernel (csrc/fft_team.h), 2
                           team_defer_kernel (csrc/fft_team_defer.h), 3 team_quad_kernel (csrc/fft_team_quad.h: whole-line row
                           segments, both steps decimated by 4, the exchange in four rounds through the XCD's L2) */
    /* r2c / c2r plans: algo ... team_kernel describe the complex core (length n/2 for even n, n for odd n); a core on the
       mixed-radix engine reports what the 1D mixed-radix plan of that length reports: algo = 7, bluestein_m = 0, n_passes
       1 or 2, factors its split; fused = 0 (the split / merge runs as a kernel of its own).
       2D plans: algo, chunk_batch, bluestein_m, team_* describe the row transforms (length cols): algo = 7 and
       bluestein_m = 0 when they run on the mixed-radix engine; n_passes and factors the strided column passes: 1 the
       direct column pass, 2 two strided passes, 0 the columns run on the transposed image -- every row count that is no
       power of two, on the mixed-radix engine where it is 7-smooth and the plan asks for it -- (or rows == 1: there are none).
       workspace_bytes includes the scratch images of two-pass mixed-radix cores. */
} fft_gpu_plan_info_t;

/* Per-plan switches (tests and integrators; nothing here changes results) */
typedef enum {
    FFT_GPU_OPT_TEAM_FORCE_FALLBACK = 1, /* 1: the team kernel behaves as if it could not form its XCD teams (status 1, nothing
                                            touched) and the multi-pass plan queued behind it does the work */
    FFT_GPU_OPT_TEAM_ENABLE = 2,         /* 0: run the multi-pass schedule only; 1: back to the team kernel where the plan has one */
    FFT_GPU_OPT_NO_FUSION = 3,           /* 1: Bluestein / fused-consumer plans run their element-wise steps as kernels of their own
                                            instead of fusing them into the FFT passes (same results to rounding; tests); frames plans
                                            run their per-signal fallback, inverse frames plans their merge kernel + plain inverse */
    FFT_GPU_OPT_NO_CHAIN = 4,            /* 1: Bluestein / fused-consumer plans keep the forward transform's last pass and the inverse
                                            transform's first pass as two kernels (by default they run as one where their tiles agree
                                            and the transform has >= 2^19 points; tests); 2: as one wherever the tiles agree (tools) */
    FFT_GPU_OPT_TEAM_NO_REPLAY = 5       /* 1: the caller does NOT keep the buffers of its asynchronous executes alive and unmodified until
                                            the next fft_gpu_plan_sync_hip (e.g. they come from a stream-ordered caching allocator): a team
                                            kernel timeout is then never repaired by repeating executes, fft_gpu_plan_sync_hip returns -1 */
} fft_gpu_plan_option_t;

/* Fused consumers of the transform (reference applications/convolution.c, applications/power_spectrum.c): FFT ->
 * element-wise -> inverse FFT with the zero padding, the spectral product and the truncation fused into the FFT passes. */
typedef enum {
    FFT_GPU_FUSED_CONV_LINEAR = 0,   /* y = x * h, x: nx, h: nh (fixed at plan time), y: nx + nh - 1   convolution.c:34-69   */
    FFT_GPU_FUSED_CONV_CIRCULAR = 1, /* y = x (*) h, all of length nx (a power of two)                   convolution.c:72-96   */
    FFT_GPU_FUSED_AUTOCORR = 2,      /* first nx lags of IFFT(|FFT(x, zero padded)|^2)                   power_spectrum.c:133-158 */
    FFT_GPU_FUSED_XCORR = 3,         /* first nx lags of IFFT(conj(FFT(x)) FFT(y))                       power_spectrum.c:161-190 */
    FFT_GPU_FUSED_PSD = 4            /* one-sided Hann periodogram, nx/2 + 1 REAL values (nx a power of two) power_spectrum.c:58-86 */
} fft_gpu_fused_t;

/* Short-time transforms on overlapping frames (reference applications/power_spectrum.c:87-130, welch_psd, and what it is the
 * segmented form of): frame w of a signal is its samples w * hop ... w * hop + n - 1, windowed and transformed. */
typedef enum { FFT_GPU_WINDOW_RECT = 0, FFT_GPU_WINDOW_HANN = 1, FFT_GPU_WINDOW_HAMMING = 2,
               FFT_GPU_WINDOW_BLACKMAN = 3, FFT_GPU_WINDOW_USER = 4 } fft_gpu_window_t; /* the reference's formulas, n - 1 denominators: power_spectrum.c:5-25 */
typedef enum { FFT_GPU_FRAMES_STFT = 0,    /* [S][nw][n] complex, unscaled */
               FFT_GPU_FRAMES_POWER = 1,   /* [S][nw][n/2 + 1] real: one periodogram per frame */
               FFT_GPU_FRAMES_WELCH = 2 }  /* [S][n/2 + 1] real: their mean over the frames */ fft_gpu_frames_out_t;
/* Two-signal statistics on the same frames (scipy's csd / coherence; what the reference's compute_coherence,
 * applications/power_spectrum.c:195-224, leaves as a placeholder): with X_w, Y_w the STFT rows of frame w of a pair (x, y),
 *     Pxx[k] = c_k mean_w |X_w[k]|^2,   Pyy[k] = c_k mean_w |Y_w[k]|^2,   Pxy[k] = c_k mean_w conj(X_w[k]) Y_w[k],
 * c_k = 1 / (sample_rate * P), doubled for 0 < k < n/2 (the POWER / WELCH scaling); hb = n/2 + 1 bins per pair. */
typedef enum { FFT_GPU_CROSS_CSD = 0,        /* [S][hb] complex: Pxy */
               FFT_GPU_CROSS_COHERENCE = 1,  /* [S][hb] real: |Pxy|^2 / (Pxx Pyy); exactly 0 where Pxx Pyy is not > 0 (power_spectrum.c:213-217) */
               FFT_GPU_CROSS_TRANSFER = 2,   /* [S][hb] complex: H1 = Pxy / Pxx; exactly (0, 0) where Pxx is not > 0 */
               FFT_GPU_CROSS_ALL = 3 }       /* [S][hb][4] reals: Pxx, Pyy, Re Pxy, Im Pxy */ fft_gpu_cross_out_t;

/* backend-level additive entry points */
int fft_gpu_device_count_hip(void);
int fft_gpu_set_device_hip(int device);
int fft_gpu_get_device_hip(void);
fft_gpu_memory_t fft_gpu_alloc_bytes_hip(size_t bytes);
int fft_gpu_copy_h2d_bytes_hip(fft_gpu_memory_t dst, const void* src, size_t bytes);
int fft_gpu_copy_d2h_bytes_hip(void* dst, fft_gpu_memory_t src, size_t bytes);
void* fft_gpu_memory_ptr_hip(fft_gpu_memory_t mem);
size_t fft_gpu_memory_bytes_hip(fft_gpu_memory_t mem);
/* page-lock / release a host array for the lifetime of a plan that borrows it (pinned H2D / D2H); 0 / -1 */
int fft_gpu_host_register_hip(void* host_ptr, size_t bytes);
int fft_gpu_host_unregister_hip(void* host_ptr);
int fft_gpu_host_is_registered_hip(const void* host_ptr); /* 1 page-locked and known to the runtime, 0 not */
/* the box's practical memory ceiling: best read + write rate (GB/s) of a plain 16-byte-per-lane device copy over `bytes`
 * bytes, a few launch shapes, `iters` launches each; -1 on failure */
double fft_gpu_copy_bench_hip(size_t bytes, int iters);
/* the same yardstick per direction: mode 0 copy (read + written bytes / s), 1 read-only stream, 2 write-only stream; the best of
 * several launch shapes with and without the non-temporal hint (copy: also an LDS-DMA tile copy in the engine's own shape), GB/s */
double fft_gpu_stream_bench_hip(size_t bytes, int iters, int mode);
/* resource counters of this process (tests): device allocations and streams the backend has created so far */
void fft_gpu_debug_counters_hip(long long* device_allocations, long long* streams_created);
/* FFT_MEASURE at the device level: time the plan's candidate schedules (team kernel vs multi-pass) on scratch buffers of
 * the plan's own size and keep the faster; returns 1 team kernel kept, 0 multi-pass kept / nothing to choose, -1 error */
int fft_gpu_plan_measure_hip(fft_gpu_plan_t plan, int iters);
fft_gpu_plan_t fft_gpu_plan_1d_ex_hip(int n, int batch, fft_direction dir, fft_precision_t prec, fft_gpu_algo_t algo);
/* 2D complex transforms of `n_matrices` row-major rows x cols matrices: rows = one batched 1D execute, columns = the
 * strided column pass of the four-step engine (or transpose + batched 1D); the inverse is scaled once by 1/(rows*cols).
 * Execute with fft_gpu_execute(_ptr/_async); in == out allowed.  fft_gpu_plan_2d_hip replaces the stub gpu/fft_gpu.c:377-385. */
fft_gpu_plan_t fft_gpu_plan_2d_hip(int rows, int cols, fft_direction dir);
fft_gpu_plan_t fft_gpu_plan_2d_ex_hip(int rows, int cols, int n_matrices, fft_direction dir, fft_precision_t prec);
/* 3D complex transforms of `n_volumes` row-major [depth][rows][cols] volumes (cols fastest, contiguous): numpy's fftn / ifftn over the
 * last three axes; the inverse is scaled once by 1 / (depth * rows * cols).  Execute with fft_gpu_execute(_ptr/_async); in == out allowed.
 * Where rows and cols are powers of two >= 8 and a plane fits the device's LDS together with a register prefetch of the next (on the MI355X
 * planes of up to 8192 values in fp32 and 4096 in fp64: every plane from 8 x 8 to 64 x 64 in both precisions) an execute is two launches and two HBM round trips: one kernel transforms whole
 * contiguous planes inside LDS, the depth transforms then run in place as strided column passes (depth a power of two) or on the
 * transposed volume in a workspace of the plan's own.  Every other shape >= 1 x 1 x 1, and FFT_GPU_OPT_NO_FUSION: the 2D plan on the
 * planes, then the same depth step.  AUTO only; 7-smooth lengths follow fft_gpu_set_smooth_policy_hip as fft_gpu_plan_2d_ex_hip's do.
 * fft_gpu_plan_info_hip: n = cols, batch = n_volumes, factors = {cols, rows, depth}, fused = 1 where the plane kernel runs,
 * n_passes = launches per execute (a chirp-z depth counts as an estimate).
 * NULL: a size < 1, depth * rows * cols > 2^30, rows * cols * n_volumes or depth * n_volumes * max(rows, cols) > 2^31 - 1, a failed allocation. */
fft_gpu_plan_t fft_gpu_plan_3d_hip(int depth, int rows, int cols, int n_volumes, fft_direction dir, fft_precision_t prec);
/* real-input forward / real-output inverse 1D transforms (reference stubs algorithms/auto/fft_auto.c:391-409): r2c reads
 * [batch][n] reals and writes [batch][n/2 + 1] complex bins; c2r the reverse, scaled by 1/n.  Execute with fft_gpu_execute_ptr. */
fft_gpu_plan_t fft_gpu_plan_r2c_1d_hip(int n, int batch, fft_precision_t prec);
fft_gpu_plan_t fft_gpu_plan_c2r_1d_hip(int n, int batch, fft_precision_t prec);
/* The same three with the algorithm named.  algo: FFT_GPU_ALGO_AUTO (what the entry points above pass: 7-smooth lengths
 * stay on chirp-z unless fft_gpu_set_smooth_policy_hip(1) is in force) or FFT_GPU_ALGO_MIXED_RADIX: every length of the
 * plan with fft_gpu_mixed_radix_passes_hip(length) > 0 that is no power of two runs on the mixed-radix engine; anything
 * else returns NULL.  2D decides rows and columns independently: 64 x 1000 keeps the power-of-two column pass and gets
 * mixed-radix rows, 1009 x 1000 keeps chirp-z columns on the transposed image; 7-smooth row counts run on the transposed
 * image with a mixed-radix plan (two passes above 4096 rows).  Real plans: the half-length (odd n: full-length) complex core; powers of two and other lengths get
 * the plan AUTO builds. */
fft_gpu_plan_t fft_gpu_plan_2d_algo_hip(int rows, int cols, int n_matrices, fft_direction dir, fft_precision_t prec, fft_gpu_algo_t algo);
fft_gpu_plan_t fft_gpu_plan_r2c_1d_algo_hip(int n, int batch, fft_precision_t prec, fft_gpu_algo_t algo);
fft_gpu_plan_t fft_gpu_plan_c2r_1d_algo_hip(int n, int batch, fft_precision_t prec, fft_gpu_algo_t algo);
/* fused consumers; h_host: the nh kernel samples (host memory, complex of `prec`) of the two convolutions, else ignored */
fft_gpu_plan_t fft_gpu_plan_fused_hip(fft_gpu_fused_t kind, int nx, int nh, const void* h_host, int batch, fft_precision_t prec);
int fft_gpu_fused_out_len_hip(fft_gpu_plan_t plan); /* elements per output row (complex; FFT_GPU_FUSED_PSD: real) */
/* async on the plan's stream.  d_x: [batch][nx] complex; d_y: the second signal of FFT_GPU_FUSED_XCORR, else NULL;
 * d_out: [batch][out_len]; sample_rate scales FFT_GPU_FUSED_PSD only */
int fft_gpu_execute_fused_hip(fft_gpu_plan_t plan, const void* d_x, const void* d_y, void* d_out, double sample_rate);
/* STFT, spectrogram and Welch PSD of n_signals complex signals of signal_len samples.  n: the frame length, a power of two >= 2;
 * 1 <= hop <= n; signal_len >= n; anything else returns NULL.  Every signal has nw = (signal_len - (n - hop)) / hop frames
 * (power_spectrum.c:92-93); no frame reaches past signal_len, trailing samples that fill no whole frame are ignored.
 * w_host: the n window values (host memory, reals of `prec`) of FFT_GPU_WINDOW_USER, else ignored.  POWER and WELCH rows are
 * |X[k]|^2 / (sample_rate * P), doubled for 0 < k < n/2 (power_spectrum.c:72-80), P = 0.375 n for the Hann window (the
 * reference's constant, as in FFT_GPU_FUSED_PSD) and sum w[i]^2 for every other window.  Where n fits one hooked pass the
 * frames are read in place by ONE launch (no [frames][n] copy), windowed on the way in, and POWER / WELCH rows leave that launch
 * as reals; WELCH adds the mean kernel (double accumulation, no atomics: bit-reproducible).  Every other n, and
 * FFT_GPU_OPT_NO_FUSION: one hooked execute per signal, a power kernel, the mean.  fft_gpu_plan_info_hip: n, batch = n_signals * nw,
 * the core's passes, fused = 1 when the framed load and the stores ride on the pass.  Sync, set_stream, destroy as for fused plans. */
fft_gpu_plan_t fft_gpu_plan_frames_hip(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window,
                                       const void* w_host /* n reals of prec, USER only */, fft_gpu_frames_out_t out, fft_precision_t prec);
/* The same for REAL signals, with one-sided rows: n_signals signals of signal_len REAL samples of `prec` (float / double), frame
 * w of a signal = its reals w * hop ... w * hop + n - 1; n: a power of two >= 4 (n = 2 returns NULL), hop, signal_len, window,
 * w_host and the POWER / WELCH scaling as above.  Rows: STFT [S][nw][n/2 + 1] complex, unscaled, bins 0 ... n/2 of the frame's
 * transform (DC and Nyquist bins have an imaginary part of exactly 0); POWER [S][nw][n/2 + 1] real; WELCH [S][n/2 + 1] real.
 * The transform behind a frame is ONE complex transform of length n/2 on the reals read as pairs; where n/2 fits one hooked pass
 * (n <= 8192 fp32, 4096 fp64) one launch reads the reals in place, windows them, transforms, splits the half-length spectrum
 * into the n/2 + 1 bins and stores the rows: no widened copy, half the loaded bytes.  16-byte loads are used where every frame starts
 * 16-byte aligned -- d_x 16-byte aligned, hop and signal_pitch multiples of 16 / sizeof(real) (4 fp32, 2 fp64) -- and reads
 * component by component otherwise (any hop, pitch and base a real allows).  Every other n, and FFT_GPU_OPT_NO_FUSION: a pack
 * kernel, the plain half-length transform, a split kernel, a power kernel.  fft_gpu_plan_info_hip: n = the frame length, batch =
 * n_signals * nw, passes / factors of the length-n/2 core, fused = 1 on the one-launch path.  Executed by
 * fft_gpu_execute_frames_hip with d_x real and signal_pitch in reals; fft_gpu_frames_count_hip, set_stream, sync, set_option and
 * destroy as for complex frames plans. */
fft_gpu_plan_t fft_gpu_plan_frames_real_hip(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window,
                                            const void* w_host /* n reals of prec, USER only */, fft_gpu_frames_out_t out, fft_precision_t prec);
int fft_gpu_frames_count_hip(fft_gpu_plan_t plan);   /* nw = (signal_len - (n - hop)) / hop; -1: not a frames plan */
/* async on the plan's stream.  d_x: complex signals, signal s at d_x + s * signal_pitch elements (0: signal_len; < signal_len: -1);
 * a plan of fft_gpu_plan_frames_real_hip reads d_x as reals and counts signal_pitch in reals;
 * d_out: see fft_gpu_frames_out_t; it must not overlap d_x (d_out == d_x returns -1); sample_rate scales POWER and WELCH only */
int fft_gpu_execute_frames_hip(fft_gpu_plan_t plan, const void* d_x, long long signal_pitch /* 0: signal_len */,
                               void* d_out, double sample_rate);
/* Inverse STFT of real signals by weighted overlap-add: the way back from fft_gpu_plan_frames_real_hip's STFT rows.  d_X holds
 * n_signals * n_frames one-sided rows of n/2 + 1 complex bins of `prec`, contiguous ([S][nw][n/2 + 1], exactly what the real
 * frames plan's STFT writes); the result is n_signals REAL signals of out_len = (n_frames - 1) * hop + n samples.  With
 * v_w = irfft_n(X[s][w]) -- scaled by 1/n, so that irfft(rfft(x)) = x like every inverse of the library; the imaginary parts of
 * bins 0 and n/2 are ignored, as numpy's irfft does -- and g the window (same kinds and formulas as the frames plans: one window
 * serves analysis and synthesis):
 *     env[t] = sum_w g[t - w hop]^2,    y[s][t] = (sum_w g[t - w hop] v_w[t - w hop]) / env[t]      (w: the frames that cover t)
 * the least-squares inverse: it returns x exactly for X = stft(x) wherever env[t] > 0.  1 / env is a plan-time table (long double).
 * Where env[t] <= 1e-10 max g^2 (scipy's istft constant; e.g. the two end samples under the symmetric Hann window) the sample cannot
 * be recovered and y[s][t] is written as exactly 0; fft_gpu_iframes_unrecoverable_hip counts those samples of one signal.
 * n: a power of two >= 4; 1 <= hop <= n; n_frames, n_signals >= 1; n_frames * n_signals <= 2^31 - 1 and frames * n <= 2^40; a USER
 * window needs w_host; anything else, or a failed allocation, returns NULL.  The transform behind a frame is ONE inverse complex
 * transform of length n/2; where that fits one hooked pass (n <= 8192 fp32, 4096 fp64; not n = 4) one launch reads the one-sided
 * rows, merges them on the way in and writes the [frames][n] real workspace (allocated at plan time).  Every other n, and
 * FFT_GPU_OPT_NO_FUSION: a merge kernel and the plain half-length inverse.  The overlap-add kernel (double accumulation, no atomics:
 * bit-reproducible) then writes every sample t < out_len of every signal and nothing else.  fft_gpu_plan_info_hip: n = the frame
 * length, batch = n_signals * n_frames, direction +1, passes / factors of the length-n/2 core, fused = 1 on the one-launch transform
 * path.  set_stream, sync, set_option and destroy as for frames plans. */
fft_gpu_plan_t fft_gpu_plan_iframes_real_hip(int n, int hop, int n_frames, int n_signals, fft_gpu_window_t window,
                                             const void* w_host /* n reals of prec, USER only */, fft_precision_t prec);
int fft_gpu_iframes_len_hip(fft_gpu_plan_t plan);            /* out_len; -1: not such a plan */
int fft_gpu_iframes_unrecoverable_hip(fft_gpu_plan_t plan);  /* samples per signal written as 0; -1: not such a plan */
/* async on the plan's stream.  d_X: the one-sided rows; d_y: the real signals, signal s at d_y + s * signal_pitch reals (0: out_len;
 * < out_len: -1); the signal_pitch - out_len reals between signals are never touched.  NULL pointers and d_X == d_y return -1;
 * nothing is launched then. */
int fft_gpu_execute_iframes_hip(fft_gpu_plan_t plan, const void* d_X, void* d_y, long long signal_pitch /* 0: out_len */);
/* Cross-spectral density, magnitude-squared coherence and H1 transfer estimate of n_signals PAIRS of signals of signal_len samples
 * (see fft_gpu_cross_out_t; the kind is fixed at plan time).  n, hop, signal_len, n_signals, window, w_host, nw and the limits are
 * those of fft_gpu_plan_frames_hip (complex signals, n >= 2) and fft_gpu_plan_frames_real_hip (real signals, n >= 4); anything else,
 * a bad kind or a failed allocation returns NULL.  The plan owns one frames plan in STFT mode, used unchanged -- its one-launch path
 * where it has one, its fallback where not or under FFT_GPU_OPT_NO_FUSION -- and runs it on x and on y into two row workspaces
 * allocated at plan time ([S * nw][n/2 + 1] complex for real signals, [S * nw][n] for complex ones, of which bins 0 .. n/2 are
 * read).  Two kernels reduce them: one thread per (pair, chunk of C frames, bin) sums |X|^2, |Y|^2 and conj(X) Y in double, frames
 * ascending; one thread per (pair, bin) sums the chunks ascending in double, scales by c_k / nw, forms the output kind in double and
 * rounds once.  No atomics: bit-reproducible, independent of the launch geometry; C is a function of (nw, n_signals, n) alone
 * (fft_gpu_cross_chunk_hip).  A zero-power bin gives 0 as stated above (a NaN is not zero power: it propagates to its pair's rows
 * and to no other pair's).  fft_gpu_plan_info_hip: n, batch = n_signals * nw, the inner core's passes, fused = the inner plan's,
 * chunk_batch = C.  fft_gpu_frames_count_hip, set_stream, sync, set_option and destroy as for frames plans. */
fft_gpu_plan_t fft_gpu_plan_cross_frames_hip(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window,
                                             const void* w_host /* n reals of prec, USER only */, fft_gpu_cross_out_t out, fft_precision_t prec);
fft_gpu_plan_t fft_gpu_plan_cross_frames_real_hip(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window,
                                                  const void* w_host /* n reals of prec, USER only */, fft_gpu_cross_out_t out, fft_precision_t prec);
int fft_gpu_cross_chunk_hip(fft_gpu_plan_t plan);    /* C, frames per chunk of the reduction; -1: not a cross frames plan */
/* async on the plan's stream.  d_x, d_y: the two signals of every pair, pair s at d_x + s * x_pitch and d_y + s * y_pitch elements
 * (reals for a real plan; 0: signal_len; < signal_len: -1).  d_x == d_y is legal.  d_out must overlap neither input.  NULL
 * pointers, short pitches and an overlapping output return -1; nothing is launched then. */
int fft_gpu_execute_cross_frames_hip(fft_gpu_plan_t plan, const void* d_x, long long x_pitch, const void* d_y, long long y_pitch,
                                     void* d_out, double sample_rate);
/* Overlap-save FIR filtering of n_signals long signals of signal_len complex samples with n_taps fixed complex taps (what the
 * reference's applications/fft_filtering.c is for, as a device plan).  The signals are cut into overlapping blocks of n samples (a
 * power of two > n_taps - 1; 0: the plan chooses min(nmax, max(256, next_pow2(4 n_taps))), nmax = 4096 fp32 / 2048 fp64, and
 * next_pow2(4 n_taps) for taps too long for that -- an unmeasured guess) that advance by B = n - (n_taps - 1); every block is
 * transformed, multiplied by FFT_n(taps) (computed once at plan time), transformed back, and its last B values go straight into
 * the output signal.  Where n fits one hooked pass (n <= nmax) that is ONE kernel launch and one round trip of the data: no
 * [blocks][n] copy in or out; fft_gpu_plan_info_hip then reports fused = 3.  Any other n, and FFT_GPU_OPT_NO_FUSION /
 * FFT_GPU_OPT_NO_CHAIN, take a gather kernel, the fused-convolution middle and a scatter kernel on bounded chunks of blocks
 * (fused = 2 / 1 / 0 by what the middle runs).  info: n = the block length, batch = n_signals * blocks per signal.
 * NULL: n_taps < 1, signal_len < 1, n_signals < 1, n not a power of two, n <= n_taps - 1, more than 2^31 - 1 blocks or output
 * samples, a failed allocation. */
typedef enum { FFT_GPU_FILTER_FULL = 0,     /* out_len = signal_len + n_taps - 1, np.convolve 'full'                    */
               FFT_GPU_FILTER_CAUSAL = 1,   /* out_len = signal_len, y[t] = sum_j h[j] x[t-j] (scipy lfilter(h, 1, x))  */
               FFT_GPU_FILTER_CENTRED = 2 } /* out_len = signal_len, full[(n_taps-1)/2 ...], np.convolve 'same'         */ fft_gpu_filter_out_t;
fft_gpu_plan_t fft_gpu_plan_filter_hip(int n_taps, const void* h_host /* n_taps complex of prec */, int signal_len, int n_signals,
                                       int n /* block length, power of two > n_taps - 1; 0: the plan chooses */,
                                       fft_gpu_filter_out_t out, fft_precision_t prec);
int fft_gpu_filter_out_len_hip(fft_gpu_plan_t plan);   /* -1: not a filter plan */
int fft_gpu_filter_block_hip(fft_gpu_plan_t plan);     /* n actually used; -1: not a filter plan */
/* async on the plan's stream.  Signal s is read at d_x + s * x_pitch and written at d_y + s * y_pitch (elements; 0: signal_len /
 * out_len); the elements between signals are neither read nor written.  -1, nothing launched: NULL pointers, a pitch smaller than
 * its row, d_y overlapping d_x (blocks re-read their neighbours' input: in place cannot work). */
int fft_gpu_execute_filter_hip(fft_gpu_plan_t plan, const void* d_x, long long x_pitch /* 0: signal_len */,
                               void* d_y, long long y_pitch /* 0: out_len */);
/* 2D convolution and frequency-domain filtering of n_matrices row-major rows x cols complex images with ONE kernel fixed at plan time:
 * out = IFFT2(FFT2(x zero padded to P x Q) . H).  The reference declares fft_convolution_2d and leaves a placeholder
 * (applications/convolution.c:99-109); applications/image_fft.c:147-235 masks the 2D spectrum of an image.  P = next_pow2(rows + krows - 1),
 * Q = next_pow2(cols + kcols - 1) for FULL / SAME / VALID; P = rows, Q = cols for CIRCULAR / SPECTRUM.  H is computed once at plan time (the
 * kernel placed in a [P][Q] array, circularly shifted by the mode's output offset, transformed on the device).  The result carries one
 * 1 / (P Q), like the 2D plans (the reference's fft_2d divides twice, image_fft.c:64-71).  Where the P rows of C columns fit one LDS tile
 * with row segments of at least 64 bytes (P >= 8) and the rows of length Q run with fused ends, an execute is three launches and three HBM
 * round trips of compact work images: row transforms of the rows image rows only, ONE kernel for forward columns . H . inverse columns,
 * row transforms of the out_rows wanted rows straight into d_y.  Everything else, and FFT_GPU_OPT_NO_FUSION: pad, forward 2D plan,
 * product, inverse 2D plan, crop -- five round trips of the padded image.  fft_gpu_plan_info_hip: n = Q, batch = n_matrices,
 * factors = {Q, P, Q}, n_passes = 3 / 5, fused = 1 / 0.  NULL: non-positive sizes, P Q > 2^30, VALID with a kernel larger than the image,
 * CIRCULAR / SPECTRUM with sizes that are no powers of two (CIRCULAR: a kernel larger than the image; SPECTRUM: krows != rows or
 * kcols != cols), a failed allocation. */
typedef enum { FFT_GPU_CONV2D_FULL = 0,      /* out (rows+krows-1) x (cols+kcols-1), scipy convolve2d 'full'          */
               FFT_GPU_CONV2D_SAME = 1,      /* out rows x cols = full[(krows-1)/2 ..][(kcols-1)/2 ..]                */
               FFT_GPU_CONV2D_VALID = 2,     /* out (rows-krows+1) x (cols-kcols+1); krows <= rows, kcols <= cols     */
               FFT_GPU_CONV2D_CIRCULAR = 3,  /* rows, cols powers of two; kernel krows <= rows, kcols <= cols, wraps  */
               FFT_GPU_CONV2D_SPECTRUM = 4   /* rows, cols powers of two; k_host IS H[rows][cols] in natural (unshifted)
                                                order, krows = rows, kcols = cols: out = IFFT2(FFT2(x) . H)           */
} fft_gpu_conv2d_t;
fft_gpu_plan_t fft_gpu_plan_conv2d_hip(int rows, int cols, int krows, int kcols, const void* k_host /* complex of prec, row-major */,
                                       int n_matrices, fft_gpu_conv2d_t mode, fft_precision_t prec);
int fft_gpu_conv2d_out_rows_hip(fft_gpu_plan_t plan);     /* -1: not such a plan */
int fft_gpu_conv2d_out_cols_hip(fft_gpu_plan_t plan);
int fft_gpu_conv2d_padded_rows_hip(fft_gpu_plan_t plan);  /* P */
int fft_gpu_conv2d_padded_cols_hip(fft_gpu_plan_t plan);  /* Q */
/* async on the plan's stream.  Matrix m is read at d_x + m * x_pitch and written at d_y + m * y_pitch (elements); the elements between
 * matrices are neither read nor written.  -1, nothing launched: NULL pointers, a pitch smaller than its matrix, d_y overlapping d_x. */
int fft_gpu_execute_conv2d_hip(fft_gpu_plan_t plan, const void* d_x, long long x_pitch /* elements between matrices, 0: rows*cols */,
                               void* d_y, long long y_pitch /* 0: out_rows*out_cols */);
/* Real 2D transforms of n_matrices row-major rows x cols real images, numpy's rfft2 / irfft2 (the reference's applications/image_fft.c
 * starts from real pixels and widens them to complex by hand).  r2c: X = rfft2(x), [rows][cols/2 + 1] complex per image, unscaled.  c2r:
 * x = irfft2(X, s = (rows, cols)): a full complex inverse transform along the columns of all cols/2 + 1 columns, then a c2r along the
 * rows (which ignores the imaginary parts of bins 0 and, for even cols, cols/2 of every row, like numpy.fft.irfft), scaled once by
 * 1 / (rows cols): irfft2(rfft2(x)) = x, and spectra that are not Hermitian-consistent give what numpy gives.  Where cols is a power of
 * two whose half fits one single-pass row transform with fused ends and rows is a power of two >= 8 whose columns fit one LDS tile with
 * row segments of at least 64 bytes, an execute is two launches on half-size data: the rows kernel (packed real load / r2c split, or
 * c2r merge / real store) and ONE column kernel over the cols/2 + 1 one-sided columns.  Everything else, and FFT_GPU_OPT_NO_FUSION: the
 * 1D real plan on the rows, transpose, a batched 1D plan of length rows, transpose.  fft_gpu_plan_info_hip: n = cols, batch =
 * n_matrices, factors = {cols, rows}, n_passes = 2 fused (else the fallback's steps: 4, or 1 for a single row), fused = 1 / 0.
 * NULL: non-positive sizes, rows cols > 2^30, rows n_matrices or cols n_matrices > 2^31 - 1, a failed allocation. */
fft_gpu_plan_t fft_gpu_plan_r2c_2d_hip(int rows, int cols, int n_matrices, fft_precision_t prec);
fft_gpu_plan_t fft_gpu_plan_c2r_2d_hip(int rows, int cols, int n_matrices, fft_precision_t prec);
int fft_gpu_real2d_bins_hip(fft_gpu_plan_t plan);  /* cols/2 + 1; -1: not such a plan */
/* async on the plan's stream.  r2c plans read reals at d_in + m * in_pitch and write complex values at d_out + m * out_pitch; c2r plans
 * the other way round.  Pitches count elements of their own side between matrices (0: dense: rows * cols reals, rows * (cols/2 + 1)
 * complex values); the rows of a matrix are dense; the elements between matrices are neither read nor written, and the input never is
 * written.  -1, nothing launched: NULL pointers, a plan of another kind, a pitch smaller than its matrix, d_out overlapping d_in. */
int fft_gpu_execute_real2d_hip(fft_gpu_plan_t plan, const void* d_in, long long in_pitch, void* d_out, long long out_pitch);
/* Cosine and sine transforms of types II and III of batched real rows, scipy.fft's conventions (the reference's applications/image_fft.c
 * names the DCT as the transform behind image compression and has none):
 *   DCT-II   X[k] = 2 sum_n x[n] cos(pi k (2n+1) / 2N)        DCT-III  y[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)
 *   DST-II   X[k] = 2 sum_n x[n] sin(pi (k+1)(2n+1) / 2N)     DST-III  y[n] = (-1)^n X[N-1] + 2 sum_{k<N-1} X[k] sin(pi (2n+1)(k+1) / 2N)
 * NORM_NONE: as above (scipy's norm=None).  NORM_INVERSE: times 1 / (2N), what scipy's idct / idst of the OTHER type apply: idct(X, type=2)
 * is DCT3 with NORM_INVERSE.  NORM_ORTHO: scipy's norm="ortho".  Where N is a power of two, 16 <= N <= 8192 in fp32 and 8 <= N <= 4096 in
 * fp64 on the MI355X, an execute is ONE launch that reads and writes every row once (Makhoul's algorithm on a half-length complex transform
 * inside the kernel); every other N >= 1, and FFT_GPU_OPT_NO_FUSION: a permute kernel, a length-N complex plan in a workspace of the plan's
 * own, a twiddle kernel.  fft_gpu_plan_info_hip: n = N, batch, the passes and factors of that core, fused = 1 / 0.
 * NULL: non-positive sizes, an unknown type or norm, n * batch > 2^31 - 1, a failed allocation. */
typedef enum { FFT_GPU_DCT2 = 0, FFT_GPU_DCT3 = 1, FFT_GPU_DST2 = 2, FFT_GPU_DST3 = 3 } fft_gpu_dct_t;
typedef enum { FFT_GPU_DCT_NORM_NONE = 0, FFT_GPU_DCT_NORM_INVERSE = 1, FFT_GPU_DCT_NORM_ORTHO = 2 } fft_gpu_dct_norm_t;
fft_gpu_plan_t fft_gpu_plan_dct_hip(int n, int batch, fft_gpu_dct_t type, fft_gpu_dct_norm_t norm, fft_precision_t prec);
/* the same type and norm along both axes of n_matrices row-major rows x cols real images: scipy's dctn / idctn over the last two axes.
 * A composition: the row plan, a real transpose, the row plan of length rows, a transpose back; fused = 1 where both row plans are.
 * NULL also: rows * cols > 2^30 or rows * cols * n_matrices > 2^31 - 1. */
fft_gpu_plan_t fft_gpu_plan_dct_2d_hip(int rows, int cols, int n_matrices, fft_gpu_dct_t type, fft_gpu_dct_norm_t norm, fft_precision_t prec);
/* async on the plan's stream.  Pitches count reals between rows (1D plans) or between matrices (2D plans, whose rows are dense); 0: dense.
 * Any sizeof(real)-aligned base and any pitch work; 16-byte aligned bases and pitches get 16-byte accesses.  d_in == d_out with equal
 * pitches is allowed.  -1, nothing launched: a NULL plan or pointer, a plan of another kind, a pitch smaller than the row or matrix. */
int fft_gpu_execute_dct_hip(fft_gpu_plan_t plan, const void* d_in, long long in_pitch, void* d_out, long long out_pitch);
int fft_gpu_plan_info_hip(fft_gpu_plan_t plan, fft_gpu_plan_info_t* info);
/* NULL = the plan's own (non-blocking) stream.  A caller that works on HIP's default stream -- PyTorch's default stream
 * has the handle 0 -- names it explicitly: (void*)1 = hipStreamLegacy, or its work and the plan's are not ordered. */
int fft_gpu_plan_set_stream_hip(fft_gpu_plan_t plan, void* hip_stream);
int fft_gpu_execute_ptr_hip(fft_gpu_plan_t plan, const void* d_in, void* d_out); /* async on the plan's stream */
/* Waits for the plan's stream.  0: every execute since the last sync holds valid results.  Should a team kernel's bounded wait
 * have run out (a member of a formed team stopped making progress: a hardware fault, not load -- formation under load falls back
 * BEFORE anything is touched), the team kernel is retired for this plan and the executes since the last sync are repeated on the
 * multi-pass schedule before this returns (still 0) -- WHERE THAT IS PROVABLY RIGHT: the plan is a plain 1D complex plan, and the
 * execute's input still holds the caller's data, i.e. it is out of place and no LATER execute since the last sync wrote into its
 * input (A -> B then B -> A: the second launch has overwritten A), or it is in place and ran from the plan's staged copy (the plan
 * stages the input of in-place executes until one sync has seen its team kernel end well, so the FIRST use of a plan on a device is
 * always repairable).  Contract for asynchronous callers: every buffer handed to fft_gpu_execute_ptr_hip stays allocated and
 * unmodified until the next sync (or set FFT_GPU_OPT_TEAM_NO_REPLAY).  -1: the stream failed, or a timeout hit an execute that
 * could not be repeated (stderr says how many): that data is invalid.  Bluestein, 2D, real and fused plans never repeat (their
 * cores transform the plan's own intermediates): a timeout in one of their cores is reported as -1.  (fft_gpu_execute() of
 * fft_gpu.h is void, as in the reference: gpu/fft_cuda.cu:166-185, and blocks: its buffers are the caller's for the duration.) */
int fft_gpu_plan_sync_hip(fft_gpu_plan_t plan);
int fft_gpu_plan_set_option_hip(fft_gpu_plan_t plan, fft_gpu_plan_option_t option, int value);
/* planner policy for plans created after the call; a negative argument keeps the current value.  team_mode: 0 never
 * the team kernel, 1 (default) where it measured faster than the multi-pass schedule, 2 every size it is built for;
 * team_min_batch: 0 = the measured batch crossover; chunk_mb: 0 = the default multi-pass launch-group size.
 * fft_gpu_init seeds them once from FFT_HIP_TEAM / FFT_HIP_TEAM_MIN_BATCH / FFT_HIP_CHUNK_MB. */
int fft_gpu_set_policy_hip(int team_mode, int team_min_batch, int chunk_mb);
/* what FFT_GPU_ALGO_MIXED_RADIX does with n: 0 not a mixed-radix length (not 7-smooth, above 2^23, n <= 0), 1 a single pass,
 * 2 two passes.  Host arithmetic only: works without a device. */
int fft_gpu_mixed_radix_passes_hip(int n);
/* which plan FFT_GPU_ALGO_AUTO builds for a non-power-of-two n (1D plans, and the rows, columns and cores of 2D, r2c and c2r
 * plans), for plans created after the call: 0 (default) chirp-z, 1 the
 * mixed-radix plan wherever fft_gpu_mixed_radix_passes_hip(n) > 0.  A negative argument changes nothing; returns the mode in
 * force.  fft_gpu_init seeds it once from FFT_HIP_SMOOTH. */
int fft_gpu_set_smooth_policy_hip(int mode);
/* syncs the plan's stream, then: 0 the last execute was done by the team kernel, 1 its XCD teams could not be
 * formed and the multi-pass fallback did the work, 2 a team barrier timed out (results invalid; plan_sync returns -1
 * too), -1 the plan has no team kernel or it has never been launched */
int fft_gpu_plan_team_status_hip(fft_gpu_plan_t plan);
/* profiling: every workgroup of the team kernel logs its 100 MHz clock at its first `events` timeline events into
 * d_trace[workgroup * events + i] (256 * events * 8 bytes of device memory owned by the caller); NULL switches it off.
 * team_quad_kernel keeps the last two slots for itself: [events - 2] = the workgroup's clock at kernel entry, [events - 1] =
 * (team << 8) | seat (tools/quad_trace.py) */
int fft_gpu_plan_team_trace_hip(fft_gpu_plan_t plan, void* d_trace, int events);
/* `iters` back-to-back executes bracketed by hipEvents recorded on the plan's stream */
int fft_gpu_execute_timed_hip(fft_gpu_plan_t plan, const void* d_in, void* d_out, int iters, float* elapsed_ms);
/* one execute with a HIP event after every pass launch: per-pass device milliseconds and launch counts */
int fft_gpu_profile_passes_hip(fft_gpu_plan_t plan, const void* d_in, void* d_out, float* ms, int* launches, int max_passes);
int fft_gpu_dft_1d_batch_hip(const void* in, void* out, int n, int batch, fft_direction dir, fft_precision_t prec);
/* out[b][bit_reverse(i)] = in[b][i]; in == out allowed (reference: the swap loop radix2_dit.c:70-77) */
int fft_gpu_bit_reverse_hip(const void* d_in, void* d_out, int n, int batch, fft_precision_t prec, void* hip_stream);

/* public additive API (dispatcher level; same style as fft_gpu.h) */
int fft_gpu_device_count(void);
fft_gpu_memory_t fft_gpu_alloc_f32(size_t n_complex32);
void fft_gpu_copy_h2d_f32(fft_gpu_memory_t dst, const complex32_t* src, size_t n);
void fft_gpu_copy_d2h_f32(complex32_t* dst, fft_gpu_memory_t src, size_t n);
void* fft_gpu_memory_ptr(fft_gpu_memory_t mem);
fft_gpu_plan_t fft_gpu_plan_1d_f32(int n, int batch, fft_direction direction);
fft_gpu_plan_t fft_gpu_plan_1d_ex(int n, int batch, fft_direction direction, fft_precision_t prec, fft_gpu_algo_t algo);
fft_gpu_plan_t fft_gpu_plan_2d_algo(int rows, int cols, int n_matrices, fft_direction direction, fft_precision_t prec, fft_gpu_algo_t algo);
int fft_gpu_plan_info(fft_gpu_plan_t plan, fft_gpu_plan_info_t* info);
int fft_gpu_plan_set_stream(fft_gpu_plan_t plan, void* hip_stream);
int fft_gpu_execute_async(fft_gpu_plan_t plan, fft_gpu_memory_t in, fft_gpu_memory_t out);
int fft_gpu_execute_ptr(fft_gpu_plan_t plan, const void* d_in, void* d_out);
int fft_gpu_plan_sync(fft_gpu_plan_t plan);
int fft_gpu_execute_timed(fft_gpu_plan_t plan, const void* d_in, void* d_out, int iters, float* elapsed_ms);
int fft_gpu_dft_1d_f32(complex32_t* in, complex32_t* out, int n, fft_direction direction);
int fft_gpu_dft_1d_batch_f32(complex32_t* in, complex32_t* out, int n, int batch, fft_direction direction);
int fft_gpu_bit_reverse(fft_gpu_memory_t in, fft_gpu_memory_t out, int n, int batch, fft_precision_t prec);
/* frames plans (fft_gpu_plan_frames_hip above) through the dispatcher */
fft_gpu_plan_t fft_gpu_plan_frames(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                   fft_gpu_frames_out_t out, fft_precision_t prec);
fft_gpu_plan_t fft_gpu_plan_frames_real(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                        fft_gpu_frames_out_t out, fft_precision_t prec);
int fft_gpu_frames_count(fft_gpu_plan_t plan);
int fft_gpu_execute_frames(fft_gpu_plan_t plan, const void* d_x, long long signal_pitch, void* d_out, double sample_rate);
/* inverse frames plans (fft_gpu_plan_iframes_real_hip above) through the dispatcher */
fft_gpu_plan_t fft_gpu_plan_iframes_real(int n, int hop, int n_frames, int n_signals, fft_gpu_window_t window, const void* w_host,
                                         fft_precision_t prec);
int fft_gpu_iframes_len(fft_gpu_plan_t plan);
int fft_gpu_iframes_unrecoverable(fft_gpu_plan_t plan);
int fft_gpu_execute_iframes(fft_gpu_plan_t plan, const void* d_X, void* d_y, long long signal_pitch);
/* cross frames plans (fft_gpu_plan_cross_frames_hip above) through the dispatcher */
fft_gpu_plan_t fft_gpu_plan_cross_frames(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                         fft_gpu_cross_out_t out, fft_precision_t prec);
fft_gpu_plan_t fft_gpu_plan_cross_frames_real(int n, int hop, int signal_len, int n_signals, fft_gpu_window_t window, const void* w_host,
                                              fft_gpu_cross_out_t out, fft_precision_t prec);
int fft_gpu_cross_chunk(fft_gpu_plan_t plan);
int fft_gpu_execute_cross_frames(fft_gpu_plan_t plan, const void* d_x, long long x_pitch, const void* d_y, long long y_pitch, void* d_out,
                                 double sample_rate);

#ifdef __cplusplus
}
#endif

#endif /* FFT_HIP_H */
