// fft_plans_ext.h -- plans built ON the batched 1D engine (fft_engine.h) for the "next" rows of the scope table
// (SURVEY.md 8f): 2D complex transforms, real-input / real-output 1D transforms, and the fused consumers of the
// reference's applications/ (FFT convolution, auto- / cross-correlation, periodogram; STFT, spectrogram and Welch PSD on
// overlapping frames, the inverse STFT by overlap-add, overlap-save FIR filtering, 2D convolution / spectrum filtering, the real 2D
// transforms rfft2 / irfft2, the cosine / sine transforms of types II and III, and 3D complex transforms).  Templated on the same runtime policy RT as the engine, so the
// unmodified source also runs in the CPU emulation (tests/emu).
#pragma once

#include "fft_engine.h"
#include "fft_kernels_ext.h"
#include "fft_kernels_conv2d.h"
#include "fft_kernels_real2d.h"
#include "fft_kernels_dct.h"
#include "fft_kernels_plane.h"

namespace ffteng {

// ---------------------------------------------------------------------------
// Batched complex 1D transform of ANY length with a fixed direction: the power-of-two engine or Bluestein -- or, where the
// caller asks for it (smooth), the mixed-radix plan for a 7-smooth length that is no power of two (what
// fft_gpu_plan_1d_ex_hip does with FFT_GPU_ALGO_MIXED_RADIX: a device whose LDS holds no such schedule gets chirp-z).
// ---------------------------------------------------------------------------
template <typename T, typename RT>
class AnyPlan {
  public:
    int n = 0, dir = -1;
    Pow2Plan<T, RT>* p2 = nullptr;
    BluesteinPlan<T, RT>* bl = nullptr;
    MixedRadixPlan<T, RT>* mr = nullptr;
    ~AnyPlan() { delete p2; delete bl; delete mr; }
    template <class F> void each_core(F&& f) {
        if (p2) p2->each_core(f);
        if (bl) bl->each_core(f);
    }
    bool build(RT* rt, int n_, int dir_, int batch, int algo = ALGO_AUTO, bool smooth = false) {
        n = n_;
        dir = dir_ < 0 ? -1 : 1;
        if (n >= 1 && (n & (n - 1)) == 0) {
            p2 = new Pow2Plan<T, RT>();
            return p2->build(rt, ilog2(n), algo, batch);
        }
        if (n < 1 || n > (1 << 29)) return false;
        if (smooth && mr_passes(n) > 0) {
            mr = new MixedRadixPlan<T, RT>();
            if (mr->build(rt, n, batch)) return true;
            delete mr;
            mr = nullptr;
        }
        bl = new BluesteinPlan<T, RT>();
        return bl->build(rt, n, dir, algo, batch);
    }
    void execute(const cpx<T>* in, cpx<T>* out, int nb) {
        if (p2) p2->execute(in, out, nb, dir > 0);
        else if (mr) mr->execute(in, out, nb, dir > 0);
        else if (bl) bl->execute(in, out, nb);
    }
};

template <typename RT, class K, class... A>
static void launch_flat(RT* rt, K kernel, long long total, A... args) {
    long long g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    if (g < 1) g = 1;
    rt->launch(kernel, g, 256, (size_t)0, args...);
}

// ---------------------------------------------------------------------------
// 2D complex transform of row-major rows x cols matrices (reference: stubs fft_auto.c:411-415 / fft_gpu.c:377-394; CPU
// model applications/image_fft.c:35-60).  Row-column decomposition on the batched engine:
//   rows    = ONE batched 1D execute (n = cols, batch = rows * matrices);
//   columns = a strided batch: the column pass of the four-step engine in place (rows a power of two that fits one
//             LDS tile with >= 64-byte row segments, cols a multiple of the 16-byte lane access), the same transforms as two
//             strided passes with wide tiles for more rows, otherwise transpose -> batched 1D -> transpose.
// smooth (FFT_GPU_ALGO_MIXED_RADIX, or AUTO under the smooth policy): 7-smooth lengths that are no power of two run on the
// mixed-radix engine, each dimension decided on its own -- the rows through AnyPlan, the columns of a row count that is no
// power of two through AnyPlan on the transposed image (power-of-two row counts keep their strided column passes).
// The inverse is scaled ONCE by 1 / (rows * cols): each 1D inverse carries its own 1 / length and nothing is applied on
// top (the reference's image_fft.c:64-71 divides by rows * cols AGAIN after two already scaled 1D inverses).
// ---------------------------------------------------------------------------
template <typename T, typename RT>
class Plan2D {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    RT* rt = nullptr;
    int rows = 0, cols = 0, dir = -1, max_matrices = 1;
    AnyPlan<T, RT> rowp;
    Pow2Plan<T, RT>* colp = nullptr;      // direct column pass
    AnyPlan<T, RT>* colt = nullptr;       // or: batched 1D on the transposed image
    cpx<T>* tbuf = nullptr;               // transposed image (transpose path)
    bool ok = false;
    ~Plan2D() {
        delete colp;
        delete colt;
        if (rt && tbuf) rt->dfree(tbuf);
    }
    template <class F> void each_core(F&& f) {
        rowp.each_core(f);
        if (colp) f(colp);
        if (colt) colt->each_core(f);
    }
    bool build(RT* runtime, int rows_, int cols_, int dir_, int n_matrices, bool smooth = false) {
        rt = runtime; rows = rows_; cols = cols_; dir = dir_ < 0 ? -1 : 1; max_matrices = n_matrices;
        if (rows < 1 || cols < 1 || n_matrices < 1 || (long long)rows * cols > (1ll << 30) ||
            (long long)rows * n_matrices > 0x7fffffff || (long long)cols * n_matrices > 0x7fffffff) return false;
        if (!rowp.build(rt, cols, dir, rows * n_matrices, ALGO_AUTO, smooth)) return false;
        if (rows > 1) {
            if ((rows & (rows - 1)) == 0) {
                colp = new Pow2Plan<T, RT>();
                if (!colp->build_columns(rt, ilog2(rows), cols, n_matrices)) { delete colp; colp = nullptr; }
                // many rows: the one-pass column tile (rows x C columns in LDS) gets narrow (C = 2 at 4096 rows fp32: 16-byte row
                // segments) or does not fit at all -- the four-step split of the column transforms keeps whole lines
                // (build_columns2; measured profiles/r2_ext_plans.txt)
                static const int min_seg = FFT_EXP_ENV("FFT_HIP_COL2_MINSEG") ? atoi(FFT_EXP_ENV("FFT_HIP_COL2_MINSEG")) : 64;
                if (!colp || colp->passes[0].seg_bytes < min_seg) {
                    Pow2Plan<T, RT>* two = new Pow2Plan<T, RT>();
                    if (two->build_columns2(rt, ilog2(rows), cols, n_matrices)) {
                        delete colp;
                        colp = two;
                    } else {
                        delete two;
                    }
                }
            }
            if (!colp) {
                colt = new AnyPlan<T, RT>();
                if (!colt->build(rt, rows, dir, cols * n_matrices, ALGO_AUTO, smooth)) return false;
                tbuf = (cpx<T>*)rt->dmalloc((size_t)rows * cols * n_matrices * SZ);
                if (!tbuf) return false;
            }
        }
        ok = true;
        return true;
    }
    void execute(const cpx<T>* in, cpx<T>* out, int nm) {
        rowp.execute(in, out, rows * nm);
        if (rows == 1) return;
        if (colp) {
            colp->execute(out, out, nm, dir > 0);
            return;
        }
        const long long tiles = (long long)nm * ((rows + 31) / 32) * ((cols + 31) / 32);
        long long grid = tiles > 65536 ? 65536 : tiles;
        rt->launch(fftk::transpose_kernel<T>, grid, 256, (size_t)(32 * 33 * SZ), (const cpx<T>*)out, tbuf, rows, cols, tiles);
        colt->execute(tbuf, tbuf, cols * nm);
        rt->launch(fftk::transpose_kernel<T>, grid, 256, (size_t)(32 * 33 * SZ), (const cpx<T>*)tbuf, out, cols, rows, tiles);
    }
};

// ---------------------------------------------------------------------------
// Real-input forward (r2c) and real-output inverse (c2r) 1D transforms, n/2 + 1 bins (reference include/fft_auto.h:88-106;
// its r2c "implementation" copies into a temporary, plans on it and frees it -- a use-after-free, fft_auto.c:391-402 --
// and c2r returns NULL).  Even n: ONE complex transform of length n/2 on the real array read as complex, plus a split /
// merge kernel (fft_kernels_ext.h); odd n: promoted to a complex transform of length n.  c2r is scaled by 1/n like every
// inverse of the library, so c2r(r2c(x)) = x.  smooth: a 7-smooth half length (odd n: length) that is no power of two runs on
// the mixed-radix engine; the split / merge / promote / extend kernels are the same.
// ---------------------------------------------------------------------------
template <typename T, typename RT>
class RealPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    RT* rt = nullptr;
    int n = 0, h = 0, max_batch = 1;
    bool forward = true;  // r2c
    AnyPlan<T, RT> core;
    cpx<T>* w = nullptr;     // W_n^k, k <= n/2 (even n)
    cpx<T>* work = nullptr;  // [batch][n/2] (even n) or [batch][n] (odd n)
    bool ok = false;
    ~RealPlan() {
        if (rt && w) rt->dfree(w);
        if (rt && work) rt->dfree(work);
    }
    template <class F> void each_core(F&& f) { core.each_core(f); }
    bool even() const { return (n & 1) == 0; }
    bool build(RT* runtime, int n_, bool r2c, int batch, bool smooth = false) {
        rt = runtime; n = n_; forward = r2c; max_batch = batch; h = n / 2;
        if (n < 1 || batch < 1) return false;
        if (even()) {
            if (!core.build(rt, h, r2c ? -1 : 1, batch, ALGO_AUTO, smooth)) return false;
            std::vector<cpx<T>> t;
            make_twiddle_table<T>(t, n, (long long)h + 1, 1);
            w = (cpx<T>*)rt->dmalloc(t.size() * SZ);
            work = (cpx<T>*)rt->dmalloc((size_t)batch * (size_t)h * SZ);
            if (!w || !work) return false;
            rt->h2d(w, t.data(), t.size() * SZ);
        } else {
            if (!core.build(rt, n, r2c ? -1 : 1, batch, ALGO_AUTO, smooth)) return false;
            work = (cpx<T>*)rt->dmalloc((size_t)batch * (size_t)n * SZ);
            if (!work) return false;
        }
        ok = true;
        return true;
    }
    // r2c: x real [nb][n] -> X complex [nb][n/2 + 1]
    void execute_r2c(const T* x, cpx<T>* X, int nb) {
        if (even()) {
            core.execute(reinterpret_cast<const cpx<T>*>(x), work, nb);
            launch_flat(rt, fftk::r2c_split_kernel<T>, (long long)nb * (h / 2 + 1), (const cpx<T>*)work, X, (const cpx<T>*)w, h, (long long)nb * (h / 2 + 1));
        } else {
            launch_flat(rt, fftk::real_to_complex_kernel<T>, (long long)nb * n, x, work, (long long)nb * n);
            core.execute(work, work, nb);
            launch_flat(rt, fftk::copy_rows_kernel<T>, (long long)nb * (h + 1), (const cpx<T>*)work, X, n, h + 1, (long long)nb * (h + 1));
        }
    }
    // c2r: X complex [nb][n/2 + 1] (Hermitian half) -> x real [nb][n], scaled by 1/n
    void execute_c2r(const cpx<T>* X, T* x, int nb) {
        if (even()) {
            launch_flat(rt, fftk::c2r_merge_kernel<T>, (long long)nb * (h / 2 + 1), X, work, (const cpx<T>*)w, h, (long long)nb * (h / 2 + 1));
            core.execute(work, reinterpret_cast<cpx<T>*>(x), nb);
        } else {
            launch_flat(rt, fftk::hermitian_extend_kernel<T>, (long long)nb * n, X, work, n, (long long)nb * n);
            core.execute(work, work, nb);
            launch_flat(rt, fftk::complex_to_real_kernel<T>, (long long)nb * n, (const cpx<T>*)work, x, (long long)nb * n);
        }
    }
};

// ---------------------------------------------------------------------------
// Fused consumers (reference applications/convolution.c:34-96, applications/power_spectrum.c:58-80, 133-190): every one
// is FFT -> element-wise -> (inverse FFT), the shape of Bluestein's inner loop, and uses the same pass hooks
// (fftk::TileHooks): the zero padding happens in the first load (the padding is never read), the spectral product in
// the forward transform's last store, the truncation in the inverse transform's last store.
//   CONV_LINEAR    y[b] = x[b] * h          x: [batch][nx], h: [nh] fixed at plan time, y: [batch][nx + nh - 1]; m = next_pow2(ny)
//   CONV_CIRCULAR  y[b] = x[b] (*) h        all of length n (a power of two, like the reference's radix-2 path)
//   AUTOCORR       acf[b] = IFFT(|FFT(x[b] zero padded to m)|^2), first n;  m = next_pow2(2 n)
//   XCORR          ccf[b] = IFFT(conj(FFT(x[b])) FFT(y[b])), first n;       m = next_pow2(2 n)
//   PSD            one-sided periodogram of Hann-windowed x[b]: [batch][n/2 + 1] real
// ---------------------------------------------------------------------------
enum FusedKind { FUSED_CONV_LINEAR = 0, FUSED_CONV_CIRCULAR = 1, FUSED_AUTOCORR = 2, FUSED_XCORR = 3, FUSED_PSD = 4 };
enum FramesWindow { WINDOW_RECT = 0, WINDOW_HANN = 1, WINDOW_HAMMING = 2, WINDOW_BLACKMAN = 3, WINDOW_USER = 4 };

// The windows of the periodogram and the frames plans: the reference's formulas with their n - 1 denominators
// (power_spectrum.c:5-25), n values in long double; every caller rounds them to T and packs them its own way.  A window of one
// sample is 1, not 0 / 0.  w_host: the n values of WINDOW_USER, unused otherwise
template <typename T>
static std::vector<long double> window_values(int window, int n, const T* w_host) {
    std::vector<long double> w((size_t)n, 1.0L);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int i = 0; i < n; i++) {
        if (window == WINDOW_USER) w[(size_t)i] = (long double)w_host[i];
        if (window == WINDOW_USER || window == WINDOW_RECT || n == 1) continue;
        const long double a = two_pi * (long double)i / (long double)(n - 1);
        if (window == WINDOW_HANN) w[(size_t)i] = 0.5L * (1.0L - cosl(a));
        else if (window == WINDOW_HAMMING) w[(size_t)i] = 0.54L - 0.46L * cosl(a);
        else if (window == WINDOW_BLACKMAN) w[(size_t)i] = 0.42L - 0.5L * cosl(a) + 0.08L * cosl(2.0L * a);
    }
    return w;
}

// The spectrum of a kernel fixed at plan time: its nh values zero padded to the core's length m, uploaded and transformed once by
// the plan's own core.  nullptr: no device memory
template <typename T, typename RT>
static cpx<T>* kernel_spectrum(RT* rt, Pow2Plan<T, RT>& core, const cpx<T>* h_host, int nh, long long m) {
    std::vector<cpx<T>> hp((size_t)m);
    for (auto& z : hp) { z.re = 0; z.im = 0; }
    for (int i = 0; i < nh; i++) hp[(size_t)i] = h_host[i];
    cpx<T>* H = (cpx<T>*)rt->dmalloc((size_t)m * sizeof(cpx<T>));
    if (!H) return nullptr;
    rt->h2d(H, hp.data(), (size_t)m * sizeof(cpx<T>));
    core.execute(H, H, 1, false);
    return H;
}

template <typename T, typename RT>
class FusedPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    RT* rt = nullptr;
    int kind = 0, nx = 0, nh = 0, ny = 0, log2m = 0, max_batch = 1;
    Pow2Plan<T, RT> core;
    cpx<T>* H = nullptr;      // FFT_m(h) (convolutions) or the window as complex values (PSD)
    cpx<T>* work = nullptr;   // [batch][m]
    cpx<T>* work2 = nullptr;  // [batch][m] (XCORR: the spectrum of x)
    bool ok = false;
    bool no_fusion = false;   // tests: element-wise steps as kernels of their own
    bool no_chain = false;    // tests: forward-last and inverse-first pass as two kernels
    ~FusedPlan() {
        if (!rt) return;
        rt->dfree(H); rt->dfree(work); rt->dfree(work2);
    }
    template <class F> void each_core(F&& f) { f(&core); }
    void set_no_fusion(bool v) { no_fusion = v; }
    void set_no_chain(int v) { no_chain = v == 1; core.set_chain_rule(v == 2); }  // (BluesteinPlan::set_no_chain)
    long long m() const { return 1ll << log2m; }
    int out_len() const { return kind == FUSED_PSD ? nx / 2 + 1 : ny; }

    // h_host: nh kernel samples (CONV_*); ignored otherwise
    bool build(RT* runtime, int kind_, int nx_, int nh_, const cpx<T>* h_host, int batch) {
        rt = runtime; kind = kind_; nx = nx_; nh = nh_; max_batch = batch;
        if (nx < 1 || batch < 1) return false;
        long long mm = 1;
        switch (kind) {
            case FUSED_CONV_LINEAR:
                if (nh < 1 || !h_host) return false;
                ny = nx + nh - 1;
                while (mm < ny) mm <<= 1;
                break;
            case FUSED_CONV_CIRCULAR:
                if (!h_host || (nx & (nx - 1)) != 0) return false;
                nh = nx; ny = nx; mm = nx;
                break;
            case FUSED_AUTOCORR:
            case FUSED_XCORR:
                ny = nx;
                while (mm < 2ll * nx) mm <<= 1;
                break;
            case FUSED_PSD:
                if ((nx & (nx - 1)) != 0) return false;
                ny = nx; mm = nx;
                break;
            default: return false;
        }
        if (mm > (1ll << 29)) return false;
        log2m = ilog2(mm);
        core.prefer_chain = kind != FUSED_PSD;  // forward + inverse back to back (the periodogram has no inverse)
        core.wants_hooks = true;
        if (!core.build(rt, log2m, ALGO_AUTO, batch)) return false;
        work = (cpx<T>*)rt->dmalloc((size_t)batch * (size_t)mm * SZ);
        if (!work) return false;
        if (kind == FUSED_XCORR) {
            work2 = (cpx<T>*)rt->dmalloc((size_t)batch * (size_t)mm * SZ);
            if (!work2) return false;
        }
        if (kind == FUSED_CONV_LINEAR || kind == FUSED_CONV_CIRCULAR) {
            H = kernel_spectrum(rt, core, h_host, nh, mm);
            if (!H) return false;
        } else if (kind == FUSED_PSD) {
            // the Hann window as complex values; + 1 padding entry
            std::vector<cpx<T>> wv((size_t)nx + 1);
            const std::vector<long double> hann = window_values<T>(WINDOW_HANN, nx, nullptr);
            for (int i = 0; i < nx; i++) {
                wv[(size_t)i].re = (T)hann[(size_t)i];
                wv[(size_t)i].im = 0;
            }
            wv[(size_t)nx] = wv[0];
            H = (cpx<T>*)rt->dmalloc(wv.size() * SZ);
            if (!H) return false;
            rt->h2d(H, wv.data(), wv.size() * SZ);
        }
        ok = true;
        return true;
    }

    bool fused() const { return core.hook_capable() && !no_fusion; }

    // forward transform of `in` (rows of n_in valid samples, pitch in_pitch), zero padded to m, into dst (pitch m); the
    // spectrum is multiplied by tab / conj(tab) / replaced by |.|^2 on the way out; optional load-side table
    void forward(const cpx<T>* in, long long in_pitch, int n_in, const cpx<T>* pre, cpx<T>* dst, const cpx<T>* tab, long long tab_b,
                 int post_mode, int nb) {
        const long long mm = m();
        if (fused()) {
            ExecHooks<T> f;
            f.pre_tab = pre; f.pre_mode = pre ? fftk::HOOK_MUL : fftk::HOOK_NONE;
            f.n_in = n_in; f.in_pitch = in_pitch;
            f.post_tab = tab; f.post_tab_b = tab_b; f.post_mode = post_mode;
            core.execute_hooked(in, dst, nb, false, f);
            return;
        }
        const unsigned per_block = 256 * BLU_PER_THREAD;
        const unsigned bpr = (unsigned)((mm + per_block - 1) / per_block);
        rt->launch(fftk::pad_mul_kernel<T>, (long long)bpr * nb, 256, (size_t)0, in, in_pitch, n_in, pre,
                   (int)(pre ? fftk::HOOK_MUL : fftk::HOOK_NONE), dst, (int)mm, bpr);
        core.execute(dst, dst, nb, false);
        if (post_mode != fftk::HOOK_NONE)
            rt->launch(fftk::mul_store_kernel<T>, (long long)bpr * nb, 256, (size_t)0, (const cpx<T>*)dst, mm, tab, tab_b, post_mode, dst, mm,
                       (int)mm, (T)1, bpr);
    }
    // inverse transform of `src` (pitch m), first n_out values of every row into out (pitch out_pitch)
    void inverse(cpx<T>* src, cpx<T>* out, long long out_pitch, int n_out, int nb) {
        const long long mm = m();
        if (fused()) {
            ExecHooks<T> g;
            g.n_out = n_out; g.out_pitch = out_pitch;
            core.execute_hooked(src, out, nb, true, g);
            return;
        }
        core.execute(src, src, nb, true);
        const unsigned per_block = 256 * BLU_PER_THREAD;
        const unsigned bpr = (unsigned)(((long long)n_out + per_block - 1) / per_block);
        rt->launch(fftk::mul_store_kernel<T>, (long long)bpr * nb, 256, (size_t)0, (const cpx<T>*)src, mm, (const cpx<T>*)nullptr, 0ll,
                   (int)fftk::HOOK_NONE, out, out_pitch, n_out, (T)1, bpr);
    }

    // forward + spectral product + inverse in one go; the middle of it as ONE kernel where the plan allows (execute_chain)
    void forward_inverse(const cpx<T>* in, int n_in, const cpx<T>* tab, long long tab_b, int post_mode, cpx<T>* out, int n_out, int nb) {
        if (fused() && !no_chain && core.round_capable() && tab_b == 0) {  // the padded transform fits one tile: ONE kernel
            ExecHooks<T> rr;
            rr.n_in = n_in; rr.in_pitch = n_in;
            rr.mid_tab = tab; rr.mid_mode = post_mode;
            rr.n_out = n_out; rr.out_pitch = n_out;
            core.execute_round(in, out, nb, rr);
            return;
        }
        if (fused() && !no_chain && core.chain_capable()) {
            ExecHooks<T> f, g;
            f.n_in = n_in; f.in_pitch = n_in;
            f.post_tab = tab; f.post_tab_b = tab_b; f.post_mode = post_mode;
            g.n_out = n_out; g.out_pitch = n_out;
            if (core.execute_chain(in, out, nb, f, g)) return;
        }
        forward(in, n_in, n_in, nullptr, work, tab, tab_b, post_mode, nb);
        inverse(work, out, n_out, n_out, nb);
    }

    // x: [nb][nx]; y: second input of XCORR ([nb][nx]), else unused; out: [nb][out_len()] complex
    // (PSD: out is [nb][nx/2 + 1] REAL values of type T, sample_rate scales it)
    void execute(const cpx<T>* x, const cpx<T>* y, void* out, int nb, T sample_rate = (T)1) {
        switch (kind) {
            case FUSED_CONV_LINEAR:
            case FUSED_CONV_CIRCULAR:
                forward_inverse(x, nx, H, 0, fftk::HOOK_MUL, (cpx<T>*)out, ny, nb);
                break;
            case FUSED_AUTOCORR:
                forward_inverse(x, nx, nullptr, 0, fftk::HOOK_ABS2, (cpx<T>*)out, ny, nb);
                break;
            case FUSED_XCORR:
                forward(x, nx, nx, nullptr, work2, nullptr, 0, fftk::HOOK_NONE, nb);                    // X
                forward_inverse(y, nx, work2, m(), fftk::HOOK_MUL_CONJ, (cpx<T>*)out, ny, nb);           // IFFT(Y conj(X))
                break;
            case FUSED_PSD: {
                forward(x, nx, nx, H, work, nullptr, 0, fftk::HOOK_NONE, nb);
                const T scale = (T)(1.0L / ((long double)sample_rate * 0.375L * (long double)nx));  // Hann window power (power_spectrum.c:70-71)
                launch_flat(rt, fftk::psd_onesided_kernel<T>, (long long)nb * (nx / 2 + 1), (const cpx<T>*)work, (T*)out, nx, scale,
                            (long long)nb * (nx / 2 + 1));
                break;
            }
            default: break;
        }
    }
};

// ---------------------------------------------------------------------------
// Short-time transforms on overlapping frames: the STFT, the spectrogram (one periodogram per frame) and Welch's averaged
// periodogram (reference applications/power_spectrum.c:87-130, welch_psd; windows :5-25, periodogram scaling :70-80).
//   x: [n_signals] complex signals of signal_len samples, signal s at x + s * signal_pitch;
//   frame w of a signal = its samples w * hop ... w * hop + n - 1, w < nw = (signal_len - (n - hop)) / hop (:92-93): no frame
//   reaches past signal_len (the reference's zero-fill branch :105-109 is dead), trailing samples that fill no frame are ignored;
//   FRAMES_STFT   out[s][w][k] = FFT_n(window * frame)[k]                        complex, unscaled
//   FRAMES_POWER  out[s][w][k] = |.|^2 / (sample_rate * P), doubled for 0 < k < n/2, k <= n/2     real
//   FRAMES_WELCH  out[s][k]    = mean over w of the POWER rows                                     real
//   P = 0.375 n for the Hann window (hard-coded in the reference, :72; FUSED_PSD uses the same), sum w[i]^2 otherwise.
// n a power of two that fits ONE hook-capable pass: one launch of the hooked single-pass kernel with the framed load (frames of
// all signals are its tile columns; the window is its load-side table; POWER / WELCH: its one-sided power store), Welch adds
// frames_mean_kernel.  Every other n, and no_fusion: per signal one execute_hooked with in_pitch = hop (pad_mul_kernel + a plain
// execute where the core has no hooks or a signal does not start 16-byte aligned), psd_onesided_kernel, frames_mean_kernel --
// a correct fallback, not a tuned one.
//
// real_input: x holds REAL signals (signal_len, hop, signal_pitch count reals), n a power of two >= 4, and every row is one-sided:
//   FRAMES_STFT out[s][w][k], k <= n/2 complex; POWER / WELCH as above.  The core is the transform of HALF the length, L = n/2, on
//   z[m] = y[2m] + i y[2m+1] (y the windowed frame: the reals read as complex pairs, the window table packed the same way), and
//   the split  E = (Z[k] + conj Z[L-k]) / 2, O = (Z[k] - conj Z[L-k]) / (2i), X[k] = E + W_n^k O  yields the n/2 + 1 bins.
//   Where L fits one hook-capable pass the split rides in that pass's store (tile_fft_kernel's HOOKBIT_REAL: both Z[k] and Z[L-k] of a
//   frame lie in one LDS row there): one launch reads the reals in place and writes the one-sided rows.  Every other n, and
//   no_fusion: frames_pack_real_kernel (windowed frames -> [frames][L] complex), the plain core, r2c_split_kernel, and for POWER /
//   WELCH psd_onesided_rows_kernel -- correct, not tuned.
// ---------------------------------------------------------------------------
enum FramesOut { FRAMES_STFT = 0, FRAMES_POWER = 1, FRAMES_WELCH = 2 };

// the load side every frames execute shares: frames of n_in samples of the core, `hop` apart, times the window `win` on the way in (NULL: none)
template <typename T>
ExecHooks<T> frame_hooks(const cpx<T>* win, int win_mode, long long n_in, long long hop) {
    ExecHooks<T> f;
    f.pre_tab = win; f.pre_mode = win_mode;
    f.n_in = n_in; f.in_pitch = hop;
    return f;
}

template <typename T, typename RT>
class FramesPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr int V = 16 / SZ;
    RT* rt = nullptr;
    int n = 0, hop = 0, signal_len = 0, n_signals = 0, nw = 0, window = 0, out_kind = 0;
    long double window_power = 1.0L;  // P
    Pow2Plan<T, RT> core;
    cpx<T>* win = nullptr;    // the window as complex values, + 1 padding entry (ExecHooks::pre_tab)
    T* power = nullptr;       // WELCH: [n_signals * nw][n/2 + 1]
    cpx<T>* work = nullptr;   // fallback, POWER / WELCH: the complex rows [n_signals * nw][n] (allocated at its first use)
    bool real_input = false;  // real signals, one-sided rows (see above); win then holds n/2 (+ 1) PAIRS of window values
    cpx<T>* wsplit = nullptr; // real_input: W_n^k, k <= n/2
    cpx<T>* zwork = nullptr;  // real_input fallback: the packed frames and their spectra [n_signals * nw][n/2] (allocated at its first use)
    cpx<T>* xwork = nullptr;  // real_input fallback, POWER / WELCH: the split rows [n_signals * nw][n/2 + 1] (allocated at its first use)
    bool ok = false;
    bool no_fusion = false;
    ~FramesPlan() {
        if (!rt) return;
        rt->dfree(win); rt->dfree(power); rt->dfree(work); rt->dfree(wsplit); rt->dfree(zwork); rt->dfree(xwork);
    }
    template <class F> void each_core(F&& f) { f(&core); }
    void set_no_fusion(bool v) { no_fusion = v; }
    long long frames() const { return (long long)n_signals * nw; }
    int bins() const { return n / 2 + 1; }
    bool fused() const { return ok && !no_fusion && core.round_capable() && core.frames_exact(frames(), nw); }

    // w_host: n window values of type T (WINDOW_USER), ignored otherwise
    bool build(RT* runtime, int n_, int hop_, int signal_len_, int n_signals_, int window_, const T* w_host, int out_kind_, bool real_input_ = false) {
        rt = runtime; n = n_; hop = hop_; signal_len = signal_len_; n_signals = n_signals_; window = window_; out_kind = out_kind_;
        real_input = real_input_;
        if (n < (real_input ? 4 : 2) || (n & (n - 1)) != 0 || n > (1 << 29) || hop < 1 || hop > n || signal_len < n || n_signals < 1) return false;
        if (window < WINDOW_RECT || window > WINDOW_USER || (window == WINDOW_USER && !w_host)) return false;
        if (out_kind < FRAMES_STFT || out_kind > FRAMES_WELCH) return false;
        nw = (signal_len - (n - hop)) / hop;
        if (nw < 1 || frames() > 0x7fffffff || frames() * (long long)n > (1ll << 40)) return false;
        core.wants_hooks = true;
        if (!core.build(rt, ilog2(real_input ? n / 2 : n), ALGO_AUTO, (int)frames())) return false;
        // the window as complex values; + 1 padding entry
        std::vector<cpx<T>> wv((size_t)n + 1);
        const std::vector<long double> wl = window_values(window, n, w_host);
        long double sum2 = 0.0L;
        for (int i = 0; i < n; i++) {
            sum2 += wl[(size_t)i] * wl[(size_t)i];
            wv[(size_t)i].re = (T)wl[(size_t)i];
            wv[(size_t)i].im = 0;
        }
        wv[(size_t)n] = wv[0];
        window_power = window == WINDOW_HANN ? 0.375L * (long double)n : sum2;
        if (out_kind != FRAMES_STFT && !(window_power > 0.0L)) return false;
        if (real_input) {  // entry m = (w[2m], w[2m+1]): the factors of the real samples that make up complex sample m (+ 1 padding entry)
            const int h = n / 2;
            for (int m = 0; m < h; m++) {
                const T w0 = wv[(size_t)(2 * m)].re, w1 = wv[(size_t)(2 * m + 1)].re;
                wv[(size_t)m].re = w0;
                wv[(size_t)m].im = w1;
            }
            wv[(size_t)h] = wv[0];
            wv.resize((size_t)h + 1);
            std::vector<cpx<T>> t;
            make_twiddle_table<T>(t, n, (long long)h + 1, 1);
            wsplit = (cpx<T>*)rt->dmalloc(t.size() * SZ);
            if (!wsplit) return false;
            rt->h2d(wsplit, t.data(), t.size() * SZ);
        }
        win = (cpx<T>*)rt->dmalloc(wv.size() * SZ);
        if (!win) return false;
        rt->h2d(win, wv.data(), wv.size() * SZ);
        if (out_kind == FRAMES_WELCH) {
            power = (T*)rt->dmalloc((size_t)frames() * (size_t)bins() * sizeof(T));
            if (!power) return false;
        }
        ok = true;
        return true;
    }

    // x: the signals (signal_pitch elements apart; 0: signal_len); out: see FramesOut.  0 / -1 (bad arguments: nothing is launched)
    // real_input: x points at REAL samples and signal_pitch counts reals
    int execute(const cpx<T>* x, long long signal_pitch, void* out, double sample_rate) {
        if (!ok || !x || !out || (const void*)x == (const void*)out) return -1;
        if (signal_pitch == 0) signal_pitch = signal_len;
        if (signal_pitch < signal_len) return -1;
        const long long nf = frames();
        const int hb = bins();
        const T scale = (T)(1.0L / ((long double)sample_rate * window_power));
        T* rows = out_kind == FRAMES_WELCH ? power : (T*)out;  // where the power rows go
        if (real_input) {
            const int h = n / 2;
            if (fused()) {
                ExecHooks<T> f = frame_hooks<T>(win, fftk::HOOK_MUL_PAIR, h, hop);
                f.frames_per_signal = nw; f.signal_pitch = signal_pitch;
                f.real_frames = true; f.post_tab = wsplit; f.out_pitch = hb;
                if (out_kind == FRAMES_STFT) {
                    core.execute_frames(x, (cpx<T>*)out, (int)nf, f);
                } else {
                    f.power_out = rows; f.power_scale = scale;
                    core.execute_frames(x, reinterpret_cast<cpx<T>*>(rows), (int)nf, f);  // (complex `out` unused: the power store replaces it)
                }
            } else {
                if (!zwork) zwork = (cpx<T>*)rt->dmalloc((size_t)nf * (size_t)h * SZ);
                if (!zwork) return -1;
                cpx<T>* X = (cpx<T>*)out;
                if (out_kind != FRAMES_STFT) {
                    if (!xwork) xwork = (cpx<T>*)rt->dmalloc((size_t)nf * (size_t)hb * SZ);
                    if (!xwork) return -1;
                    X = xwork;
                }
                launch_flat(rt, fftk::frames_pack_real_kernel<T>, nf * h, reinterpret_cast<const T*>(x), signal_pitch, hop, nw, h, (const cpx<T>*)win, zwork, nf * h);
                core.execute(zwork, zwork, (int)nf, false);
                launch_flat(rt, fftk::r2c_split_kernel<T>, nf * (h / 2 + 1), (const cpx<T>*)zwork, X, (const cpx<T>*)wsplit, h, nf * (h / 2 + 1));
                if (out_kind != FRAMES_STFT)
                    launch_flat(rt, fftk::psd_onesided_rows_kernel<T>, nf * hb, (const cpx<T>*)X, (long long)hb, rows, hb, scale, nf * hb);
            }
        } else if (fused()) {
            ExecHooks<T> f = frame_hooks<T>(win, fftk::HOOK_MUL, n, hop);
            f.frames_per_signal = nw; f.signal_pitch = signal_pitch;
            if (out_kind == FRAMES_STFT) {
                core.execute_frames(x, (cpx<T>*)out, (int)nf, f);
            } else {
                f.power_out = rows; f.power_scale = scale;
                core.execute_frames(x, reinterpret_cast<cpx<T>*>(rows), (int)nf, f);  // (complex `out` unused: the power store replaces it)
            }
        } else {
            cpx<T>* stage = (cpx<T>*)out;
            if (out_kind != FRAMES_STFT) {
                if (!work) work = (cpx<T>*)rt->dmalloc((size_t)nf * (size_t)n * SZ);
                if (!work) return -1;
                stage = work;
            }
            const bool aligned = (signal_pitch % V) == 0 && ((uintptr_t)x & 15) == 0;  // every signal starts 16-byte aligned
            if (core.hook_capable() && aligned) {
                const ExecHooks<T> f = frame_hooks<T>(win, fftk::HOOK_MUL, n, hop);
                for (int s = 0; s < n_signals; s++)
                    core.execute_hooked(x + (long long)s * signal_pitch, stage + (long long)s * nw * n, nw, false, f);
            } else {
                const unsigned per_block = 256 * BLU_PER_THREAD;
                const unsigned bpr = (unsigned)(((long long)n + per_block - 1) / per_block);
                for (int s = 0; s < n_signals; s++)
                    rt->launch(fftk::pad_mul_kernel<T>, (long long)bpr * nw, 256, (size_t)0, x + (long long)s * signal_pitch, (long long)hop, n,
                               (const cpx<T>*)win, (int)fftk::HOOK_MUL, stage + (long long)s * nw * n, n, bpr);
                core.execute(stage, stage, (int)nf, false);
            }
            if (out_kind != FRAMES_STFT)
                launch_flat(rt, fftk::psd_onesided_kernel<T>, nf * hb, (const cpx<T>*)stage, rows, n, scale, nf * hb);
        }
        if (out_kind == FRAMES_WELCH)
            launch_flat(rt, fftk::frames_mean_kernel<T>, (long long)n_signals * hb, (const T*)power, (T*)out, nw, hb, (long long)n_signals * hb);
        return 0;
    }
};

// ---------------------------------------------------------------------------
// Inverse STFT: the way back from the real frames plan's STFT rows to real signals, by weighted overlap-add.
//   X: [n_signals][nw][n/2 + 1] one-sided rows, contiguous (what FramesPlan with real_input writes as FRAMES_STFT);
//   v_w = irfft_n(X[s][w]), scaled by 1/n (irfft(rfft(x)) = x); the imaginary parts of bins 0 and n/2 are ignored;
//   env[t]  = sum_w g[t - w hop]^2,    y[s][t] = (sum_w g[t - w hop] v_w[t - w hop]) / env[t],    t < out_len = (nw - 1) hop + n,
//   w over the frames that cover t, g the window (FramesPlan's own kinds: one window serves analysis and synthesis).  This is the
//   least-squares inverse: y = x for X = stft(x) wherever env[t] > 0.  Where env[t] <= 1e-10 max g^2 (scipy's istft constant) the
//   sample cannot be recovered: inv_env[t] = 0 and y[s][t] is written as exactly 0 (`unrecoverable` counts them per signal).
//   Signal s starts at y + s * signal_pitch reals.
// The core is the inverse transform of HALF the length, L = n/2, on the c2r merge of every row (RealPlan's identity).  Where L fits
// one hook-capable pass the merge rides in that pass's load (tile_fft_kernel's HOOKBIT_HERM): one launch turns the rows into the
// [frames][n] real workspace.  Every other n (n = 4 included), and no_fusion: iframes_merge_kernel and the plain core in place on
// the workspace -- correct, not tuned.  frames_overlap_add_kernel then writes the signals.
// ---------------------------------------------------------------------------
template <typename T, typename RT>
class IFramesPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    RT* rt = nullptr;
    int n = 0, hop = 0, nw = 0, n_signals = 0, window = 0;
    int unrecoverable = 0;    // samples per signal with a vanishing envelope (written as 0)
    Pow2Plan<T, RT> core;     // length n/2
    T* win = nullptr;         // the window, n reals
    T* inv_env = nullptr;     // 1 / env[t], out_len reals (0 where env vanishes)
    cpx<T>* wmerge = nullptr; // W_n^k, k <= n/2
    cpx<T>* work = nullptr;   // [frames][n/2] complex = [frames][n] reals
    bool ok = false;
    bool no_fusion = false;
    ~IFramesPlan() {
        if (!rt) return;
        rt->dfree(win); rt->dfree(inv_env); rt->dfree(wmerge); rt->dfree(work);
    }
    template <class F> void each_core(F&& f) { f(&core); }
    void set_no_fusion(bool v) { no_fusion = v; }
    long long frames() const { return (long long)n_signals * nw; }
    long long out_len() const { return (long long)(nw - 1) * hop + n; }
    bool fused() const { return ok && !no_fusion && core.round_capable(); }

    // w_host: n window values of type T (WINDOW_USER), ignored otherwise
    bool build(RT* runtime, int n_, int hop_, int n_frames_, int n_signals_, int window_, const T* w_host) {
        rt = runtime; n = n_; hop = hop_; nw = n_frames_; n_signals = n_signals_; window = window_;
        if (n < 4 || (n & (n - 1)) != 0 || n > (1 << 29) || hop < 1 || hop > n || nw < 1 || n_signals < 1) return false;
        if (window < WINDOW_RECT || window > WINDOW_USER || (window == WINDOW_USER && !w_host)) return false;
        if (frames() > 0x7fffffff || frames() * (long long)n > (1ll << 40) || out_len() > 0x7fffffff) return false;
        const int h = n / 2;
        core.wants_hooks = true;
        if (!core.build(rt, ilog2(h), ALGO_AUTO, (int)frames())) return false;
        // the frames plans' windows as reals of T; the envelope is built from those ROUNDED values -- the ones the kernels multiply
        // by -- in long double
        std::vector<T> g((size_t)n);
        const std::vector<long double> wl = window_values(window, n, w_host);
        long double gmax2 = 0.0L;
        for (int i = 0; i < n; i++) {
            g[(size_t)i] = (T)wl[(size_t)i];
            const long double g2 = (long double)g[(size_t)i] * (long double)g[(size_t)i];
            if (g2 > gmax2) gmax2 = g2;
        }
        const long long ol = out_len();
        std::vector<T> ie((size_t)ol);
        unrecoverable = 0;
        for (long long t = 0; t < ol; t++) {
            const long long w0 = t < n ? 0 : (t - n + hop) / hop;
            long long w1 = t / hop;
            if (w1 > nw - 1) w1 = nw - 1;
            long double env = 0.0L;
            for (long long w = w0; w <= w1; w++) {
                const long double gv = (long double)g[(size_t)(t - w * hop)];
                env += gv * gv;
            }
            if (env > 1e-10L * gmax2) {
                ie[(size_t)t] = (T)(1.0L / env);
            } else {
                ie[(size_t)t] = (T)0;
                unrecoverable++;
            }
        }
        std::vector<cpx<T>> tw;
        make_twiddle_table<T>(tw, n, (long long)h + 1, 1);
        win = (T*)rt->dmalloc((size_t)n * sizeof(T));
        inv_env = (T*)rt->dmalloc((size_t)ol * sizeof(T));
        wmerge = (cpx<T>*)rt->dmalloc(tw.size() * SZ);
        work = (cpx<T>*)rt->dmalloc((size_t)frames() * (size_t)h * SZ);
        if (!win || !inv_env || !wmerge || !work) return false;
        rt->h2d(win, g.data(), (size_t)n * sizeof(T));
        rt->h2d(inv_env, ie.data(), (size_t)ol * sizeof(T));
        rt->h2d(wmerge, tw.data(), tw.size() * SZ);
        ok = true;
        return true;
    }

    // X: the one-sided rows; y: the signals (signal_pitch reals apart; 0: out_len).  0 / -1 (bad arguments: nothing is launched)
    int execute(const cpx<T>* X, T* y, long long signal_pitch) {
        if (!ok || !X || !y || (const void*)X == (const void*)y) return -1;
        if (signal_pitch == 0) signal_pitch = out_len();
        if (signal_pitch < out_len()) return -1;
        const long long nf = frames();
        const int h = n / 2;
        if (fused()) {
            ExecHooks<T> f;
            f.pre_tab = wmerge;
            core.execute_iframes(X, work, (int)nf, f);
        } else {
            launch_flat(rt, fftk::iframes_merge_kernel<T>, nf * h, X, work, (const cpx<T>*)wmerge, h, nf * h);
            core.execute(work, work, (int)nf, true);
        }
        const long long total = (long long)n_signals * out_len();
        launch_flat(rt, fftk::frames_overlap_add_kernel<T>, total, reinterpret_cast<const T*>(work), (const T*)win, (const T*)inv_env, y, signal_pitch, n, hop,
                    nw, out_len(), total);
        return 0;
    }
};

// ---------------------------------------------------------------------------
// Overlap-save FIR filtering of long signals (reference applications/fft_filtering.c is the CPU consumer; its whole-signal mask is not
// rebuilt): y = x * h for n_signals signals of signal_len samples and M = n_taps fixed taps, block by block.
//   block length n (a power of two > M - 1), lead = M - 1, advance B = n - lead; block w of a signal holds its samples
//   q = w B - lead + l, l < n (zero outside [0, signal_len)); of IFFT_n(FFT_n(block) . FFT_n(h)) the values l >= lead are the full
//   convolution's samples w B ... w B + B - 1 (the first lead values are the circular wrap and are dropped);
//   FULL     out_len = signal_len + M - 1, out_off = 0            np.convolve(x, h)
//   CAUSAL   out_len = signal_len,         out_off = 0            y[t] = sum_j h[j] x[t - j]
//   CENTRED  out_len = signal_len,         out_off = (M - 1) / 2  np.convolve(x, h, 'same')
//   y[p] = full[p + out_off], p < out_len;  nb = ceil((out_off + out_len) / B) blocks per signal.
// FFT_n(h) is computed once at plan time by the plan's own core.  Where n fits one hook-capable pass: ONE launch of the hooked
// single-pass kernel over all n_signals * nb blocks (bounded framed load, spectral product and inverse on the registers, valid-part
// framed store: tile_fft_kernel's HOOKBIT_BOUND and HOOKBIT_VALID) -- one HBM round trip of the user's data, no [blocks][n] copy in or out.  Every
// other n, a block count frames_exact() refuses, no_fusion and no_chain: filter_gather_kernel -> the core's forward . H . inverse
// (one kernel, chained or hooked, as FusedPlan's circular convolution runs them) -> filter_scatter_kernel on chunks of blocks, so
// the workspace stays bounded -- correct, not tuned.
// n = 0: the plan chooses min(nmax, max(256, next_pow2(4 M))), nmax = 4096 (fp32) / 2048 (fp64); taps with M - 1 >= nmax / 2 get
// next_pow2(4 M) on the fallback.  The rule is a guess, not a measurement.
// ---------------------------------------------------------------------------
enum FilterOut { FILTER_FULL = 0, FILTER_CAUSAL = 1, FILTER_CENTRED = 2 };

template <typename T, typename RT>
class FilterPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr int kNmax = SZ == 8 ? 4096 : 2048;          // the largest block length one hooked pass holds
    static constexpr long long kChunkElems = 1ll << 22;          // fallback: values per workspace (two of them)
    RT* rt = nullptr;
    int n_taps = 0, signal_len = 0, n_signals = 0, n = 0, B = 0, lead = 0, out_kind = 0, out_len = 0, out_off = 0, nb = 0;
    Pow2Plan<T, RT> core;
    cpx<T>* H = nullptr;       // FFT_n(h zero padded to n)
    cpx<T>* work = nullptr;    // fallback: [chunk_blocks][n] gathered blocks, and [chunk_blocks][n] results behind them (allocated at its first use)
    int chunk_blocks = 1;
    bool ok = false;
    bool no_fusion = false;
    bool no_chain = false;
    ~FilterPlan() {
        if (!rt) return;
        rt->dfree(H); rt->dfree(work);
    }
    template <class F> void each_core(F&& f) { f(&core); }
    void set_no_fusion(bool v) { no_fusion = v; }
    void set_no_chain(int v) { no_chain = v == 1; core.set_chain_rule(v == 2); }  // (BluesteinPlan::set_no_chain)
    long long blocks() const { return (long long)n_signals * nb; }
    static int choose_n(int n_taps) {
        long long want = 1;
        while (want < 4ll * n_taps) want <<= 1;
        if (n_taps - 1 >= kNmax / 2) return want > (1ll << 30) ? 0 : (int)want;
        if (want < 256) want = 256;
        return want > kNmax ? kNmax : (int)want;
    }
    bool hooked() const { return ok && !no_fusion && core.hook_capable(); }
    // (n <= kNmax: a device whose LDS holds one pass of 4096 fp64 points still takes the fallback there -- the one-launch kernel is
    // checked up to kNmax and no further)
    bool fused() const { return hooked() && !no_chain && n <= kNmax && core.round_capable() && core.frames_exact(blocks(), nb); }
    // what fft_gpu_plan_info_hip reports: 3 the one-launch path; on the fallback 2 the middle is one kernel or chained, 1 hooked passes, 0 plain
    int path() const {
        if (fused()) return 3;
        if (!hooked()) return 0;
        return (!no_chain && (core.round_capable() || core.chain_capable())) ? 2 : 1;
    }

    // h_host: n_taps complex taps; n_: the block length, 0: the plan chooses
    bool build(RT* runtime, int n_taps_, const cpx<T>* h_host, int signal_len_, int n_signals_, int n_, int out_kind_) {
        rt = runtime; n_taps = n_taps_; signal_len = signal_len_; n_signals = n_signals_; out_kind = out_kind_;
        if (n_taps < 1 || !h_host || signal_len < 1 || n_signals < 1 || n_ < 0 || out_kind < FILTER_FULL || out_kind > FILTER_CENTRED) return false;
        n = n_ ? n_ : choose_n(n_taps);
        if (n < 1 || (n & (n - 1)) != 0 || n > (1 << 29) || n <= n_taps - 1) return false;
        lead = n_taps - 1;
        B = n - lead;
        const long long ol = out_kind == FILTER_FULL ? (long long)signal_len + lead : (long long)signal_len;
        if (ol > 0x7fffffff) return false;
        out_len = (int)ol;
        out_off = out_kind == FILTER_CENTRED ? lead / 2 : 0;
        const long long per = ((long long)out_off + out_len + B - 1) / B;
        if (per * n_signals > 0x7fffffff) return false;
        nb = (int)per;
        long long cb = kChunkElems / n;
        if (cb < 1) cb = 1;
        chunk_blocks = (int)(cb < blocks() ? cb : blocks());
        core.prefer_chain = true;
        core.wants_hooks = true;
        // a block length above kNmax never takes the one-launch path and only ever runs on chunks: its (multi-pass) core and the
        // scratch images that core owns are sized for one chunk, not for the whole execute
        if (!core.build(rt, ilog2(n), ALGO_AUTO, n > kNmax ? chunk_blocks : (int)blocks())) return false;
        H = kernel_spectrum(rt, core, h_host, n_taps, n);
        if (!H) return false;
        ok = true;
        return true;
    }

    // out = IFFT(FFT(in) . H) for nbk contiguous blocks: the circular convolution of FusedPlan, by the same kernels
    void middle(const cpx<T>* in, cpx<T>* out, int nbk) {
        if (hooked() && !no_chain && core.round_capable()) {
            ExecHooks<T> rr;
            rr.mid_tab = H; rr.mid_mode = fftk::HOOK_MUL;
            core.execute_round(in, out, nbk, rr);
            return;
        }
        if (hooked()) {
            ExecHooks<T> f, g;
            f.post_tab = H; f.post_mode = fftk::HOOK_MUL;
            if (!no_chain && core.chain_capable() && core.execute_chain(in, out, nbk, f, g)) return;
            core.execute_hooked(in, out, nbk, false, f);
            core.execute_hooked(out, out, nbk, true, g);
            return;
        }
        const unsigned per_block = 256 * BLU_PER_THREAD;
        const unsigned bpr = (unsigned)(((long long)n + per_block - 1) / per_block);
        core.execute(in, out, nbk, false);
        rt->launch(fftk::mul_store_kernel<T>, (long long)bpr * nbk, 256, (size_t)0, (const cpx<T>*)out, (long long)n, (const cpx<T>*)H, 0ll, (int)fftk::HOOK_MUL, out,
                   (long long)n, n, (T)1, bpr);
        core.execute(out, out, nbk, true);
    }

    // x: the signals (x_pitch elements apart; 0: signal_len); y: the outputs (y_pitch apart; 0: out_len), overlapping x nowhere -- blocks
    // re-read their neighbours' input, so in place cannot work.  0 / -1 (bad arguments: nothing is launched)
    int execute(const cpx<T>* x, long long x_pitch, cpx<T>* y, long long y_pitch) {
        if (!ok || !x || !y) return -1;
        if (x_pitch == 0) x_pitch = signal_len;
        if (y_pitch == 0) y_pitch = out_len;
        if (x_pitch < signal_len || y_pitch < out_len) return -1;
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)((long long)(n_signals - 1) * x_pitch + signal_len) * SZ;
        const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (size_t)((long long)(n_signals - 1) * y_pitch + out_len) * SZ;
        if (x0 < y1 && y0 < x1) return -1;
        if (fused()) {
            ExecHooks<T> f;
            f.in_pitch = B;
            f.frames_per_signal = nb; f.signal_pitch = x_pitch;
            f.frame_lead = lead; f.signal_len = signal_len;
            f.mid_tab = H; f.mid_mode = fftk::HOOK_MUL;
            f.out_signal_pitch = y_pitch; f.out_len = out_len; f.out_off = out_off;
            core.execute_filter(x, y, (int)blocks(), f);
            return 0;
        }
        if (!work) work = (cpx<T>*)rt->dmalloc((size_t)2 * (size_t)chunk_blocks * (size_t)n * SZ);
        if (!work) return -1;
        cpx<T>* res = work + (size_t)chunk_blocks * (size_t)n;
        const int log2n = ilog2(n);
        for (long long f0 = 0; f0 < blocks(); f0 += chunk_blocks) {
            const int cb = (int)(blocks() - f0 < chunk_blocks ? blocks() - f0 : chunk_blocks);
            const long long total = (long long)cb * n;
            launch_flat(rt, fftk::filter_gather_kernel<T>, total, x, x_pitch, signal_len, nb, B, lead, log2n, f0, work, total);
            middle(work, res, cb);
            launch_flat(rt, fftk::filter_scatter_kernel<T>, total, (const cpx<T>*)res, y, y_pitch, out_len, out_off, nb, B, lead, log2n, f0, total);
        }
        return 0;
    }
};

// ---------------------------------------------------------------------------
// 2D convolution and frequency-domain image filtering: y = IFFT2( FFT2(x zero padded to P x Q) . H ) for n_matrices row-major
// rows x cols images and ONE kernel fixed at plan time (reference applications/convolution.c:99-109, fft_convolution_2d, is a
// placeholder; applications/image_fft.c:147-235 masks the 2D spectrum of an image).
//   FULL      out (rows + krows - 1) x (cols + kcols - 1)                      scipy.signal.convolve2d 'full'
//   SAME      out rows x cols           = full[(krows-1)/2 ..][(kcols-1)/2 ..]
//   VALID     out (rows - krows + 1) x (cols - kcols + 1), krows <= rows, kcols <= cols    = full[krows-1 ..][kcols-1 ..]
//   CIRCULAR  rows, cols powers of two, krows <= rows, kcols <= cols: the kernel wraps, out rows x cols
//   SPECTRUM  rows, cols powers of two, k_host IS H[rows][cols] in natural (unshifted) order: out = IFFT2(FFT2(x) . H)
// P = next_pow2(rows + krows - 1), Q = next_pow2(cols + kcols - 1) for the three linear modes, P = rows, Q = cols otherwise.  The
// result carries ONE 1 / (P Q), like Plan2D (the reference's fft_2d divides twice, image_fft.c:64-71).
//
// The shift.  At plan time the kernel goes into a [P][Q] host array at k'[(i - sr) mod P][(j - sc) mod Q] = k[i][j], with the
// output offset (sr, sc) = ((krows-1)/2, (kcols-1)/2) for SAME, (krows-1, kcols-1) for VALID, (0, 0) otherwise; H = FFT2(k') is
// computed once on the device by a Plan2D.  The circular convolution c of the padded image with k' is then
//   c[u][v] = sum over (s, t) with s = u + sr (mod P), t = v + sc (mod Q) of full[s][t],
// full being the linear convolution, supported on 0 <= s <= F - 1 = rows + krows - 2 (and the same along the columns).  Every wanted
// output has 0 <= u < out_rows, and in each mode u + sr lies in [0, F - 1]: FULL [0, F - 1]; SAME [sr, rows - 1 + sr] with
// sr <= krows - 1; VALID [krows - 1, rows - 1].  The other members of its residue class are u + sr + P >= P >= F (beyond the support)
// and u + sr - P <= F - 1 - P < 0 (before it): exactly one term, c[u][v] = full[u + sr][v + sc].  So no wanted output aliases, the
// wanted block starts at [0][0], and no pass needs an offset.
//
// Fused path (three HBM round trips of compact work images, nothing zero-filled, copied or cropped):
//   1  rows forward   rows * M transforms of length Q, execute_hooked with n_in = cols: the padding COLUMNS are never read, the
//                     padding ROWS are never transformed or stored -> work1 [M][rows][Q]
//   2  column round   tile_fft_colround_kernel: forward column stages, product with H, inverse column stages on one P x C tile;
//                     loads rows < rows, stores rows < out_rows -> work2 [M][out_rows][Q]
//   3  rows inverse   out_rows * M transforms with n_out = out_cols, straight into the caller's matrices
// taken where the one-pass column plan (Pow2Plan::build_columns) exists with E = 8 (P >= 8) and row segments of at least
// min_seg_bytes = 64 bytes -- Plan2D's own criterion for its one-pass column -- and the row plan is hook capable.  A caller's base
// pointer that is not 16-byte aligned (or, with a matrix pitch of its own, a pitch that is no multiple of 16 bytes) keeps steps 2 and
// the other end but pads / crops that end's rows with pad_mul_kernel / mul_store_kernel around the plain row plan.
// Fallback (everything else and no_fusion; five round trips of the padded image, correct, not tuned): conv2d_pad_kernel into
// [M][P][Q], forward Plan2D, mul_store_kernel against H, inverse Plan2D, conv2d_crop_kernel.  Its plans and image are made at the
// first execute that needs them.
// ---------------------------------------------------------------------------
enum Conv2DMode { CONV2D_FULL = 0, CONV2D_SAME = 1, CONV2D_VALID = 2, CONV2D_CIRCULAR = 3, CONV2D_SPECTRUM = 4 };

// the column round as a step of its own: P x Q matrices (Q any multiple of the 16-byte lane access), rows_in rows in, rows_out rows out
template <typename T, typename RT>
class ColRoundStep {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    RT* rt = nullptr;
    Pow2Plan<T, RT> colp;  // build_columns: the tile and the stage tables
    int log2P = 0, Q = 0;
    bool ok = false;
    template <class F> void each_core(F&& f) {
        if (colp.ok) f(&colp);
    }
    bool build(RT* runtime, int log2P_, int Q_, int n_matrices, int min_seg_bytes) {
        rt = runtime; log2P = log2P_; Q = Q_;
        if (!colp.build_columns(rt, log2P, Q, n_matrices)) return false;
        const PassDesc& a = colp.passes[0];
        ok = a.E == 8 && a.log2H == 0 && a.nthreads <= 512 && a.seg_bytes >= min_seg_bytes;
        return ok;
    }
    int tile_cols() const { return ok ? 1 << colp.passes[0].log2C : 0; }
    // out[m][K][c] = (1/P) IFFT_P( FFT_P(in[m][.][c], rows >= rows_in zero) . H[.][c] )[K], K < rows_out
    void run(const cpx<T>* in, int rows_in, const cpx<T>* H, cpx<T>* out, int rows_out, int nm) {
        const PassDesc& a = colp.passes[0];
        fftk::ColRoundParams<T> q;
        memset(&q, 0, sizeof(q));
        q.in = in; q.out = out; q.spec = H; q.tables = colp.pass_tables[0];
        q.group_bytes = a.group_bytes; q.tables_bytes = a.tables_elems * SZ; q.off_tables = a.off_tables; q.o_sb = a.o_sb; q.sa_bits = a.sa_bits;
        q.log2L = a.log2L; q.log2C = a.log2C; q.n_ct = a.n_ct; q.n_cols = Q;
        q.rows_in = rows_in; q.rows_out = rows_out;
        q.in_b = (long long)rows_in * Q; q.out_b = (long long)rows_out * Q; q.ld = Q;
        q.n_tiles = (long long)nm * a.n_ct;
        q.nt = a.seg_bytes >= 128 ? 3 : 0;  // the tile passes' rule (Pow2Plan::pass_params): whole 128-byte lines only; not measured here
        q.scale = (T)(1.0L / (long double)(1ll << log2P));
        int per_cu = rt->max_blocks_per_cu(fftk::tile_fft_colround_kernel<T>, a.nthreads, (size_t)a.smem_bytes);
        if (per_cu < 1) per_cu = 1;
        long long grid = (long long)rt->num_cus() * per_cu;
        if (grid > q.n_tiles) grid = q.n_tiles;
        rt->launch(fftk::tile_fft_colround_kernel<T>, grid, a.nthreads, (size_t)a.smem_bytes, q);
    }
};

template <typename T, typename RT>
class Conv2DPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr int V = 16 / SZ;
    RT* rt = nullptr;
    int rows = 0, cols = 0, krows = 0, kcols = 0, n_matrices = 0, mode = 0;
    int P = 0, Q = 0, out_rows = 0, out_cols = 0;
    Pow2Plan<T, RT> rowp;          // length Q, hooked ends
    ColRoundStep<T, RT> round;
    cpx<T>* H = nullptr;           // [P][Q]: FFT2 of the placed kernel, or the caller's spectrum
    cpx<T>* work1 = nullptr;       // fused: [M][rows][Q]
    cpx<T>* work2 = nullptr;       // fused: [M][out_rows][Q]
    Plan2D<T, RT>* fwd = nullptr;  // fallback (made at its first use)
    Plan2D<T, RT>* inv = nullptr;
    cpx<T>* fwork = nullptr;       // fallback: [M][P][Q]
    int min_seg_bytes = 64;        // the fused path's row-segment criterion (tests narrow it to reach narrow tiles)
    bool ok = false;
    bool no_fusion = false;
    ~Conv2DPlan() {
        delete fwd;
        delete inv;
        if (!rt) return;
        rt->dfree(H); rt->dfree(work1); rt->dfree(work2); rt->dfree(fwork);
    }
    template <class F> void each_core(F&& f) {
        f(&rowp);
        round.each_core(f);
        if (fwd) fwd->each_core(f);  // (the fallback's plans: once an execute has made them)
        if (inv) inv->each_core(f);
    }
    void set_no_fusion(bool v) { no_fusion = v; }
    bool fusable() const { return ok && round.ok && rowp.ok && rowp.hook_capable() && work1 && work2; }
    bool fused() const { return fusable() && !no_fusion; }
    int passes() const { return fused() ? 3 : 5; }  // HBM round trips of the work image

    static bool sizes(int rows, int cols, int krows, int kcols, int mode, int& P, int& Q, int& orows, int& ocols) {
        if (rows < 1 || cols < 1 || krows < 1 || kcols < 1 || mode < CONV2D_FULL || mode > CONV2D_SPECTRUM) return false;
        const long long fr = (long long)rows + krows - 1, fc = (long long)cols + kcols - 1;
        if (mode >= CONV2D_CIRCULAR) {
            if ((rows & (rows - 1)) != 0 || (cols & (cols - 1)) != 0) return false;
            if (mode == CONV2D_CIRCULAR ? (krows > rows || kcols > cols) : (krows != rows || kcols != cols)) return false;
            P = rows; Q = cols; orows = rows; ocols = cols;
        } else {
            if (mode == CONV2D_VALID && (krows > rows || kcols > cols)) return false;
            if (fr > (1ll << 30) || fc > (1ll << 30)) return false;
            long long p = 1, q = 1;
            while (p < fr) p <<= 1;
            while (q < fc) q <<= 1;
            P = (int)p; Q = (int)q;
            orows = mode == CONV2D_FULL ? (int)fr : mode == CONV2D_SAME ? rows : rows - krows + 1;
            ocols = mode == CONV2D_FULL ? (int)fc : mode == CONV2D_SAME ? cols : cols - kcols + 1;
        }
        return (long long)P * Q <= (1ll << 30);
    }

    // k_host: krows x kcols complex values, row-major (SPECTRUM: H itself)
    bool build(RT* runtime, int rows_, int cols_, int krows_, int kcols_, const cpx<T>* k_host, int n_matrices_, int mode_, int min_seg = 64) {
        rt = runtime; rows = rows_; cols = cols_; krows = krows_; kcols = kcols_; n_matrices = n_matrices_; mode = mode_; min_seg_bytes = min_seg;
        if (!k_host || n_matrices < 1 || !sizes(rows, cols, krows, kcols, mode, P, Q, out_rows, out_cols)) return false;
        if ((long long)P * n_matrices > 0x7fffffff || (long long)Q * n_matrices > 0x7fffffff) return false;
        const size_t pq = (size_t)P * (size_t)Q;
        {   // H
            std::vector<cpx<T>> hp(pq);
            if (mode == CONV2D_SPECTRUM) {
                std::copy(k_host, k_host + pq, hp.begin());
            } else {
                for (auto& z : hp) { z.re = 0; z.im = 0; }
                const int sr = mode == CONV2D_SAME ? (krows - 1) / 2 : mode == CONV2D_VALID ? krows - 1 : 0;
                const int sc = mode == CONV2D_SAME ? (kcols - 1) / 2 : mode == CONV2D_VALID ? kcols - 1 : 0;
                for (int i = 0; i < krows; i++)
                    for (int j = 0; j < kcols; j++)
                        hp[(size_t)((i - sr + P) % P) * Q + (size_t)((j - sc + Q) % Q)] = k_host[(size_t)i * kcols + j];
            }
            H = (cpx<T>*)rt->dmalloc(pq * SZ);
            if (!H) return false;
            rt->h2d(H, hp.data(), pq * SZ);
            if (mode != CONV2D_SPECTRUM) {
                Plan2D<T, RT> once;
                if (!once.build(rt, P, Q, -1, 1)) return false;
                once.execute(H, H, 1);  // the kernel's spectrum, once
            }
        }
        ok = true;
        const int big = rows > out_rows ? rows : out_rows;
        if (P >= 8 && Q >= V && round.build(rt, ilog2(P), Q, n_matrices, min_seg_bytes)) {
            rowp.wants_hooks = true;
            if (rowp.build(rt, ilog2(Q), ALGO_AUTO, big * n_matrices) && rowp.hook_capable()) {
                work1 = (cpx<T>*)rt->dmalloc((size_t)n_matrices * (size_t)rows * (size_t)Q * SZ);
                work2 = (cpx<T>*)rt->dmalloc((size_t)n_matrices * (size_t)out_rows * (size_t)Q * SZ);
                if (!work1 || !work2) { ok = false; return false; }
            }
        }
        if (!fusable() && !ensure_fallback()) { ok = false; return false; }
        return true;
    }

    bool ensure_fallback() {
        if (fwd && inv && fwork) return true;
        if (!fwd) {
            fwd = new Plan2D<T, RT>();
            if (!fwd->build(rt, P, Q, -1, n_matrices)) { delete fwd; fwd = nullptr; return false; }
        }
        if (!inv) {
            inv = new Plan2D<T, RT>();
            if (!inv->build(rt, P, Q, 1, n_matrices)) { delete inv; inv = nullptr; return false; }
        }
        if (!fwork) fwork = (cpx<T>*)rt->dmalloc((size_t)n_matrices * (size_t)P * (size_t)Q * SZ);
        return fwork != nullptr;
    }

    // x: the images (x_pitch elements apart; 0: rows * cols); y: the outputs (y_pitch apart; 0: out_rows * out_cols), overlapping x
    // nowhere.  0 / -1 (bad arguments or a failed allocation: nothing is launched)
    int execute(const cpx<T>* x, long long x_pitch, cpx<T>* y, long long y_pitch) {
        if (!ok || !x || !y) return -1;
        const long long xm = (long long)rows * cols, ym = (long long)out_rows * out_cols;
        if (x_pitch == 0) x_pitch = xm;
        if (y_pitch == 0) y_pitch = ym;
        if (x_pitch < xm || y_pitch < ym) return -1;
        const int M = n_matrices;
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)((long long)(M - 1) * x_pitch + xm) * SZ;
        const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (size_t)((long long)(M - 1) * y_pitch + ym) * SZ;
        if (x0 < y1 && y0 < x1) return -1;
        const unsigned per_block = 256 * BLU_PER_THREAD;
        if (fused()) {
            const unsigned bpr_q = (unsigned)(((long long)Q + per_block - 1) / per_block);
            // 1: rows forward, x -> work1 [M][rows][Q]
            const bool x_contig = x_pitch == xm, y_contig = y_pitch == ym;
            if ((x0 & 15) == 0 && (x_contig || (x_pitch % V) == 0)) {
                ExecHooks<T> f;
                f.n_in = cols; f.in_pitch = cols;
                if (x_contig) {
                    rowp.execute_hooked(x, work1, rows * M, false, f);
                } else {
                    for (int m = 0; m < M; m++) rowp.execute_hooked(x + (long long)m * x_pitch, work1 + (size_t)m * rows * Q, rows, false, f);
                }
            } else {
                for (int m = 0; m < M; m++)
                    rt->launch(fftk::pad_mul_kernel<T>, (long long)bpr_q * rows, 256, (size_t)0, x + (long long)m * x_pitch, (long long)cols, cols,
                               (const cpx<T>*)nullptr, (int)fftk::HOOK_NONE, work1 + (size_t)m * rows * Q, Q, bpr_q);
                rowp.execute(work1, work1, rows * M, false);
            }
            // 2: column round, work1 -> work2 [M][out_rows][Q]
            round.run(work1, rows, H, work2, out_rows, M);
            // 3: rows inverse, work2 -> y
            if ((y0 & 15) == 0 && (y_contig || (y_pitch % V) == 0)) {
                ExecHooks<T> g;
                g.n_out = out_cols; g.out_pitch = out_cols;
                if (y_contig) {
                    rowp.execute_hooked(work2, y, out_rows * M, true, g);
                } else {
                    for (int m = 0; m < M; m++) rowp.execute_hooked(work2 + (size_t)m * out_rows * Q, y + (long long)m * y_pitch, out_rows, true, g);
                }
            } else {
                rowp.execute(work2, work2, out_rows * M, true);
                const unsigned bpr_o = (unsigned)(((long long)out_cols + per_block - 1) / per_block);
                for (int m = 0; m < M; m++)
                    rt->launch(fftk::mul_store_kernel<T>, (long long)bpr_o * out_rows, 256, (size_t)0, (const cpx<T>*)(work2 + (size_t)m * out_rows * Q), (long long)Q,
                               (const cpx<T>*)nullptr, 0ll, (int)fftk::HOOK_NONE, y + (long long)m * y_pitch, (long long)out_cols, out_cols, (T)1, bpr_o);
            }
            return 0;
        }
        if (!ensure_fallback()) return -1;
        const long long pq = (long long)P * Q;
        const int log2P = ilog2(P), log2Q = ilog2(Q);
        launch_flat(rt, fftk::conv2d_pad_kernel<T>, pq * M, x, x_pitch, rows, cols, fwork, log2P, log2Q, pq * M);
        fwd->execute(fwork, fwork, M);
        const unsigned bpr = (unsigned)((pq + per_block - 1) / per_block);
        rt->launch(fftk::mul_store_kernel<T>, (long long)bpr * M, 256, (size_t)0, (const cpx<T>*)fwork, pq, (const cpx<T>*)H, 0ll, (int)fftk::HOOK_MUL, fwork, pq,
                   (int)pq, (T)1, bpr);
        inv->execute(fwork, fwork, M);
        launch_flat(rt, fftk::conv2d_crop_kernel<T>, ym * M, (const cpx<T>*)fwork, log2P, log2Q, y, y_pitch, out_rows, out_cols, ym * M);
        return 0;
    }
};

// ---------------------------------------------------------------------------
// Two-signal statistics on the same frames: cross-spectral density, magnitude-squared coherence, H1 transfer estimate (scipy's
// csd / coherence; what the reference's compute_coherence, applications/power_spectrum.c:195-224, leaves as a placeholder).
//   pairs (x[s], y[s]), s < n_signals, of signal_len samples each, every side with its own base and pitch; frames, windows, nw and
//   P are FramesPlan's; X_w, Y_w the STFT rows of frame w, hb = n/2 + 1 bins; c_k = 1 / (sample_rate * P), doubled for 0 < k < n/2:
//       Pxx[k] = c_k mean_w |X_w[k]|^2,   Pyy[k] = c_k mean_w |Y_w[k]|^2,   Pxy[k] = c_k mean_w conj(X_w[k]) Y_w[k]
//   out: see fftk::frames_cross_finish_kernel (CROSS_CSD / COHERENCE / TRANSFER / ALL).
// The plan owns ONE FramesPlan in FRAMES_STFT mode, used unchanged (real or complex input, its fused path or its fallback), and runs
// it on x and on y into two row workspaces ([frames][hb] one-sided rows for real input, [frames][n] for complex input, of which
// bins 0 .. n/2 are read); frames_cross_partial_kernel then reduces chunks of C frames to double partial sums and
// frames_cross_finish_kernel sums the chunks and forms the output.
// The chunk length is a function of (nw, n_signals, hb) alone -- never of the grid or the device, so results do not depend on
// either: C = max(kMinChunk, ceil(nw / ceil(kTargetThreads / (n_signals * hb)))), chunks = ceil(nw / C).  kTargetThreads = 2^18
// threads (four waves per SIMD of a 256-CU device) for few long signals; C >= 32 frames keeps the partial sums (32 bytes per chunk
// and bin) at or below 1/16 of the rows they sum up.  Both figures are guesses until timed.
// ---------------------------------------------------------------------------
template <typename T, typename RT>
class CrossFramesPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr long long kTargetThreads = 1ll << 18;
    static constexpr int kMinChunk = 32;
    RT* rt = nullptr;
    FramesPlan<T, RT> inner;
    int out_kind = 0;
    int C = 0, chunks = 0;
    long long row_pitch = 0;    // elements between the rows of a workspace
    cpx<T>* rows_x = nullptr;   // [frames][row_pitch]
    cpx<T>* rows_y = nullptr;
    double* part = nullptr;     // [n_signals][chunks][hb][4]
    int max_grid = 16384, block = 256;  // launch geometry of the two kernels (the results do not depend on it: tests vary it)
    bool ok = false;
    ~CrossFramesPlan() {
        if (!rt) return;
        rt->dfree(rows_x); rt->dfree(rows_y); rt->dfree(part);
    }
    template <class F> void each_core(F&& f) { inner.each_core(f); }
    void set_no_fusion(bool v) { inner.set_no_fusion(v); }
    static int chunk_len(int nw, int n_signals, int hb) {
        const long long per_chunk = (long long)n_signals * hb;
        const long long want = (kTargetThreads + per_chunk - 1) / per_chunk;
        const long long c = ((long long)nw + want - 1) / want;
        return c < kMinChunk ? kMinChunk : (int)c;
    }
    int bins() const { return inner.bins(); }
    size_t rows_bytes() const { return (size_t)inner.frames() * (size_t)row_pitch * SZ; }
    size_t part_bytes() const { return (size_t)inner.n_signals * (size_t)chunks * (size_t)bins() * 4 * sizeof(double); }
    // values of T per (pair, bin) of the output
    int out_width() const { return out_kind == fftk::CROSS_COHERENCE ? 1 : out_kind == fftk::CROSS_ALL ? 4 : 2; }

    bool build(RT* runtime, int n, int hop, int signal_len, int n_signals, int window, const T* w_host, int out_kind_, bool real_input) {
        rt = runtime; out_kind = out_kind_;
        if (out_kind < fftk::CROSS_CSD || out_kind > fftk::CROSS_ALL) return false;
        if (!inner.build(rt, n, hop, signal_len, n_signals, window, w_host, FRAMES_STFT, real_input)) return false;
        if (!(inner.window_power > 0.0L)) return false;
        C = chunk_len(inner.nw, n_signals, bins());
        chunks = (inner.nw + C - 1) / C;
        row_pitch = real_input ? bins() : n;
        rows_x = (cpx<T>*)rt->dmalloc(rows_bytes());
        rows_y = (cpx<T>*)rt->dmalloc(rows_bytes());
        part = (double*)rt->dmalloc(part_bytes());
        if (!rows_x || !rows_y || !part) return false;
        ok = true;
        return true;
    }

    template <class K, class... A>
    void launch(K kernel, long long total, A... args) {
        long long g = (total + block - 1) / block;
        if (g > max_grid) g = max_grid;
        if (g < 1) g = 1;
        rt->launch(kernel, g, block, (size_t)0, args...);
    }

    // x, y: the signals of every pair (pitches in elements -- reals for real input; 0: signal_len); x == y is legal; out must
    // overlap neither.  0 / -1 (bad arguments: nothing is launched)
    int execute(const void* x, long long x_pitch, const void* y, long long y_pitch, void* out, double sample_rate) {
        if (!ok || !x || !y || !out) return -1;
        if (x_pitch == 0) x_pitch = inner.signal_len;
        if (y_pitch == 0) y_pitch = inner.signal_len;
        if (x_pitch < inner.signal_len || y_pitch < inner.signal_len) return -1;
        const long long S = inner.n_signals;
        const int hb = bins();
        const size_t esz = inner.real_input ? sizeof(T) : (size_t)SZ;
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)S * hb * out_width() * sizeof(T);
        const uintptr_t in[2] = {(uintptr_t)x, (uintptr_t)y};
        const long long pitch[2] = {x_pitch, y_pitch};
        for (int i = 0; i < 2; i++) {
            const uintptr_t i1 = in[i] + (size_t)((S - 1) * pitch[i] + inner.signal_len) * esz;
            if (o0 < i1 && in[i] < o1) return -1;
        }
        if (inner.execute((const cpx<T>*)x, x_pitch, rows_x, 1.0) != 0) return -1;
        if (inner.execute((const cpx<T>*)y, y_pitch, rows_y, 1.0) != 0) return -1;
        const double base = (double)(1.0L / ((long double)sample_rate * inner.window_power));
        const long long tp = S * chunks * hb;
        launch(fftk::frames_cross_partial_kernel<T>, tp, (const cpx<T>*)rows_x, (const cpx<T>*)rows_y, row_pitch, part, inner.nw, hb, C, chunks, tp);
        launch(fftk::frames_cross_finish_kernel<T>, S * hb, (const double*)part, (T*)out, inner.nw, hb, chunks, base, out_kind, S * hb);
        return 0;
    }
};

// ---------------------------------------------------------------------------
// Real 2D transforms of row-major images, numpy's rfft2 / irfft2 (the reference's applications/image_fft.c:35-60 starts from real
// pixels and widens them to complex by hand):
//   forward  X = rfft2(x):  x [M][rows][cols] real -> X [M][rows][cols/2 + 1] complex, unscaled
//   inverse  x = irfft2(X, s = (rows, cols)): a full complex inverse transform along the columns of all cols/2 + 1 columns, then a c2r
//            along the rows (which ignores the imaginary parts of bins 0 and -- even cols -- cols/2 of every row, like numpy.fft.irfft),
//            scaled ONCE by 1 / (rows * cols), like Plan2D: irfft2(rfft2(x)) = x, and input that is not Hermitian-consistent gives
//            what numpy gives.
// Matrices lie in_pitch / out_pitch elements apart (reals on the real side, complex values on the spectral side; 0: dense); the rows
// of a matrix are dense.  Input and output must not overlap; the input is never written.
//
// Fused path: two launches on half-size data.  L = cols/2, hb = L + 1, P = rows.
//   forward  1  rows     ONE launch of the hooked single-pass rows kernel over rows * M frames of cols reals (tile_fft_kernel's HOOKBIT_REAL:
//                        packed real load where the image lies -- any base, any matrix pitch -- r2c split in the store) -> the one-sided
//                        rows of the work image [M][rows][ld], ld = L + V: its rows are 16-byte aligned
//            2  columns  tile_fft_colpass_kernel over hb live columns: 16-byte loads from the work image, stores straight into the
//                        caller's [M][rows][hb] (value by value in fp32, where those rows are only 8-byte aligned)
//   inverse  1  columns  tile_fft_colpass_kernel, inverse, scale 1 / P: the caller's X (value by value in fp32) -> work image
//                        [M][rows][hb] -- the pitch the Hermitian rows load reads (execute_iframes fixes it at L + 1)
//            2  rows     ONE launch of the hooked rows kernel with HOOKBIT_HERM, inverse, scale 1 / L -> the real rows, straight into the
//                        caller's x where that is dense and 16-byte aligned; otherwise into an image of the plan's own and from there
//                        by real2d_copy_kernel (a third launch: the rows kernel stores 16 bytes at a time)
// taken where cols is a power of two whose half fits ONE hook-capable pass (FramesPlan's criterion: core.round_capable() and
// frames_exact(), up to kLmax), rows is a power of two with a one-pass column tile of E = 8 (rows >= 8) and row segments of at least
// min_seg_bytes = 64 bytes (ColRoundStep's criterion).
// Fallback (everything else and no_fusion; correct, not tuned): RealPlan on the rows (odd cols: its promoted path), then -- rows > 1 --
// transpose_kernel, AnyPlan of length rows on the hb * M transposed columns, transpose_kernel; the inverse runs the same steps in
// reverse, and real2d_real_ends_kernel first zeroes the imaginary parts a c2r ignores (RealPlan's merge reads them).  Everything goes through images of the plan's own (the input stays untouched, RealPlan sees dense 16-byte aligned rows);
// real2d_copy_kernel moves matrices to or from a caller's buffer that has a pitch of its own or is not 16-byte aligned.  Its plans
// and images are made at the first execute that needs them.
// ---------------------------------------------------------------------------

// one run of the column stages as a step of its own: P rows, n_cols live columns, separate pitches on the two sides
template <typename T, typename RT>
class ColPassStep {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr int V = 16 / SZ;
    RT* rt = nullptr;
    Pow2Plan<T, RT> colp;  // build_columns: the tile and the stage tables
    int log2P = 0, n_cols = 0, n_ct = 0;
    bool ok = false;
    template <class F> void each_core(F&& f) {
        if (colp.ok) f(&colp);
    }
    // the tile is that of the n_cols - 1 columns before the last (rounded down to the 16-byte lane access): for the L + 1 columns of
    // a real image's row spectra C divides L, and the last tile of every matrix holds exactly one live column
    bool build(RT* runtime, int log2P_, int n_cols_, int n_matrices, int min_seg_bytes) {
        rt = runtime; log2P = log2P_; n_cols = n_cols_;
        int tc = (n_cols - 1) / V * V;
        if (tc < V) tc = V;
        if (n_cols < 1 || !colp.build_columns(rt, log2P, tc, n_matrices)) return false;
        const PassDesc& a = colp.passes[0];
        n_ct = (int)((n_cols + (1ll << a.log2C) - 1) >> a.log2C);
        ok = a.E == 8 && a.log2H == 0 && a.nthreads <= 512 && a.seg_bytes >= min_seg_bytes;
        return ok;
    }
    int tile_cols() const { return ok ? 1 << colp.passes[0].log2C : 0; }
    // out[m][K][c] = scale * sum_l in[m][l][c] W_P^(+-K l), c < n_cols.  vec: base, row pitch and matrix pitch of that side are
    // multiples of 16 bytes
    void run(const cpx<T>* in, long long in_ld, long long in_b, bool in_vec, cpx<T>* out, long long out_ld, long long out_b, bool out_vec, int nm,
             bool inverse, T scale) {
        const PassDesc& a = colp.passes[0];
        fftk::ColPassParams<T> q;
        memset(&q, 0, sizeof(q));
        q.in = in; q.out = out; q.tables = colp.pass_tables[0];
        q.group_bytes = a.group_bytes; q.tables_bytes = a.tables_elems * SZ; q.off_tables = a.off_tables; q.o_sb = a.o_sb; q.sa_bits = a.sa_bits;
        q.log2L = a.log2L; q.log2C = a.log2C; q.n_ct = n_ct; q.n_cols = n_cols;
        q.in_b = in_b; q.out_b = out_b; q.in_ld = in_ld; q.out_ld = out_ld;
        q.n_tiles = (long long)nm * n_ct;
        q.in_vec = in_vec ? 1 : 0; q.out_vec = out_vec ? 1 : 0;
        q.inverse = inverse ? 1 : 0;
        q.nt = a.seg_bytes >= 128 ? 3 : 0;  // the tile passes' rule (Pow2Plan::pass_params): whole 128-byte lines only; not measured here
        q.scale = scale;
        int per_cu = rt->max_blocks_per_cu(fftk::tile_fft_colpass_kernel<T>, a.nthreads, (size_t)a.smem_bytes);
        if (per_cu < 1) per_cu = 1;
        long long grid = (long long)rt->num_cus() * per_cu;
        if (grid > q.n_tiles) grid = q.n_tiles;
        rt->launch(fftk::tile_fft_colpass_kernel<T>, grid, a.nthreads, (size_t)a.smem_bytes, q);
    }
};

template <typename T, typename RT>
class Real2DPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr int V = 16 / SZ;
    // the longest half-row the fused path takes: what the hooked rows kernel's HOOKBIT_REAL and HOOKBIT_HERM are checked at (the real frames plans' tests
    // stop at frames of 8192 reals in fp32, 4096 in fp64).  A device whose LDS holds one pass of 4096 fp64 points still takes the
    // fallback there, as FilterPlan does beyond its kNmax
    static constexpr int kLmax = SZ == 8 ? 4096 : 2048;
    RT* rt = nullptr;
    int rows = 0, cols = 0, n_matrices = 0;
    bool forward = true;           // r2c
    int L = 0, hb = 0;             // cols / 2, cols / 2 + 1
    long long ld = 0;              // fused: elements between the rows of the work image
    Pow2Plan<T, RT> core;          // fused: length L, hooked
    ColPassStep<T, RT> cstep;
    cpx<T>* wtab = nullptr;        // fused: W_cols^k, k <= L (the split's / merge's table)
    cpx<T>* work = nullptr;        // fused: [M][rows][ld]
    T* rout = nullptr;             // fused inverse: [M][rows][cols] for a caller's x the rows kernel cannot store to (made at its first use)
    RealPlan<T, RT>* rp = nullptr; // fallback (made at its first use)
    AnyPlan<T, RT>* colt = nullptr;
    cpx<T>* fwork = nullptr;       // fallback: [M][rows][hb]
    cpx<T>* tbuf = nullptr;        // fallback: [M][hb][rows]
    T* rstage = nullptr;           // fallback: [M][rows][cols] (made at its first use)
    int min_seg_bytes = 64;        // the fused path's row-segment criterion (tests narrow it to reach narrow tiles)
    bool ok = false;
    bool no_fusion = false;
    ~Real2DPlan() {
        delete rp;
        delete colt;
        if (!rt) return;
        rt->dfree(wtab); rt->dfree(work); rt->dfree(rout); rt->dfree(fwork); rt->dfree(tbuf); rt->dfree(rstage);
    }
    template <class F> void each_core(F&& f) {
        if (core.ok) f(&core);
        cstep.each_core(f);
        if (rp) rp->each_core(f);  // (the fallback's plans: once the build or an execute has made them)
        if (colt) colt->each_core(f);
    }
    void set_no_fusion(bool v) { no_fusion = v; }
    long long frames() const { return (long long)rows * n_matrices; }
    bool fusable() const { return ok && cstep.ok && core.ok && core.round_capable() && core.frames_exact(frames(), rows) && work && wtab; }
    bool fused() const { return fusable() && !no_fusion; }
    // what fft_gpu_plan_info_hip reports: 2 launches fused; on the fallback its steps (the row plan; transpose, column plan, transpose;
    // the copies and the inverse's zeroing of the ignored imaginary parts are not counted)
    int passes() const { return fused() ? 2 : rows > 1 ? 4 : 1; }
    size_t real_bytes() const { return (size_t)n_matrices * (size_t)rows * (size_t)cols * sizeof(T); }
    size_t spec_bytes() const { return (size_t)n_matrices * (size_t)rows * (size_t)hb * SZ; }

    bool build(RT* runtime, int rows_, int cols_, int n_matrices_, bool r2c, int min_seg = 64) {
        rt = runtime; rows = rows_; cols = cols_; n_matrices = n_matrices_; forward = r2c; min_seg_bytes = min_seg;
        if (rows < 1 || cols < 1 || n_matrices < 1 || (long long)rows * cols > (1ll << 30) || (long long)rows * n_matrices > 0x7fffffff ||
            (long long)cols * n_matrices > 0x7fffffff) return false;
        L = cols / 2; hb = L + 1;
        ok = true;
        const bool p2 = (rows & (rows - 1)) == 0 && (cols & (cols - 1)) == 0;
        if (p2 && rows >= 8 && cols >= 4 && L >= V && L <= kLmax && cstep.build(rt, ilog2(rows), hb, n_matrices, min_seg_bytes)) {
            core.wants_hooks = true;
            if (core.build(rt, ilog2(L), ALGO_AUTO, (int)frames()) && core.round_capable() && core.frames_exact(frames(), rows)) {
                // forward: the rows kernel writes at any pitch, so the rows of the work image are 16-byte aligned; inverse: the
                // Hermitian rows load reads rows of L + 1 bins and nothing else
                ld = forward ? (long long)L + V : (long long)hb;
                std::vector<cpx<T>> t;
                make_twiddle_table<T>(t, cols, (long long)L + 1, 1);
                wtab = (cpx<T>*)rt->dmalloc(t.size() * SZ);
                work = (cpx<T>*)rt->dmalloc((size_t)n_matrices * (size_t)rows * (size_t)ld * SZ);
                if (!wtab || !work) { ok = false; return false; }
                rt->h2d(wtab, t.data(), t.size() * SZ);
            }
        }
        if (!fusable() && !ensure_fallback()) { ok = false; return false; }
        return true;
    }

    bool ensure_fallback() {
        if (!rp) {
            rp = new RealPlan<T, RT>();
            if (!rp->build(rt, cols, forward, (int)frames())) { delete rp; rp = nullptr; return false; }
        }
        if (!fwork) fwork = (cpx<T>*)rt->dmalloc(spec_bytes());
        if (!fwork) return false;
        if (rows > 1) {
            if (!colt) {
                colt = new AnyPlan<T, RT>();
                if (!colt->build(rt, rows, forward ? -1 : 1, hb * n_matrices)) { delete colt; colt = nullptr; return false; }
            }
            if (!tbuf) tbuf = (cpx<T>*)rt->dmalloc(spec_bytes());
            if (!tbuf) return false;
        }
        return true;
    }

    template <typename E>
    void copy(const E* src, long long src_pitch, E* dst, long long dst_pitch, long long per) {
        launch_flat(rt, fftk::real2d_copy_kernel<E>, per * n_matrices, src, src_pitch, dst, dst_pitch, per, per * n_matrices);
    }
    void transpose(const cpx<T>* in, cpx<T>* out, int r, int c) {
        const long long tiles = (long long)n_matrices * ((r + 31) / 32) * ((c + 31) / 32);
        const long long grid = tiles > 65536 ? 65536 : tiles;
        rt->launch(fftk::transpose_kernel<T>, grid, 256, (size_t)(32 * 33 * SZ), in, out, r, c, tiles);
    }

    // forward: in = x (reals), out = X; inverse: in = X, out = x.  Pitches in elements of their own side; 0: dense.  0 / -1 (the
    // wrong direction, bad arguments or a failed allocation: nothing is launched)
    int execute(const void* in, long long in_pitch, void* out, long long out_pitch) {
        if (!ok || !in || !out) return -1;
        const long long rm = (long long)rows * cols, sm = (long long)rows * hb;
        const long long im = forward ? rm : sm, om = forward ? sm : rm;
        const size_t isz = forward ? sizeof(T) : (size_t)SZ, osz = forward ? (size_t)SZ : sizeof(T);
        if (in_pitch == 0) in_pitch = im;
        if (out_pitch == 0) out_pitch = om;
        if (in_pitch < im || out_pitch < om) return -1;
        const int M = n_matrices;
        const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (size_t)((long long)(M - 1) * in_pitch + im) * isz;
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)((long long)(M - 1) * out_pitch + om) * osz;
        if (i0 < o1 && o0 < i1) return -1;
        const bool in_dense = in_pitch == im, out_dense = out_pitch == om;
        const T* x_in = (const T*)in;
        const cpx<T>* X_in = (const cpx<T>*)in;
        T* x_out = (T*)out;
        cpx<T>* X_out = (cpx<T>*)out;
        if (fused()) {
            if (forward) {
                ExecHooks<T> f = frame_hooks<T>(nullptr, fftk::HOOK_NONE, L, cols);
                f.frames_per_signal = rows; f.signal_pitch = in_pitch;
                f.real_frames = true; f.post_tab = wtab; f.out_pitch = ld;
                core.execute_frames(reinterpret_cast<const cpx<T>*>(x_in), work, (int)frames(), f);
                const bool ovec = (o0 & 15) == 0 && (hb % V) == 0 && (out_pitch % V) == 0;  // fp64: every bin is 16 bytes
                cstep.run(work, ld, (long long)rows * ld, true, X_out, hb, out_pitch, ovec, M, false, (T)1);
            } else {
                const bool direct = out_dense && (o0 & 15) == 0;
                if (!direct && !rout) rout = (T*)rt->dmalloc(real_bytes());
                if (!direct && !rout) return -1;
                const bool ivec = (i0 & 15) == 0 && (hb % V) == 0 && (in_pitch % V) == 0;
                cstep.run(X_in, hb, in_pitch, ivec, work, ld, (long long)rows * ld, (ld % V) == 0, M, true, (T)(1.0L / (long double)rows));
                ExecHooks<T> g;
                g.pre_tab = wtab;
                core.execute_iframes(work, reinterpret_cast<cpx<T>*>(direct ? x_out : rout), (int)frames(), g);
                if (!direct) copy<T>(rout, rm, x_out, out_pitch, rm);
            }
            return 0;
        }
        if (!ensure_fallback()) return -1;
        const int nf = (int)frames();
        if (forward) {
            const T* src = x_in;
            if (!in_dense || (i0 & 15) != 0) {
                if (!rstage) rstage = (T*)rt->dmalloc(real_bytes());
                if (!rstage) return -1;
                copy<T>(x_in, in_pitch, rstage, rm, rm);
                src = rstage;
            }
            if (rows == 1) {
                rp->execute_r2c(src, out_dense ? X_out : fwork, nf);
            } else {
                rp->execute_r2c(src, fwork, nf);
                transpose(fwork, tbuf, rows, hb);
                colt->execute(tbuf, tbuf, hb * M);
                transpose(tbuf, out_dense ? X_out : fwork, hb, rows);
            }
            if (!out_dense) copy<cpx<T>>(fwork, sm, X_out, out_pitch, sm);
        } else {
            const bool direct = out_dense && (o0 & 15) == 0;
            if (!direct && !rstage) rstage = (T*)rt->dmalloc(real_bytes());
            if (!direct && !rstage) return -1;
            if (rows > 1) {
                const cpx<T>* src = X_in;
                if (!in_dense) {
                    copy<cpx<T>>(X_in, in_pitch, fwork, sm, sm);
                    src = fwork;
                }
                transpose(src, tbuf, rows, hb);
                colt->execute(tbuf, tbuf, hb * M);
                transpose(tbuf, fwork, hb, rows);
            } else {
                copy<cpx<T>>(X_in, in_pitch, fwork, sm, sm);
            }
            // RealPlan's c2r uses the imaginary parts of bins 0 and cols/2 of a row; numpy's ignores them
            launch_flat(rt, fftk::real2d_real_ends_kernel<T>, (long long)nf, fwork, hb, (cols & 1) == 0 ? 1 : 0, (long long)nf);
            rp->execute_c2r(fwork, direct ? x_out : rstage, nf);
            if (!direct) copy<T>(rstage, rm, x_out, out_pitch, rm);
        }
        return 0;
    }
};

// ---------------------------------------------------------------------------
// Cosine and sine transforms of types II and III of batched real rows, scipy.fft's dct / idct / dst / idst (the reference's
// applications/image_fft.c names the DCT as the transform behind image compression and has none):
//   DCT-II   X[k] = 2 sum_n x[n] cos(pi k (2n+1) / 2N)          DCT-III  y[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)
//   DST-II   X[k] = 2 sum_n x[n] sin(pi (k+1)(2n+1) / 2N)       DST-III  y[n] = (-1)^n X[N-1] + 2 sum_{k<N-1} X[k] sin(pi (2n+1)(k+1) / 2N)
// norm: NONE as above; INVERSE times 1 / (2N) (DCT-III INVERSE = scipy's idct of type 2); ORTHO scipy's norm = "ortho" (the odd index
// out is k = 0 for the cosine and k = N - 1 for the sine transforms).  The factors live in the plan's tables, made in long double and
// rounded once.  Rows lie in_pitch / out_pitch reals apart (0: dense), at any sizeof(T)-aligned base.
//
// Fused path: ONE launch of dct_rows_kernel (fft_kernels_dct.h) for all rows, one HBM round trip of N reals per row, in place
// allowed.  Taken where N is a power of two, a row is at least 64 bytes (N >= 16 fp32, 8 fp64) and L = N/2 fits ONE hook-capable pass
// of the rows kernel up to kLmax (Real2DPlan's cap: what the real frames tests check).
// Fallback (everything else, any N >= 1, and no_fusion; correct, not tuned): Makhoul's algorithm on a length-N complex transform --
// dct_pre_kernel (permute, or twiddle into the Hermitian spectrum), AnyPlan on a work image of the plan's own, dct_post_kernel.
// ---------------------------------------------------------------------------
enum { DCT_II = 0, DCT_III = 1, DST_II = 2, DST_III = 3 };
enum { DCT_NORM_NONE = 0, DCT_NORM_INVERSE = 1, DCT_NORM_ORTHO = 2 };

template <typename T, typename RT>
class DctPlan {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr int V = 16 / SZ;
    static constexpr int kLmax = Real2DPlan<T, RT>::kLmax;
    RT* rt = nullptr;
    int n = 0, batch = 0, type = 0, norm = 0;
    int L = 0;
    Pow2Plan<T, RT> core;           // fused: length L, the tile and the stage tables of the hooked rows kernel
    cpx<T>* ta = nullptr;           // fused: fftk::DctParams::ta / tb
    cpx<T>* tb = nullptr;
    AnyPlan<T, RT>* full = nullptr; // fallback (made at its first use): length n
    cpx<T>* ftab = nullptr;         // fallback: [n]
    cpx<T>* work = nullptr;         // fallback: [batch][n]
    bool ok = false;
    bool no_fusion = false;
    ~DctPlan() {
        delete full;
        if (!rt) return;
        rt->dfree(ta); rt->dfree(tb); rt->dfree(ftab); rt->dfree(work);
    }
    template <class F> void each_core(F&& f) {
        if (core.ok) f(&core);
        if (full) full->each_core(f);
    }
    void set_no_fusion(bool v) { no_fusion = v; }
    bool inverse() const { return (type & 1) != 0; }
    bool sine() const { return (type & 2) != 0; }
    bool fusable() const { return ok && core.ok && core.round_capable() && ta && tb; }
    bool fused() const { return fusable() && !no_fusion; }

    // f_k (forward: on output k) or g_k (inverse: on input k) of the cosine transform the plan runs; k = 0 is ORTHO's odd index out
    long double factor(int k) const {
        const long double N = (long double)n;
        if (norm == DCT_NORM_INVERSE) return 1.0L / (2.0L * N);
        if (norm == DCT_NORM_ORTHO) {
            if (inverse()) return k == 0 ? 1.0L / sqrtl(N) : 1.0L / sqrtl(2.0L * N);
            return k == 0 ? 1.0L / sqrtl(4.0L * N) : 1.0L / sqrtl(2.0L * N);
        }
        return 1.0L;
    }
    static cpx<T> rounded(long double re, long double im) {  // a table entry: made in long double, rounded once
        cpx<T> c;
        c.re = (T)re; c.im = (T)im;
        return c;
    }
    cpx<T>* upload(const std::vector<cpx<T>>& t) {
        cpx<T>* d = (cpx<T>*)rt->dmalloc(t.size() * SZ);
        if (d) rt->h2d(d, t.data(), t.size() * SZ);
        return d;
    }

    bool build(RT* runtime, int n_, int batch_, int type_, int norm_) {
        rt = runtime; n = n_; batch = batch_; type = type_; norm = norm_;
        if (n < 1 || batch < 1 || type < DCT_II || type > DST_III || norm < DCT_NORM_NONE || norm > DCT_NORM_ORTHO ||
            (long long)n * batch > 0x7fffffffll) return false;
        L = n / 2;
        ok = true;
        const long double pi = 3.141592653589793238462643383279502884L;
        if ((n & (n - 1)) == 0 && (size_t)n * sizeof(T) >= 64 && L <= kLmax) {
            core.wants_hooks = true;
            if (core.build(rt, ilog2(L), ALGO_AUTO, batch) && core.round_capable()) {
                std::vector<cpx<T>> a((size_t)L + 1), b((size_t)L + 1);
                for (int k = 0; k <= L; k++) {
                    const long double f = factor(k), tq = pi * k / (2.0L * n), tw = 2.0L * pi * k / n;
                    if (!inverse()) {  // qa = f q, qb = f q W / i
                        a[k] = rounded(f * cosl(tq), -f * sinl(tq));
                        b[k] = rounded(-f * sinl(tq + tw), -f * cosl(tq + tw));
                    } else {           // cq = g conj q, cw = conj W
                        a[k] = rounded(f * cosl(tq), f * sinl(tq));
                        b[k] = rounded(cosl(tw), sinl(tw));
                    }
                }
                ta = upload(a); tb = upload(b);
                if (!ta || !tb) { ok = false; return false; }
            }
        }
        if (!fusable() && !ensure_fallback()) { ok = false; return false; }
        return true;
    }

    bool ensure_fallback() {
        if (!full) {
            full = new AnyPlan<T, RT>();
            if (!full->build(rt, n, inverse() ? 1 : -1, batch)) { delete full; full = nullptr; return false; }
        }
        if (!ftab) {
            const long double pi = 3.141592653589793238462643383279502884L;
            std::vector<cpx<T>> t((size_t)n);
            for (int k = 0; k < n; k++) {
                const long double tq = pi * k / (2.0L * n);
                // forward: 2 f q;  inverse: n g conj q (AnyPlan's inverse carries 1 / n, Makhoul's is unscaled)
                const long double f = inverse() ? factor(k) * (long double)n : 2.0L * factor(k);
                t[k] = rounded(f * cosl(tq), (inverse() ? f : -f) * sinl(tq));
            }
            ftab = upload(t);
        }
        if (!work) work = (cpx<T>*)rt->dmalloc((size_t)batch * (size_t)n * SZ);
        return ftab && work;
    }

    // 0 / -1 (bad arguments or a failed allocation: nothing is launched)
    int execute(const T* in, long long in_pitch, T* out, long long out_pitch) {
        if (!ok || !in || !out) return -1;
        if (in_pitch == 0) in_pitch = n;
        if (out_pitch == 0) out_pitch = n;
        if (in_pitch < n || out_pitch < n) return -1;
        if (fused()) {
            const PassDesc& a = core.passes[0];
            fftk::DctParams<T> q;
            memset(&q, 0, sizeof(q));
            q.in = in; q.out = out; q.tables = core.pass_tables[0]; q.ta = ta; q.tb = tb;
            q.group_bytes = a.group_bytes; q.tables_bytes = a.tables_elems * SZ; q.off_tables = a.off_tables; q.o_sb = a.o_sb; q.sa_bits = a.sa_bits;
            q.log2L = a.log2L; q.log2C = a.log2C;
            q.in_pitch = in_pitch; q.out_pitch = out_pitch;
            q.n_rows = batch;
            q.n_tiles = ((long long)batch + (1ll << a.log2C) - 1) >> a.log2C;
            q.in_vec = (((uintptr_t)in & 15) == 0 && (in_pitch * (long long)sizeof(T)) % 16 == 0) ? 1 : 0;
            q.out_vec = (((uintptr_t)out & 15) == 0 && (out_pitch * (long long)sizeof(T)) % 16 == 0) ? 1 : 0;
            q.sine = sine() ? 1 : 0;
            if (inverse()) launch_rows(fftk::dct_rows_kernel<T, true>, q, a);
            else launch_rows(fftk::dct_rows_kernel<T, false>, q, a);
            return 0;
        }
        if (!ensure_fallback()) return -1;
        const long long total = (long long)batch * n;
        launch_flat(rt, fftk::dct_pre_kernel<T>, total, in, in_pitch, work, (const cpx<T>*)ftab, n, inverse() ? 1 : 0, sine() ? 1 : 0, total);
        full->execute(work, work, batch);
        launch_flat(rt, fftk::dct_post_kernel<T>, total, (const cpx<T>*)work, (const cpx<T>*)ftab, out, out_pitch, n, inverse() ? 1 : 0, sine() ? 1 : 0, total);
        return 0;
    }

  private:
    template <class K>
    void launch_rows(K kernel, const fftk::DctParams<T>& q, const PassDesc& a) {
        int per_cu = rt->max_blocks_per_cu(kernel, a.nthreads, (size_t)a.smem_bytes);
        if (per_cu < 1) per_cu = 1;
        long long grid = (long long)rt->num_cus() * per_cu;
        if (grid > q.n_tiles) grid = q.n_tiles;
        rt->launch(kernel, grid, a.nthreads, (size_t)a.smem_bytes, q);
    }
};

// ---------------------------------------------------------------------------
// The same transform along both axes of [M][rows][cols] real images, scipy's dctn / idctn over the last two axes.  Composition only:
// the row plan on the rows, transpose_real_kernel, the row plan of length `rows` on the transposed image, transpose back.  Matrices lie
// in_pitch / out_pitch reals apart (0: dense); the rows of a matrix are dense.  In place is allowed (everything in between happens in
// images of the plan's own).
// ---------------------------------------------------------------------------
template <typename T, typename RT>
class Dct2DPlan {
  public:
    RT* rt = nullptr;
    int rows = 0, cols = 0, n_matrices = 0;
    DctPlan<T, RT> rowp, colp;  // length cols on M * rows rows; length rows on M * cols rows
    T* t1 = nullptr;            // [M][rows][cols]
    T* t2 = nullptr;            // [M][cols][rows]
    bool ok = false;
    ~Dct2DPlan() {
        if (!rt) return;
        rt->dfree(t1); rt->dfree(t2);
    }
    template <class F> void each_core(F&& f) {
        rowp.each_core(f);
        colp.each_core(f);
    }
    void set_no_fusion(bool v) { rowp.set_no_fusion(v); colp.set_no_fusion(v); }
    bool fused() const { return rowp.fused() && colp.fused(); }
    bool build(RT* runtime, int rows_, int cols_, int n_matrices_, int type, int norm) {
        rt = runtime; rows = rows_; cols = cols_; n_matrices = n_matrices_;
        if (rows < 1 || cols < 1 || n_matrices < 1 || (long long)rows * cols > (1ll << 30) || (long long)rows * cols * n_matrices > 0x7fffffffll) return false;
        if (!rowp.build(rt, cols, rows * n_matrices, type, norm) || !colp.build(rt, rows, cols * n_matrices, type, norm)) return false;
        const size_t bytes = (size_t)n_matrices * (size_t)rows * (size_t)cols * sizeof(T);
        t1 = (T*)rt->dmalloc(bytes);
        t2 = (T*)rt->dmalloc(bytes);
        ok = t1 && t2;
        return ok;
    }
    void transpose(const T* in, long long in_b, T* out, long long out_b, int r, int c) {
        const long long tiles = (long long)n_matrices * ((r + 31) / 32) * ((c + 31) / 32);
        const long long grid = tiles > 65536 ? 65536 : tiles;
        rt->launch(fftk::transpose_real_kernel<T>, grid, 256, (size_t)(32 * 33 * sizeof(T)), in, in_b, out, out_b, r, c, tiles);
    }
    int execute(const T* in, long long in_pitch, T* out, long long out_pitch) {
        if (!ok || !in || !out) return -1;
        const long long rm = (long long)rows * cols;
        if (in_pitch == 0) in_pitch = rm;
        if (out_pitch == 0) out_pitch = rm;
        if (in_pitch < rm || out_pitch < rm) return -1;
        if (in_pitch != rm) {  // the row plan takes ONE pitch between rows: matrices with a pitch of their own are gathered first
            launch_flat(rt, fftk::real2d_copy_kernel<T>, rm * n_matrices, in, in_pitch, t1, rm, rm, rm * n_matrices);
            in = t1;
        }
        if (rowp.execute(in, cols, t1, cols) != 0) return -1;
        transpose(t1, rm, t2, rm, rows, cols);
        if (colp.execute(t2, rows, t2, rows) != 0) return -1;
        transpose(t2, rm, out, out_pitch, cols, rows);
        return 0;
    }
};

// ---------------------------------------------------------------------------
// 3D complex transform of n_volumes row-major [depth][rows][cols] volumes (cols fastest, contiguous), numpy's fftn / ifftn over the last
// three axes; in == out allowed.  Two steps: the 2D transform of the depth * n_volumes planes, then the transforms along depth in place
// on `out`.
//   planes, fused   rows and cols powers of two >= 8 whose tile fits the LDS budget with at most two strips per step, the layouts with the
//                   register prefetch (choose_plane; on the MI355X planes up to 8192 values in fp32, 4096 in fp64): ONE launch of
//                   plane_fft_kernel (fft_kernels_plane.h), in -> out, whole contiguous planes through LDS;
//   planes, composition (every other shape, and no_fusion)   Plan2D(rows, cols, depth * n_volumes), used unchanged -- correct for every
//                   shape >= 1 x 1 x 1, not tuned;
//   depth           the image [depth][rows * cols] of a volume: depth a power of two >= 2 and rows * cols a multiple of V: a column Pow2Plan
//                   with cols' = rows * cols (one pass, or build_columns2 under Plan2D::build's segment rule); any other depth > 1:
//                   transpose_kernel, a batched AnyPlan of length depth, transpose_kernel, in a workspace of the plan's own; depth = 1: nothing.
// smooth: what Plan2D takes (7-smooth lengths that are no power of two on the mixed-radix engine).
// The inverse is scaled ONCE by 1 / (depth * rows * cols): the plane step carries 1 / (rows * cols) -- in the store of plane_fft_kernel, or in
// Plan2D's two 1D inverses -- and the depth step 1 / depth, like every 1D inverse of the engine.
// Limits: depth * rows * cols <= 2^30, and the products the inner plans index with ints stay below 2^31 (Plan2D::build's, and the depth
// route's batch rows * cols * n_volumes).
// ---------------------------------------------------------------------------
template <typename T, typename RT>
class Plan3D {
  public:
    static constexpr int SZ = (int)sizeof(cpx<T>);
    static constexpr int V = 16 / SZ;
    static constexpr int kMinSeg = 64;  // Plan2D::build's default: below it the one-pass column tile gives way to build_columns2
    RT* rt = nullptr;
    int depth = 0, rows = 0, cols = 0, n_volumes = 0, dir = -1;
    bool smooth = false;
    // the plane kernel's tile (choose_plane) and its tables
    fftk::PlaneParams<T> pk;
    int pk_threads = 0, pk_smem = 0, pk_npf = 0;
    bool plane_ok = false;
    cpx<T>* ptab = nullptr;
    Plan2D<T, RT>* comp = nullptr;     // the composition's planes (made at the build where the plane kernel does not run, else at the first execute under no_fusion)
    Pow2Plan<T, RT>* dcol = nullptr;   // depth: strided column passes in place
    AnyPlan<T, RT>* dany = nullptr;    // or: batched 1D on the transposed volumes
    cpx<T>* tbuf = nullptr;            // [n_volumes][rows * cols][depth]
    bool ok = false;
    bool no_fusion = false;
    // take tiles without the register prefetch too (more than two strips per step).  Off: measured on the MI355X that layout loses to the
    // composition (128^3 fp32: 2.02 ms against 1.17 ms, profiles/fft3d_vs_composition.txt), the prefetched layouts win; the emulation's tests turn it on
    bool take_unprefetched = false;
    ~Plan3D() {
        delete comp;
        delete dcol;
        delete dany;
        if (!rt) return;
        rt->dfree(ptab); rt->dfree(tbuf);
    }
    template <class F> void each_core(F&& f) {
        if (comp) comp->each_core(f);
        if (dcol) f(dcol);
        if (dany) dany->each_core(f);
    }
    void set_no_fusion(bool v) { no_fusion = v; }
    bool fused() const { return ok && plane_ok && !no_fusion; }
    long long planes() const { return (long long)depth * n_volumes; }
    long long plane_elems() const { return (long long)rows * cols; }
    int tile_planes() const { return plane_ok ? 1 << pk.log2G : 0; }
    // launches per execute; exact for power-of-two and mixed-radix lengths, an estimate for a chirp-z transform inside a route (one kernel
    // where its padded length fits one tile, else its core's passes twice)
    static int any_launches(const AnyPlan<T, RT>* a) {
        if (!a) return 0;
        if (a->p2) return a->p2->passes.empty() ? 1 : (int)a->p2->passes.size();
        if (a->mr) return (int)a->mr->passes.size();
        if (!a->bl) return 0;
        const int c = a->bl->core.passes.empty() ? 1 : (int)a->bl->core.passes.size();
        return (a->bl->core.hook_capable() && a->bl->core.round_capable()) ? 1 : 2 * c;
    }
    int launches() const {
        int n = 0;
        if (fused()) n = 1;
        else if (comp) n = any_launches(&comp->rowp) + (comp->colp ? (int)comp->colp->passes.size() : comp->colt ? 2 + any_launches(comp->colt) : 0);
        else n = 2;  // (the composition is not made yet: its usual two)
        if (dcol) n += (int)dcol->passes.size();
        if (dany) n += 2 + any_launches(dany);
        return n;
    }
    size_t workspace_bytes() const {
        size_t b = 0;
        if (tbuf) b += (size_t)n_volumes * (size_t)depth * (size_t)plane_elems() * SZ;
        if (dcol) b += dcol->scratch_bytes;
        if (comp && comp->tbuf) b += (size_t)planes() * (size_t)plane_elems() * SZ;
        return b;
    }

    // The plane kernel's tile for this shape inside `budget` bytes of LDS (the rule of fft_kernels_plane.h); false: no plane kernel
    bool choose_plane(int budget) {
        if (rows < 8 || cols < 8 || (rows & (rows - 1)) != 0 || (cols & (cols - 1)) != 0 || cols * SZ < 64) return false;
        const int per_thread = 4 * V;  // values of a strip per thread
        const long long pe = plane_elems();
        int log2G = 0;  // small planes: several per tile, up to 256 threads' worth -- fewer where the budget asks for it
        while ((pe << (log2G + 1)) <= 256ll * per_thread && (2ll << log2G) <= planes()) log2G++;
        const int min_nt = (rows > cols ? rows : cols) / 4;
        const long long tables = (long long)(rows + cols) * SZ;
        long long tv = 0, image = 0, nt = 0;
        for (;; log2G--) {
            tv = pe << log2G;
            image = ((long long)rows << log2G) * ((long long)cols * SZ + 16);
            nt = tv / per_thread;
            if (nt > 512) nt = 512;
            while (nt >= min_nt && image + nt * per_thread * SZ + tables > budget) nt >>= 1;
            if (nt >= min_nt && nt >= 1) break;
            if (log2G == 0) return false;
        }
        memset(&pk, 0, sizeof(pk));
        pk.log2P = ilog2(rows); pk.log2Q = ilog2(cols); pk.log2G = log2G;
        pk.log2SR = ilog2(nt * per_thread / cols); pk.log2SC = ilog2(nt * per_thread / rows);
        pk.off_exch = (int)image; pk.off_tables = (int)(image + nt * per_thread * SZ); pk.tables_bytes = (int)tables;
        pk.n_planes = planes(); pk.n_tiles = (planes() + (1ll << log2G) - 1) >> log2G;
        pk.inverse = dir > 0 ? 1 : 0;
        pk.scale = dir > 0 ? (T)(1.0L / (long double)pe) : (T)1;
        pk_threads = (int)nt;
        pk_smem = (int)(image + nt * per_thread * SZ + tables);
        const long long chunks_per_thread = tv / V / nt;
        pk_npf = chunks_per_thread <= 8 ? (int)chunks_per_thread : 0;
        return true;
    }

    bool build(RT* runtime, int depth_, int rows_, int cols_, int dir_, int n_volumes_, bool smooth_ = false) {
        rt = runtime; depth = depth_; rows = rows_; cols = cols_; dir = dir_ < 0 ? -1 : 1; n_volumes = n_volumes_; smooth = smooth_;
        if (depth < 1 || rows < 1 || cols < 1 || n_volumes < 1) return false;
        const long long pe = plane_elems();
        if (pe * depth > (1ll << 30) || planes() > 0x7fffffff || planes() * rows > 0x7fffffff || planes() * cols > 0x7fffffff ||
            pe * n_volumes > 0x7fffffff) return false;
        if (choose_plane(rt->max_lds_bytes()) && (pk_npf > 0 || take_unprefetched)) {
            std::vector<cpx<T>> t, u;
            make_twiddle_table<T>(t, cols, cols, 1);
            make_twiddle_table<T>(u, rows, rows, 1);
            t.insert(t.end(), u.begin(), u.end());
            ptab = (cpx<T>*)rt->dmalloc(t.size() * SZ);
            if (!ptab) return false;
            rt->h2d(ptab, t.data(), t.size() * SZ);
            pk.tables = ptab;
            plane_ok = true;
        } else if (!ensure_composition()) {
            return false;
        }
        if (depth > 1) {
            if ((depth & (depth - 1)) == 0 && pe % V == 0) {
                dcol = new Pow2Plan<T, RT>();
                if (!dcol->build_columns(rt, ilog2(depth), (int)pe, n_volumes)) { delete dcol; dcol = nullptr; }
                if (!dcol || dcol->passes[0].seg_bytes < kMinSeg) {  // (Plan2D::build's rule for many rows)
                    Pow2Plan<T, RT>* two = new Pow2Plan<T, RT>();
                    if (two->build_columns2(rt, ilog2(depth), (int)pe, n_volumes)) {
                        delete dcol;
                        dcol = two;
                    } else {
                        delete two;
                    }
                }
            }
            if (!dcol) {
                dany = new AnyPlan<T, RT>();
                if (!dany->build(rt, depth, dir, (int)(pe * n_volumes), ALGO_AUTO, smooth)) return false;
                tbuf = (cpx<T>*)rt->dmalloc((size_t)n_volumes * (size_t)depth * (size_t)pe * SZ);
                if (!tbuf) return false;
            }
        }
        ok = true;
        return true;
    }

    bool ensure_composition() {
        if (comp) return true;
        comp = new Plan2D<T, RT>();
        if (!comp->build(rt, rows, cols, dir, (int)planes(), smooth)) { delete comp; comp = nullptr; return false; }
        return true;
    }

    void launch_planes(const cpx<T>* in, cpx<T>* out) {
        fftk::PlaneParams<T> q = pk;
        q.in = in; q.out = out;
        auto go = [&](auto kernel) {
            int per_cu = rt->max_blocks_per_cu(kernel, pk_threads, (size_t)pk_smem);
            if (per_cu < 1) per_cu = 1;
            long long grid = (long long)rt->num_cus() * per_cu;
            if (grid > q.n_tiles) grid = q.n_tiles;
            rt->launch(kernel, grid, pk_threads, (size_t)pk_smem, q);
        };
        if (pk_npf == 4) go(fftk::plane_fft_kernel<T, 4>);
        else if (pk_npf == 8) go(fftk::plane_fft_kernel<T, 8>);
        else go(fftk::plane_fft_kernel<T, 0>);
    }
    void transpose(const cpx<T>* in, cpx<T>* out, int r, int c) {
        const long long tiles = (long long)n_volumes * ((r + 31) / 32) * ((c + 31) / 32);
        const long long grid = tiles > 65536 ? 65536 : tiles;
        rt->launch(fftk::transpose_kernel<T>, grid, 256, (size_t)(32 * 33 * SZ), in, out, r, c, tiles);
    }

    // 0 / -1 (the composition could not be made: nothing is launched)
    int execute(const cpx<T>* in, cpx<T>* out) {
        if (!ok || !in || !out) return -1;
        if (fused()) {
            launch_planes(in, out);
        } else {
            if (!ensure_composition()) return -1;
            comp->execute(in, out, (int)planes());
        }
        if (dcol) {
            dcol->execute(out, out, n_volumes, dir > 0);
        } else if (dany) {
            transpose(out, tbuf, depth, (int)plane_elems());
            dany->execute(tbuf, tbuf, (int)(plane_elems() * n_volumes));
            transpose(tbuf, out, (int)plane_elems(), depth);
        }
        return 0;
    }
};

}  // namespace ffteng
