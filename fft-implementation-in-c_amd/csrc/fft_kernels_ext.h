// fft_kernels_ext.h -- the small kernels around the batched 1D engine that the "next" rows of the scope table need
// (SURVEY.md 8f): matrix transpose (2D transforms whose column length does not fit one LDS tile), the split /
// merge steps of real-input transforms, one-sided power spectra.  All HBM-bound element-wise or tiled copies.
#pragma once

#include "fft_kernels.h"

namespace fftk {

// out[b][c][r] = in[b][r][c]: 32 x 32 tiles through LDS (padded rows: no bank conflicts), coalesced on both sides.
// grid = batch * tiles_r * tiles_c workgroups of 256 threads (32 x 8).
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) transpose_kernel(const cpx<T>* in, cpx<T>* out, int rows, int cols, long long n_tiles) {
    FFT_DYN_SMEM(smem);
    cpx<T>* tile = reinterpret_cast<cpx<T>*>(smem);  // [32][33]
    const int tr = (rows + 31) / 32, tc = (cols + 31) / 32;
    const int tx = FFT_TID & 31, ty = FFT_TID >> 5;
    for (long long t = FFT_BID; t < n_tiles; t += FFT_NBLOCKS) {
        const long long b = t / ((long long)tr * tc);
        const int rem = (int)(t - b * (long long)tr * tc);
        const int r0 = (rem / tc) * 32, c0 = (rem % tc) * 32;
        const cpx<T>* src = in + b * (long long)rows * cols;
        cpx<T>* dst = out + b * (long long)rows * cols;
        FFT_SYNC();
        FFT_UNROLL
        for (int k = 0; k < 4; k++) {
            const int r = r0 + ty + 8 * k, c = c0 + tx;
            if (r < rows && c < cols) tile[(ty + 8 * k) * 33 + tx] = src[(long long)r * cols + c];
        }
        FFT_SYNC();
        FFT_UNROLL
        for (int k = 0; k < 4; k++) {
            const int c = c0 + ty + 8 * k, r = r0 + tx;
            if (r < rows && c < cols) dst[(long long)c * rows + r] = tile[tx * 33 + ty + 8 * k];
        }
    }
}

// Real input of even length n = 2 h, transformed as ONE complex transform of length h on z[j] = x[2j] + i x[2j+1]
// (the real array IS that complex array, no copy).  With Z = FFT_h(z):
//   E[k] = (Z[k] + conj(Z[h-k])) / 2          spectrum of the even samples
//   O[k] = (Z[k] - conj(Z[h-k])) / (2i)       spectrum of the odd samples        (Z[h] = Z[0])
//   X[k] = E[k] + W_n^k O[k],  k = 0 .. h      the n/2 + 1 non-redundant bins (reference include/fft_auto.h:88-96)
// w[k] = W_n^k = exp(-2 pi i k / n), k <= h, comes from a plan-time table.  z: [batch][h], x_out: [batch][h + 1].
// One thread per PAIR of bins (k, h - k), k = 0 .. h/2 (round 3: one thread per bin read every Z twice): with t = W_n^k O[k],
//   X[k] = E[k] + t,   X[h-k] = conj(E[k] - t)      (E[h-k] = conj E[k], O[h-k] = conj O[k], W_n^(h-k) = -conj W_n^k);
// k = 0 yields X[0] and X[h] from Z[0] alone, 2k = h a single bin.  `total` = batch * (h/2 + 1).
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) r2c_split_kernel(const cpx<T>* z, cpx<T>* x_out, const cpx<T>* w, int h, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    const int hp = h / 2 + 1;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long b = i / hp;
        const int k = (int)(i - b * hp);
        const cpx<T>* zb = z + b * h;
        cpx<T>* xb = x_out + b * (h + 1);
        const cpx<T> a = zb[k];
        const cpx<T> c0 = zb[k == 0 ? 0 : h - k];
        const cpx<T> c = mk<T>(c0.re, -c0.im);                                   // conj(Z[h-k])
        const cpx<T> e = cscale(cadd(a, c), (T)0.5);
        const cpx<T> o = mul_neg_i(cscale(csub(a, c), (T)0.5));                  // (a - c) / (2i)
        const cpx<T> t = cmul(w[k], o);
        xb[k] = cadd(e, t);
        if (2 * k != h) {
            const cpx<T> m = csub(e, t);
            xb[h - k] = mk<T>(m.re, -m.im);
        }
    }
}

// The inverse of the split: X[0..h] (Hermitian half spectrum of a real signal of even length n = 2h) -> Z[0..h-1] with
//   E[k] = (X[k] + conj(X[h-k])) / 2,  O[k] = (X[k] - conj(X[h-k])) / 2 * conj(W_n^k),  Z[k] = E[k] + i O[k],  Z[h-k] = conj(E[k] - i O[k])
// (one thread per pair, `total` = batch * (h/2 + 1)); the inverse complex transform of length h (scaled by 1/h like every inverse
// here) then returns the n real samples.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) c2r_merge_kernel(const cpx<T>* x_in, cpx<T>* z, const cpx<T>* w, int h, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    const int hp = h / 2 + 1;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long b = i / hp;
        const int k = (int)(i - b * hp);
        const cpx<T>* xb = x_in + b * (h + 1);
        cpx<T>* zb = z + b * h;
        const cpx<T> a = xb[k];
        const cpx<T> c0 = xb[h - k];
        const cpx<T> c = mk<T>(c0.re, -c0.im);
        const cpx<T> e = cscale(cadd(a, c), (T)0.5);
        const cpx<T> io = mul_pos_i(cmul_conj(cscale(csub(a, c), (T)0.5), w[k]));
        zb[k] = cadd(e, io);
        if (k != 0 && 2 * k != h) {
            const cpx<T> m = csub(e, io);
            zb[h - k] = mk<T>(m.re, -m.im);
        }
    }
}

// odd lengths: promote the real samples to complex / keep the real parts (the transform itself is then a plain
// complex one of length n, Bluestein for a non-power-of-two)
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) real_to_complex_kernel(const T* x, cpx<T>* z, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) z[i] = mk<T>(x[i], (T)0);
}
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) complex_to_real_kernel(const cpx<T>* z, T* x, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) x[i] = z[i].re;
}
// rows of `len_in` -> rows of `len_out` <= len_in (keep the first len_out of every row)
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) copy_rows_kernel(const cpx<T>* in, cpx<T>* out, int len_in, int len_out, long long total_out) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total_out; i += stride) {
        const long long b = i / len_out;
        out[i] = in[b * len_in + (i - b * len_out)];
    }
}
// Hermitian extension: rows of h + 1 bins -> rows of n bins, X[n - k] = conj(X[k])  (odd-length c2r)
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) hermitian_extend_kernel(const cpx<T>* half, cpx<T>* full, int n, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    const int hb = n / 2 + 1;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long b = i / n;
        const int k = (int)(i - b * n);
        cpx<T> v = half[b * hb + (k < hb ? k : n - k)];
        if (k >= hb) v.im = -v.im;
        full[i] = v;
    }
}

// One-sided power spectral density of a (windowed) spectrum: psd[k] = |X[k]|^2 * scale, doubled for 0 < k < n/2
// (reference applications/power_spectrum.c:73-80).  X: [batch][n], psd: [batch][n/2 + 1] real.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) psd_onesided_kernel(const cpx<T>* X, T* psd, int n, T scale, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    const int hb = n / 2 + 1;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long b = i / hb;
        const int k = (int)(i - b * hb);
        const cpx<T> v = X[b * n + k];
        T pw = (v.re * v.re + v.im * v.im) * scale;
        if (k > 0 && k < n / 2) pw *= (T)2;  // the reference's own condition (integer n / 2)
        psd[i] = pw;
    }
}

// The same for rows that already hold only their one-sided bins (the r2c split's rows of hb = n/2 + 1 bins, `pitch` elements apart):
// psd[b][k] = |X[b][k]|^2 * scale, doubled for 0 < k < hb - 1.  `total` = batch * hb.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) psd_onesided_rows_kernel(const cpx<T>* X, long long pitch, T* psd, int hb, T scale, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long b = i / hb;
        const int k = (int)(i - b * hb);
        const cpx<T> v = X[b * pitch + k];
        T pw = (v.re * v.re + v.im * v.im) * scale;
        if (k > 0 && k < hb - 1) pw *= (T)2;
        psd[i] = pw;
    }
}

// Real frames -> the packed complex rows a half-length transform reads (the unfused path of the real frames plan):
// z[f][m] = (x_f[2m] * win[m].re, x_f[2m+1] * win[m].im), m < h, where frame f = s * nw + w starts at real sample
// s * signal_pitch + w * hop of x and win[m] = (w[2m], w[2m+1]).  Read value by value: a frame may start at any real.
// `total` = frames * h.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) frames_pack_real_kernel(const T* x, long long signal_pitch, int hop, int nw, int h, const cpx<T>* win, cpx<T>* z,
                                                                long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long f = i / h;
        const int m = (int)(i - f * h);
        const long long s = f / nw;
        const T* src = x + s * signal_pitch + (f - s * nw) * (long long)hop + 2 * m;
        const cpx<T> w = win[m];
        z[i] = mk<T>(src[0] * w.re, src[1] * w.im);
    }
}

// Welch average of periodograms: psd[s][k] = (1 / nw) * sum_w power[s][w][k], power: [signals][nw][hb] one-sided power rows
// (hb = n/2 + 1), psd: [signals][hb].  One thread per output value, lanes along k (coalesced on both sides); w ascends inside the
// thread and the sum is kept in double for both precisions (the kernel is memory bound, and the error must not grow with the
// frame count).  No atomics: the result is bit-reproducible.  `total` = signals * hb.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) frames_mean_kernel(const T* power, T* psd, int nw, int hb, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long s = i / hb;
        const int k = (int)(i - s * hb);
        const T* col = power + s * (long long)nw * hb + k;
        double acc = 0.0;
        for (int w = 0; w < nw; w++) acc += (double)col[(long long)w * hb];
        psd[i] = (T)(acc / (double)nw);
    }
}

// One-sided rows -> the complex rows a half-length inverse transform reads (the unfused path of the inverse frames plan): row f of
// h + 1 bins at x_in + f * (h + 1) -> z[f][k], k < h, by the c2r merge
//   E = (X[k] + conj X[h-k]) / 2,  O = (X[k] - conj X[h-k]) / 2 * conj(W_n^k),  Z[k] = E + i O
// with X[0] and X[h] taken as REAL: their imaginary parts are never read into the result (numpy's irfft does the same;
// c2r_merge_kernel lets them through).  One thread per value of z; `total` = frames * h.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) iframes_merge_kernel(const cpx<T>* x_in, cpx<T>* z, const cpx<T>* w, int h, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long f = i / h;
        const int k = (int)(i - f * h);
        const cpx<T>* xb = x_in + f * (h + 1);
        if (k == 0) {
            const T dc = xb[0].re, ny = xb[h].re;
            z[i] = mk<T>((dc + ny) * (T)0.5, (dc - ny) * (T)0.5);
        } else {
            const cpx<T> a = xb[k];
            const cpx<T> m = xb[h - k];
            const cpx<T> c = mk<T>(m.re, -m.im);
            const cpx<T> e = cscale(cadd(a, c), (T)0.5);
            const cpx<T> o = cmul_conj(cscale(csub(a, c), (T)0.5), w[k]);
            z[i] = cadd(e, mul_pos_i(o));
        }
    }
}

// Weighted overlap-add of windowed frames, normalised by the window envelope (the inverse frames plan's second step):
//   y[s][t] = inv_env[t] * sum_w g[t - w hop] * v[s][w][t - w hop],   w over the frames that cover t,
// v: [signals][nw][n] real frames, g: the n window values, inv_env: out_len = (nw - 1) hop + n values (0 where the envelope
// vanishes: the sample is written as exactly 0, whatever the frames hold), y: signal s at y + s * signal_pitch.  One thread per
// output sample, lanes along t (the reads of each frame and the stores are coalesced); w ascends inside the thread and the sum is
// kept in double for both precisions.  No atomics: the result is bit-reproducible and independent of the grid.  Writes every
// t < out_len of every signal and nothing else.  `total` = signals * out_len.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) frames_overlap_add_kernel(const T* v, const T* g, const T* inv_env, T* y, long long signal_pitch, int n, int hop,
                                                                  int nw, long long out_len, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long s = i / out_len;
        const long long t = i - s * out_len;
        const T ie = inv_env[t];
        T r = (T)0;
        if (ie != (T)0) {
            long long w0 = t < n ? 0 : (t - n + hop) / hop;  // ceil((t - n + 1) / hop)
            long long w1 = t / hop;
            if (w1 > nw - 1) w1 = nw - 1;
            const T* frames = v + s * (long long)nw * n;
            double acc = 0.0;
            for (long long w = w0; w <= w1; w++) {
                const long long j = t - w * hop;
                acc += (double)g[j] * (double)frames[w * n + j];
            }
            r = (T)(acc * (double)ie);
        }
        y[s * signal_pitch + t] = r;
    }
}

// The cross kernels below rest on exact identities (Im conj(X) X == 0, swapped inputs give the conjugate bit for bit): a product
// and the sum it enters must round separately, so the compiler may not contract them into an fma.
#if defined(__clang__)
#define FFT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FFT_NO_CONTRACT
#endif

enum { CROSS_CSD = 0, CROSS_COHERENCE = 1, CROSS_TRANSFER = 2, CROSS_ALL = 3 };

// Two sets of STFT rows -> partial sums of the auto and cross spectra (the cross frames plan's first step).
//   X, Y: rows of frame f = s * nw + w at X + f * pitch (bins 0 .. hb - 1 are read: pitch = hb for one-sided rows, n for full ones);
//   part[s][c][k][0..3] = sum over the frames w of chunk c (w = c * C .. min(nw, (c + 1) * C) - 1, ascending) of
//       |X_w[k]|^2,  |Y_w[k]|^2,  Re conj(X_w[k]) Y_w[k],  Im conj(X_w[k]) Y_w[k].
// One thread per (pair, chunk, bin), lanes along k: both row reads are coalesced, as is the store.  Products and sums are formed in
// double for both precisions (memory bound; the error must not grow with the frame count), never contracted.  No atomics: the
// result is bit-reproducible and independent of the grid.  `total` = signals * chunks * hb.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) frames_cross_partial_kernel(const cpx<T>* X, const cpx<T>* Y, long long pitch, double* part, int nw, int hb,
                                                                    int C, int chunks, long long total) {
    FFT_NO_CONTRACT
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long sc = i / hb;
        const int k = (int)(i - sc * hb);
        const long long s = sc / chunks;
        const long long c = sc - s * chunks;
        const long long w0 = c * (long long)C;
        long long w1 = w0 + C;
        if (w1 > nw) w1 = nw;
        const cpx<T>* xr = X + (s * nw + w0) * pitch + k;
        const cpx<T>* yr = Y + (s * nw + w0) * pitch + k;
        double sxx = 0.0, syy = 0.0, sre = 0.0, sim = 0.0;
        for (long long w = w0; w < w1; w++, xr += pitch, yr += pitch) {
            const cpx<T> a = *xr, b = *yr;
            const double ar = (double)a.re, ai = (double)a.im, br = (double)b.re, bi = (double)b.im;
            sxx += ar * ar + ai * ai;
            syy += br * br + bi * bi;
            sre += ar * br + ai * bi;
            sim += ar * bi - ai * br;
        }
        double* p = part + i * 4;
        p[0] = sxx; p[1] = syy; p[2] = sre; p[3] = sim;
    }
}

// Partial sums -> the output rows of the cross frames plan (its second step).  One thread per (pair, bin): the chunks are summed in
// ascending order in double, scaled by c_k / nw (c_k = base, doubled for 0 < k < hb - 1: the POWER / WELCH scaling), the output
// kind is formed in double and rounded ONCE to T:
//   CROSS_CSD        out[s][k] = Pxy                                  complex
//   CROSS_COHERENCE  out[s][k] = |Pxy|^2 / (Pxx Pyy), 0 where Pxx Pyy == 0    real
//   CROSS_TRANSFER   out[s][k] = Pxy / Pxx, (0, 0) where Pxx == 0              complex
//   CROSS_ALL        out[s][k][0..3] = Pxx, Pyy, Re Pxy, Im Pxy               reals
// (a NaN is not "== 0": it propagates).  Writes its rows and nothing else.  `total` = signals * hb.
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) frames_cross_finish_kernel(const double* part, T* out, int nw, int hb, int chunks, double base, int kind,
                                                                   long long total) {
    FFT_NO_CONTRACT
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long s = i / hb;
        const int k = (int)(i - s * hb);
        const double* p = part + (s * chunks * hb + k) * 4;
        double sxx = 0.0, syy = 0.0, sre = 0.0, sim = 0.0;
        for (int c = 0; c < chunks; c++, p += (long long)hb * 4) {
            sxx += p[0]; syy += p[1]; sre += p[2]; sim += p[3];
        }
        const double f = ((k > 0 && k < hb - 1) ? base * 2.0 : base) / (double)nw;
        const double pxx = sxx * f, pyy = syy * f, pre = sre * f, pim = sim * f;
        if (kind == CROSS_CSD) {
            out[2 * i] = (T)pre;
            out[2 * i + 1] = (T)pim;
        } else if (kind == CROSS_COHERENCE) {
            const double den = pxx * pyy;
            out[i] = den == 0.0 ? (T)0 : (T)((pre * pre + pim * pim) / den);
        } else if (kind == CROSS_TRANSFER) {
            const bool z = pxx == 0.0;
            out[2 * i] = z ? (T)0 : (T)(pre / pxx);
            out[2 * i + 1] = z ? (T)0 : (T)(pim / pxx);
        } else {
            out[4 * i] = (T)pxx;
            out[4 * i + 1] = (T)pyy;
            out[4 * i + 2] = (T)pre;
            out[4 * i + 3] = (T)pim;
        }
    }
}

// Device streams, 16 bytes per lane, `unroll` independent accesses in flight per thread, grid-stride: the practical ceiling
// of the box the benchmark runs on (MI355X_MICROARCH.md quotes 6.29 TB/s for a float4 copy).  MODE 0 copy, 1 read only (the
// values are folded into one word that is stored only if it is a NaN pattern the inputs never hold), 2 write only.  NT: the
// non-temporal hint on both sides -- what the FFT kernels' own streams carry.
template <int UNROLL, int MODE, int NT>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) stream16_kernel(const vec16<float>* in, vec16<float>* out, long long n16) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    long long i = FFT_BID * FFT_NTHREADS + FFT_TID;
    vec16<float> acc;
    acc.c[0] = mk<float>(0.f, 0.f);
    acc.c[1] = mk<float>(1.f, 2.f);
    for (; i + (UNROLL - 1) * stride < n16; i += UNROLL * stride) {
        vec16<float> v[UNROLL];
        FFT_UNROLL
        for (int u = 0; u < UNROLL; u++) v[u] = MODE == 2 ? acc : fft_ld16<NT>(in + i + u * stride);
        if (MODE == 1) {
            FFT_UNROLL
            for (int u = 0; u < UNROLL; u++) {
                acc.c[0].re += v[u].c[0].re;
                acc.c[0].im += v[u].c[1].im;
            }
        } else {
            FFT_UNROLL
            for (int u = 0; u < UNROLL; u++) fft_st16<NT>(out + i + u * stride, v[u]);
        }
    }
    for (; i < n16; i += stride) {
        if (MODE == 1) acc.c[0].re += fft_ld16<NT>(in + i).c[0].re;
        else fft_st16<NT>(out + i, MODE == 2 ? acc : fft_ld16<NT>(in + i));
    }
    if (MODE == 1 && acc.c[0].re != acc.c[0].re && acc.c[0].im == 12345.f) out[0] = acc;
}

// The streams in the shape of the single-pass FFT kernels (whose n = 512 instance moves 6.1 TB/s, more than any grid-stride shape above
// reached -- round-3 review): a 256-thread workgroup walks tiles of U x 4 KiB `tile = block, block + grid, ..`; per tile a thread has U
// 16-byte accesses in flight, a wave instruction covers 1 KiB, and the NEXT tile's loads are issued before this tile's stores
// (MODE as above).
template <int MODE, int NT, int U = 8>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) stream_tile_kernel(const vec16<float>* in, vec16<float>* out, long long n_tiles) {
    const int tid = FFT_TID;
    vec16<float> acc;
    acc.c[0] = mk<float>(0.f, 0.f);
    acc.c[1] = mk<float>(1.f, 2.f);
    vec16<float> cur[U], nxt[U];  // tiles of U x 4 KiB
    long long t = FFT_BID;
    if (MODE != 2 && t < n_tiles) {
        FFT_UNROLL
        for (int i = 0; i < U; i++) cur[i] = fft_ld16<NT>(in + t * (U * 256) + i * 256 + tid);
    }
    for (; t < n_tiles; t += FFT_NBLOCKS) {
        const long long tn = t + FFT_NBLOCKS;
        if (MODE != 2 && tn < n_tiles) {
            FFT_UNROLL
            for (int i = 0; i < U; i++) nxt[i] = fft_ld16<NT>(in + tn * (U * 256) + i * 256 + tid);
        }
        if (MODE == 1) {
            FFT_UNROLL
            for (int i = 0; i < U; i++) {
                acc.c[0].re += cur[i].c[0].re;
                acc.c[0].im += cur[i].c[1].im;
            }
        } else {
            FFT_UNROLL
            for (int i = 0; i < U; i++) fft_st16<NT>(out + t * (U * 256) + i * 256 + tid, MODE == 2 ? acc : cur[i]);
        }
        if (MODE != 2) {
            FFT_UNROLL
            for (int i = 0; i < U; i++) cur[i] = nxt[i];
        }
    }
    if (MODE == 1 && acc.c[0].re != acc.c[0].re && acc.c[0].im == 12345.f) out[0] = acc;
}

#if !defined(FFT_EMU)
// The copy in the shape of the engine's own kernels: one 512-thread workgroup per CU walks 64 KiB tiles, tile t + 1 lands in
// LDS by LDS-DMA (nt) while tile t leaves it through registers (ds_read_b128 + nt stores): two tiles of reads in flight per CU.
FFT_KERNEL void FFT_LAUNCH_BOUNDS(512) copy_dma_kernel(const vec16<float>* in, vec16<float>* out, long long n_tiles) {
    FFT_DYN_SMEM(smem);  // 2 x 64 KiB
    const int tid = FFT_TID;
    const unsigned lds0 = FFT_LDS_ADDR(smem);
    long long t = FFT_BID;
    auto dma = [&](long long tile, int im) __attribute__((always_inline)) {
        const vec16<float>* src = in + tile * 4096 + tid;
        FFT_UNROLL
        for (int i = 0; i < 8; i++) fft_dma16<2>(src + i * 512, lds0 + (unsigned)im * 65536u + (unsigned)(i * 512 + tid) * 16u);
    };
    if (t < n_tiles) dma(t, 0);
    int im = 0;
    bool first = true;
    for (; t < n_tiles; t += FFT_NBLOCKS, im ^= 1) {
        // this tile has landed: behind its 8 pieces this thread has issued the 8 stores of the previous tile -- except on the first
        // tile, where the pieces are the youngest thing in flight (vmcnt(8) passed at once there and the reads ran early)
        if (first) FFT_WAIT_VM0();
        else FFT_WAIT_VM_LE(8);
        first = false;
        FFT_SYNC_LDS();
        if (t + FFT_NBLOCKS < n_tiles) dma(t + FFT_NBLOCKS, im ^ 1);
        const vec16<float>* img = reinterpret_cast<const vec16<float>*>(smem + im * 65536);
        vec16<float> v[8];
        FFT_UNROLL
        for (int i = 0; i < 8; i++) v[i] = img[i * 512 + tid];
        FFT_UNROLL
        for (int i = 0; i < 8; i++) FFT_STORE16_NT(out + t * 4096 + i * 512 + tid, v[i]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}
#endif

// ---------------------------------------------------------------------------
// Overlap-save filtering, the unfused ends (FilterPlan's fallback; the fused kernel is tile_fft_kernel with HOOKBIT_BOUND and HOOKBIT_VALID and
// has the same predicates).  Block f = sig * nb + w of length n = 2^log2n holds the signal's samples q = w * B - lead + l, l < n,
// zero where q lies outside [0, signal_len); of its circular convolution with the taps the values l >= lead are samples
// p = w * B + l - lead - out_off of the signal's output, stored only for 0 <= p < out_len.  One thread per value; blocks
// f0 ... f0 + total / n - 1 of the execute live in work[(f - f0) * n + l].
// ---------------------------------------------------------------------------
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) filter_gather_kernel(const cpx<T>* x, long long x_pitch, int signal_len, int nb, int B, int lead, int log2n,
                                                            long long f0, cpx<T>* work, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long f = f0 + (i >> log2n);
        const int l = (int)(i & ((1ll << log2n) - 1));
        const long long sig = f / nb;
        const long long q = (f - sig * nb) * (long long)B - lead + l;
        cpx<T> v = mk<T>((T)0, (T)0);
        if (q >= 0 && q < signal_len) v = x[sig * x_pitch + q];
        work[i] = v;
    }
}

template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) filter_scatter_kernel(const cpx<T>* work, cpx<T>* y, long long y_pitch, int out_len, int out_off, int nb, int B,
                                                             int lead, int log2n, long long f0, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long f = f0 + (i >> log2n);
        const int l = (int)(i & ((1ll << log2n) - 1));
        if (l < lead) continue;
        const long long sig = f / nb;
        const long long p = (f - sig * nb) * (long long)B + l - lead - out_off;
        if (p >= 0 && p < out_len) y[sig * y_pitch + p] = work[i];
    }
}

}  // namespace fftk
