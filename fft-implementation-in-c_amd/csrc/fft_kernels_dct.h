// fft_kernels_dct.h -- the kernels of the cosine / sine transform plans (fft_plans_ext.h DctPlan, Dct2DPlan): DCT-II, DCT-III, DST-II
// and DST-III of real rows, scipy's conventions.
//
//   dct_rows_kernel<T, false>  one launch = the DCT-II (DST-II) of every row: permuted real load, length-N/2 complex transform, r2c split
//                              and quarter-sample twiddle in the store
//   dct_rows_kernel<T, true>   one launch = the DCT-III (DST-III) of every row: quarter-sample twiddle and c2r merge on the way to the
//                              stages, inverse length-N/2 transform, permuted real store
//   dct_pre_kernel / dct_post_kernel   the two ends of the fallback (any N): Makhoul's algorithm around a length-N complex transform
//   transpose_real_kernel      transpose_kernel's real twin (the 2D plan's composition), with a matrix pitch on either side
//
// dct_rows_kernel is a kernel of its own, not two more HOOK bits on tile_fft_kernel: the permutation and the twiddle sit where that
// kernel's bit 6 / bit 7 code sits, and every instantiation of tile_fft_kernel stays byte for byte what it was.  It runs on the tile of
// the hooked single-pass rows kernel (Pow2Plan's PassDesc for length L = N/2: E = 4 values per thread, radix-4 stages, C rows per tile,
// rows of the LDS image L * sizeof(cpx<T>) + 16 bytes apart) and reuses the stage code (stockham_all_stages) and its tables.
//
// Forward (Makhoul).  v[j] = x[2j], v[N-1-j] = x[2j+1] (j < L); z[m] = v[2m] + i v[2m+1]; Z = FFT_L(z); with Z[L] = Z[0]
//     c[k] = qa[k] (Z[k] + conj Z[L-k]) + qb[k] (Z[k] - conj Z[L-k]),   qa[k] = f_k q_k,  qb[k] = f_k q_k W_N^k / i,  q_k = e^(-i pi k / 2N)
//     X[k] = Re c[k] (k <= L),   X[N-k] = -Im c[k] (0 < k < L)
// f_k is the norm (fft_gpu_dct_norm_t), folded into the tables.  The 16-byte chunk x[4m .. 4m+3] of an fp32 row IS z[m] = (x[4m], x[4m+2])
// and z[L-1-m] = (x[4m+3], x[4m+1]); an fp64 chunk x[2q], x[2q+1] is v[q] and v[N-1-q]: every load is used whole, every byte read once.
// Inverse.  V[k] = cq[k] (X[k] - i X[N-k]), X[N] = 0, cq[k] = g_k conj q_k (k <= L);  Z[l] = (V[l] + conj V[L-l]) + i (V[l] - conj V[L-l]) cw[l],
// cw[l] = conj W_N^l; z = L * IFFT_L(Z) (the unscaled inverse); x leaves through the same permutation backwards.
// sine: DST-II(x)[k] = DCT-II((-1)^n x[n])[N-1-k]; DST-III(X)[n] = (-1)^n DCT-III(reverse X)[n]: a sign on the real side, a reversed
// index on the spectral side.
// Rows are in_pitch / out_pitch reals apart.  in_vec / out_vec: base and pitch of that side are multiples of 16 bytes and a chunk moves
// as one 16-byte access; otherwise value by value.  Rows at or past n_rows (the last tile's padding) are neither read nor written.  A
// tile's rows are all loaded before any of them is stored, and tiles are disjoint sets of rows: in place (in == out, equal pitches) works.
#pragma once

#include "fft_kernels.h"

namespace fftk {

template <typename T>
struct alignas(16) rvec16 {
    static constexpr int RV = 16 / (int)sizeof(T);
    T r[RV];
};

template <typename T>
struct DctParams {
    const T* in;
    T* out;
    const cpx<T>* tables;  // the pass's blob [ sa | sb ]
    const cpx<T>* ta;      // forward: qa[k], k <= L;  inverse: cq[k], k <= L
    const cpx<T>* tb;      // forward: qb[k], k <= L;  inverse: cw[l], l < L
    int group_bytes, tables_bytes, off_tables, o_sb, sa_bits;
    int log2L, log2C;      // L = N/2 complex points per row, C rows per tile
    long long in_pitch, out_pitch;  // reals between rows
    long long n_rows, n_tiles;
    int in_vec, out_vec;
    int sine;
};

template <typename T, bool INV>
FFT_KERNEL void FFT_LAUNCH_BOUNDS2(1024, FFT_WAVES_PER_SIMD_E4) dct_rows_kernel(DctParams<T> p) {
    constexpr int E = 4, H = 1;
    constexpr int V = vec16<T>::V;
    constexpr int RV = rvec16<T>::RV;
    constexpr int log2V = Log2<V>::value;
    constexpr int log2E = Log2<E>::value;
    constexpr int SZ = (int)sizeof(cpx<T>);
    FFT_DYN_SMEM(smem);

    const int tid_invariant = FFT_TID;
    const int nthreads = FFT_NTHREADS;
    const int log2L = p.log2L, log2C = p.log2C;
    const int L = 1 << log2L, N = 2 * L;
    const int log2TPC = log2L - log2E;
    const int log2J = log2C - log2V;
    const int J = 1 << log2J;
    const int j_invariant = tid_invariant & (J - 1);
    const int r_invariant = tid_invariant >> log2J;
    const int pitch = L * SZ + 16;      // bytes between the rows of the LDS image
    const int log2CPR = log2L - log2V;  // 16-byte chunks per row
    const int cpr_mask = (1 << log2CPR) - 1;
    const long long n_tiles = p.n_tiles;
    const long long tile_step = FFT_NBLOCKS;
    const bool sine = p.sine != 0;

    {  // stage tables -> LDS
        const vec16<T>* src = reinterpret_cast<const vec16<T>*>(p.tables);
        vec16<T>* dst = reinterpret_cast<vec16<T>*>(smem + p.off_tables);
        for (int i = tid_invariant; i < (p.tables_bytes >> 4); i += nthreads) dst[i] = src[i];
    }
    const cpx<T>* tab = reinterpret_cast<const cpx<T>*>(smem + p.off_tables);
    StageTw<T> tw;
    tw.sa = tab; tw.sb = tab + p.o_sb; tw.sa_bits = p.sa_bits; tw.log2L = log2L;

    // nxt[i] = chunk g = tid + i * nthreads of the tile: reals pos * RV ... of row c0 + t, t = g >> log2CPR, pos = g & cpr_mask
    rvec16<T> nxt[E];
    auto prefetch = [&](long long tile) __attribute__((always_inline)) {
        const long long c0 = tile << log2C;
        int tid = tid_invariant;
        FFT_OPAQUE(tid);
        FFT_UNROLL
        for (int i = 0; i < E; i++) {
            const int g = tid + i * nthreads;
            const long long row = c0 + (g >> log2CPR);
            const T* src = p.in + row * p.in_pitch + (long long)(g & cpr_mask) * RV;
            FFT_UNROLL
            for (int q = 0; q < RV; q++) nxt[i].r[q] = (T)0;
            if (row < p.n_rows) {
                if (p.in_vec) {
                    nxt[i] = fft_ld16<0>(reinterpret_cast<const rvec16<T>*>(src));
                } else {
                    FFT_UNROLL
                    for (int q = 0; q < RV; q++) nxt[i].r[q] = src[q];
                }
            }
        }
    };

    const long long tile0 = FFT_BID;
    if (tile0 < n_tiles) prefetch(tile0);
    FFT_SYNC();  // tables visible

    for (long long tile = tile0; tile < n_tiles; tile += tile_step) {
        const long long c0 = tile << log2C;
        cpx<T> x[H][E][V];
        int r = r_invariant, j = j_invariant, tid = tid_invariant;
        FFT_OPAQUE(r);
        FFT_OPAQUE(j);
        FFT_OPAQUE(tid);

        // ---- the landed chunks -> the tile's LDS image
        FFT_SYNC_LDS();  // the previous tile's store image is consumed
        FFT_UNROLL
        for (int i = 0; i < E; i++) {
            const int g = tid + i * nthreads;
            unsigned char* row = smem + (size_t)(g >> log2CPR) * pitch;
            const int pos = g & cpr_mask;
            if (INV) {  // the row of N reals as it lies in memory
                *reinterpret_cast<rvec16<T>*>(row + (size_t)pos * 16) = nxt[i];
            } else if (RV == 4) {  // x[4m .. 4m+3] = z[m] and z[L-1-m]
                const T s = sine ? (T)-1 : (T)1;
                cpx<T>* z = reinterpret_cast<cpx<T>*>(row);
                z[pos] = mk<T>(nxt[i].r[0], nxt[i].r[RV - 2]);
                z[L - 1 - pos] = mk<T>(s * nxt[i].r[RV - 1], s * nxt[i].r[1]);
            } else {  // x[2q], x[2q+1] = v[q] and v[N-1-q]
                T* v = reinterpret_cast<T*>(row);
                v[pos] = nxt[i].r[0];
                v[N - 1 - pos] = sine ? -nxt[i].r[1] : nxt[i].r[1];
            }
        }
        FFT_SYNC_LDS();
        // ---- slot e <- element l = r + TPC * e of the thread's V rows
        FFT_UNROLL
        for (int e = 0; e < E; e++) {
            const int l = r + (e << log2TPC);
            FFT_UNROLL
            for (int vv = 0; vv < V; vv++) {
                const unsigned char* row = smem + (size_t)(V * j + vv) * pitch;
                if (!INV) {
                    x[0][e][vv] = *reinterpret_cast<const cpx<T>*>(row + (size_t)l * SZ);
                } else {
                    // quarter-sample twiddle and c2r merge: Z[l] from X[l], X[N-l], X[L-l] and X[L+l] of the row's own image
                    const T* X = reinterpret_cast<const T*>(row);
                    auto Xd = [&](int k) __attribute__((always_inline)) -> T { return sine ? X[N - 1 - k] : X[k]; };
                    const T xn = Xd(l == 0 ? 0 : N - l);
                    const T xnl = l == 0 ? (T)0 : xn;  // X[N] = 0
                    const cpx<T> vl = cmul(p.ta[l], mk<T>(Xd(l), -xnl));
                    const cpx<T> vm = cmul(p.ta[L - l], mk<T>(Xd(L - l), -Xd(L + l)));
                    const cpx<T> cm = mk<T>(vm.re, -vm.im);
                    const cpx<T> z = cadd(cadd(vl, cm), mul_pos_i(cmul(csub(vl, cm), p.tb[l])));
                    x[0][e][vv] = cswap(z);  // the inverse transform = the forward one between two re <-> im swaps
                }
            }
        }
        FFT_SCHED_BARRIER();
        if (tile + tile_step < n_tiles) prefetch(tile + tile_step);  // flies during the stages and the store
        FFT_SCHED_BARRIER();

        FFT_SYNC_LDS();  // the image is fully consumed
        stockham_all_stages<T, E, FAM_R4, V, H>(x, smem, p.group_bytes, tw, r, j, log2J, log2TPC, log2L, []() {});

        // ---- slot e holds Z[K] (inverse: z[K] = v[2K] + i v[2K+1]), K = r + TPC * e -> the tile's LDS image
        FFT_SYNC_LDS();  // the last exchange is fully consumed
        FFT_UNROLL
        for (int e = 0; e < E; e++) {
            const int K = r + (e << log2TPC);
            FFT_UNROLL
            for (int vv = 0; vv < V; vv++) {
                unsigned char* row = smem + (size_t)(V * j + vv) * pitch;
                if (!INV) {
                    *reinterpret_cast<cpx<T>*>(row + (size_t)K * SZ) = x[0][e][vv];
                } else {
                    // v[i] = x[2i] (i < L), v[N-1-i'] = x[2i'+1]: the pair v[2K], v[2K+1] lands two reals apart, even or odd positions
                    const cpx<T> z = cswap(x[0][e][vv]);
                    T* xr = reinterpret_cast<T*>(row);
                    if (2 * K < L) {
                        xr[4 * K] = z.re;
                        xr[4 * K + 2] = z.im;
                    } else {
                        const int n = 2 * N - 4 * K - 1;
                        xr[n] = sine ? -z.re : z.re;
                        xr[n - 2] = sine ? -z.im : z.im;
                    }
                }
            }
        }
        FFT_SYNC_LDS();
        FFT_UNROLL
        for (int i = 0; i < E; i++) {
            const int g = tid + i * nthreads;
            const long long rowi = c0 + (g >> log2CPR);
            const int pos = g & cpr_mask;
            if (rowi < p.n_rows) {
                const unsigned char* row = smem + (size_t)(g >> log2CPR) * pitch;
                rvec16<T> o;
                if (INV) {
                    o = *reinterpret_cast<const rvec16<T>*>(row + (size_t)pos * 16);
                } else {
                    // r2c split and quarter-sample twiddle: output k from Z[k'] and Z[L-k'], k' = min(k, N-k), of the row's own image
                    const cpx<T>* Z = reinterpret_cast<const cpx<T>*>(row);
                    FFT_UNROLL
                    for (int q = 0; q < RV; q++) {
                        const int at = pos * RV + q;
                        const int k = sine ? N - 1 - at : at;
                        const int kk = k <= L ? k : N - k;
                        const cpx<T> a = Z[kk & (L - 1)], b = Z[(L - kk) & (L - 1)];
                        const cpx<T> cb = mk<T>(b.re, -b.im);
                        const cpx<T> c = cadd(cmul(p.ta[kk], cadd(a, cb)), cmul(p.tb[kk], csub(a, cb)));
                        o.r[q] = k <= L ? c.re : -c.im;
                    }
                }
                T* dst = p.out + rowi * p.out_pitch + (long long)pos * RV;
                if (p.out_vec) {
                    fft_st16<0>(reinterpret_cast<rvec16<T>*>(dst), o);
                } else {
                    FFT_UNROLL
                    for (int q = 0; q < RV; q++) dst[q] = o.r[q];
                }
            }
        }
    }
}

// ---- the fallback's two ends (any N >= 1), value by value.  work: [rows][n] complex, dense; tab: [n]
// forward: work[b][i] = (+-x[b][src(i)], 0), the permuted row (src(i) = 2i for i < ceil(n/2), else 2 (n-1-i) + 1; sine: odd samples negated)
// inverse: work[b][k] = tab[k] (X[k] - i X[n-k]), X[n] = 0 (sine: X read backwards): the full Hermitian spectrum of the permuted row
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) dct_pre_kernel(const T* in, long long in_pitch, cpx<T>* work, const cpx<T>* tab, int n, int inverse, int sine,
                                                     long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long t = FFT_BID * FFT_NTHREADS + FFT_TID; t < total; t += stride) {
        const long long b = t / n;
        const int i = (int)(t - b * n);
        const T* x = in + b * in_pitch;
        if (!inverse) {
            const int src = i < (n + 1) / 2 ? 2 * i : 2 * (n - 1 - i) + 1;
            const T v = x[src];
            work[t] = mk<T>((sine && (src & 1)) ? -v : v, (T)0);
        } else {
            const T a = sine ? x[n - 1 - i] : x[i];
            const T c = i == 0 ? (T)0 : (sine ? x[i - 1] : x[n - i]);
            work[t] = cmul(tab[i], mk<T>(a, -c));
        }
    }
}

// forward: out[b][at] = Re(tab[k] work[b][k]), k = at (sine: n - 1 - at)
// inverse: out[b][m] = +-Re work[b][i(m)], i(m) = m / 2 for even m, n - 1 - (m - 1) / 2 for odd m (sine: odd samples negated)
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) dct_post_kernel(const cpx<T>* work, const cpx<T>* tab, T* out, long long out_pitch, int n, int inverse, int sine,
                                                      long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long t = FFT_BID * FFT_NTHREADS + FFT_TID; t < total; t += stride) {
        const long long b = t / n;
        const int at = (int)(t - b * n);
        T v;
        if (!inverse) {
            const int k = sine ? n - 1 - at : at;
            const cpx<T> w = tab[k], a = work[b * n + k];
            v = w.re * a.re - w.im * a.im;
        } else {
            const int i = (at & 1) ? n - 1 - (at - 1) / 2 : at / 2;
            v = work[b * n + i].re;
            if (sine && (at & 1)) v = -v;
        }
        out[b * out_pitch + at] = v;
    }
}

// out[b * out_b + c * rows + r] = in[b * in_b + r * cols + c]: transpose_kernel (fft_kernels_ext.h) on reals, matrices in_b / out_b apart
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) transpose_real_kernel(const T* in, long long in_b, T* out, long long out_b, int rows, int cols, long long n_tiles) {
    FFT_DYN_SMEM(smem);
    T* tile = reinterpret_cast<T*>(smem);  // [32][33]
    const int tr = (rows + 31) / 32, tc = (cols + 31) / 32;
    const int tx = FFT_TID & 31, ty = FFT_TID >> 5;
    for (long long t = FFT_BID; t < n_tiles; t += FFT_NBLOCKS) {
        const long long b = t / ((long long)tr * tc);
        const int rem = (int)(t - b * (long long)tr * tc);
        const int r0 = (rem / tc) * 32, c0 = (rem % tc) * 32;
        const T* src = in + b * in_b;
        T* dst = out + b * out_b;
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

}  // namespace fftk
