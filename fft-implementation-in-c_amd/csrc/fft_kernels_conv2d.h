// fft_kernels_conv2d.h -- the kernels of the 2D convolution / spectrum-filtering plan (fft_plans_ext.h Conv2DPlan).
//
//   tile_fft_colround_kernel  forward column transforms -> product with the kernel's spectrum -> inverse column transforms of one
//                             P x C tile, without leaving the CU: the column step of  IFFT2( FFT2(x) . H )
//   conv2d_pad_kernel         fallback: the images zero padded into [M][P][Q]
//   conv2d_crop_kernel        fallback: the wanted out_rows x out_cols corner of [M][P][Q] into the caller's matrices
//
// tile_fft_colround_kernel is tile_fft_ba_kernel's simpler sibling (fft_kernels_chain.h: row stages -> product -> column stages):
// both runs of stages here are COLUMN stages on the same register layout.  After the forward stages slot e of thread (j, r) holds
// frequency K = r + TPC * e of the thread's V columns -- and that is the slot layout the stages start from (fft_kernels.h, "One
// Stockham stage"), so the inverse (the forward transform between two re <-> im swaps) runs on the registers as they are; LDS only
// carries the stages' exchanges.  The tile is that of Pow2Plan::build_columns: E = 8 values per thread, at most 512 threads.
//   load   rows l < rows_in of work1 (the row-transformed image, rows_in x Q per matrix); rows at or beyond rows_in are the zero
//          padding: zeros in registers, memory untouched
//   H      16 bytes per slot, at H + K * Q + c0 + V * j, requested before the forward stages (their latency hides behind them)
//   store  rows K < rows_out only, into work2 (rows_out x Q per matrix): the cropped rows never leave the CU
// Columns at or beyond n_cols (a last tile wider than what is left of the row) are dead on both sides: zeros in, nothing read from H,
// nothing stored.  Every matrix has tiles of its own, and the columns of a tile never mix: a NaN stays in its matrix and column.
// The next tile's loads are issued after the product, so they fly behind the second run of stages and the store.
#pragma once

#include "fft_kernels.h"
#include "fft_kernels_chain.h"

namespace fftk {

template <typename T>
struct ColRoundParams {
    const cpx<T>* in;      // work1: [matrices][rows_in][ld]
    cpx<T>* out;           // work2: [matrices][rows_out][ld]
    const cpx<T>* spec;    // H: [L][ld], shared by the matrices
    const cpx<T>* tables;  // the column pass's blob [ sa | sb ] (no inter-pass twiddle)
    int group_bytes, tables_bytes, off_tables, o_sb, sa_bits;
    int log2L, log2C;      // L = P rows, C columns per tile
    int n_ct;              // column tiles per matrix
    int n_cols;            // Q
    int rows_in, rows_out;
    long long in_b, out_b, ld;  // elements between matrices of work1 / work2; elements between rows (Q)
    long long n_tiles;     // matrices * n_ct
    int nt;                // non-temporal hint: bit 0 loads, bit 1 stores (TileParams::nt)
    T scale;               // 1 / P
};

template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS2(512, FFT_CHAIN_WAVES_PER_SIMD) tile_fft_colround_kernel(ColRoundParams<T> p) {
    constexpr int E = 8, H = 1;
    constexpr int V = vec16<T>::V;
    constexpr int log2V = Log2<V>::value;
    constexpr int log2E = Log2<E>::value;
    FFT_DYN_SMEM(smem);

    const int tid_invariant = FFT_TID;
    const int nthreads = FFT_NTHREADS;
    const bool nt_load = (p.nt & FFT_TILE_NT & 1) != 0, nt_store = (p.nt & FFT_TILE_NT & 2) != 0;
    const int log2L = p.log2L, log2C = p.log2C;
    const int log2TPC = log2L - log2E;
    const int log2J = log2C - log2V;
    const int J = 1 << log2J;
    const int j_invariant = tid_invariant & (J - 1);
    const int r_invariant = tid_invariant >> log2J;
    const long long n_tiles = p.n_tiles;
    const long long tile_step = FFT_NBLOCKS;

    {  // stage tables -> LDS
        const vec16<T>* src = reinterpret_cast<const vec16<T>*>(p.tables);
        vec16<T>* dst = reinterpret_cast<vec16<T>*>(smem + p.off_tables);
        for (int i = tid_invariant; i < (p.tables_bytes >> 4); i += nthreads) dst[i] = src[i];
    }
    const cpx<T>* tab = reinterpret_cast<const cpx<T>*>(smem + p.off_tables);
    StageTw<T> tw;
    tw.sa = tab; tw.sb = tab + p.o_sb; tw.sa_bits = p.sa_bits; tw.log2L = log2L;

    // nxt[e] = row l = r + TPC * e of columns c0 + V * j ... of the tile's matrix: in flight or landed
    vec16<T> nxt[E];
    auto prefetch_as = [&](auto nt_tag, long long tile) __attribute__((always_inline)) {
        constexpr int NTL = decltype(nt_tag)::value;
        const long long m = tile / p.n_ct;
        const int c0 = (int)(tile - m * p.n_ct) << log2C;
        int r = r_invariant, j = j_invariant;
        FFT_OPAQUE(r);
        FFT_OPAQUE(j);
        const bool live = (c0 + V * j) < p.n_cols;
        const cpx<T>* src = p.in + m * p.in_b + c0 + V * j;
        FFT_UNROLL
        for (int e = 0; e < E; e++) {
            const int l = r + (e << log2TPC);
            if (live && l < p.rows_in) {
                nxt[e] = fft_ld16<NTL>(reinterpret_cast<const vec16<T>*>(src + (long long)l * p.ld));
            } else {
                FFT_UNROLL
                for (int vv = 0; vv < V; vv++) nxt[e].c[vv] = mk<T>((T)0, (T)0);
            }
        }
    };
    auto prefetch = [&](long long tile) __attribute__((always_inline)) {  // one wave-uniform branch per tile, the loads stay one clause
        if (nt_load) prefetch_as(std::integral_constant<int, 1>{}, tile);
        else prefetch_as(std::integral_constant<int, 0>{}, tile);
    };

    const long long tile0 = FFT_BID;
    if (tile0 < n_tiles) prefetch(tile0);
    FFT_SYNC();  // tables visible

    for (long long tile = tile0; tile < n_tiles; tile += tile_step) {
        const long long m = tile / p.n_ct;
        const int c0 = (int)(tile - m * p.n_ct) << log2C;
        cpx<T> x[H][E][V];
        int r = r_invariant, j = j_invariant;
        FFT_OPAQUE(r);
        FFT_OPAQUE(j);
        const bool live = (c0 + V * j) < p.n_cols;

        FFT_UNROLL
        for (int e = 0; e < E; e++) {
            FFT_UNROLL
            for (int vv = 0; vv < V; vv++) x[0][e][vv] = nxt[e].c[vv];
        }
        // the spectrum's sixteen bytes per slot, requested BEFORE the forward stages: slot e will hold X[K][column], K = r + TPC * e
        vec16<T> hv[E];
        {
            const cpx<T>* hb = p.spec + c0 + V * j;
            FFT_UNROLL
            for (int e = 0; e < E; e++) {
                const long long K = r + ((long long)e << log2TPC);
                if (live) {
                    hv[e] = *reinterpret_cast<const vec16<T>*>(hb + K * p.ld);  // 16-byte aligned: every term is a multiple of V
                } else {
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++) hv[e].c[vv] = mk<T>((T)0, (T)0);
                }
            }
        }
        FFT_SCHED_BARRIER();
        FFT_SYNC_LDS();  // the previous tile's last exchange is fully consumed
        stockham_all_stages<T, E, FAM_SR16, V, H>(x, smem, p.group_bytes, tw, r, j, log2J, log2TPC, log2L, []() {});
        FFT_SCHED_BARRIER();

        // spectral product, and the swap that turns the second run of stages into the inverse transform
        FFT_UNROLL
        for (int e = 0; e < E; e++) {
            FFT_UNROLL
            for (int vv = 0; vv < V; vv++) x[0][e][vv] = cswap(cmul(x[0][e][vv], hv[e].c[vv]));
        }
        FFT_SCHED_BARRIER();
        if (tile + tile_step < n_tiles) prefetch(tile + tile_step);  // behind the second run of stages and the store
        FFT_SCHED_BARRIER();

        FFT_SYNC_LDS();  // the forward transform's last exchange is fully consumed
        stockham_all_stages<T, E, FAM_SR16, V, H>(x, smem, p.group_bytes, tw, r, j, log2J, log2TPC, log2L, []() {});

        cpx<T>* outp = p.out + m * p.out_b + c0 + V * j;
        auto store_as = [&](auto nt_tag) __attribute__((always_inline)) {
            constexpr int NTS = decltype(nt_tag)::value;
            FFT_UNROLL
            for (int e = 0; e < E; e++) {
                const long long K = r + ((long long)e << log2TPC);
                if (live && K < p.rows_out) {
                    vec16<T> v;
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++) v.c[vv] = cscale(cswap(x[0][e][vv]), p.scale);
                    fft_st16<NTS>(reinterpret_cast<vec16<T>*>(outp + K * p.ld), v);
                }
            }
        };
        if (nt_store) store_as(std::integral_constant<int, 1>{});
        else store_as(std::integral_constant<int, 0>{});
    }
}

// fallback: w[m][r][c] = r < rows && c < cols ? x[m * x_pitch + r * cols + c] : 0 over [M][2^log2P][2^log2Q]
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256)
    conv2d_pad_kernel(const cpx<T>* x, long long x_pitch, int rows, int cols, cpx<T>* w, int log2P, int log2Q, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const int c = (int)(i & ((1ll << log2Q) - 1));
        const int r = (int)((i >> log2Q) & ((1ll << log2P) - 1));
        const long long m = i >> (log2Q + log2P);
        cpx<T> v = mk<T>((T)0, (T)0);
        if (r < rows && c < cols) v = x[m * x_pitch + (long long)r * cols + c];
        w[i] = v;
    }
}

// fallback: y[m * y_pitch + r * out_cols + c] = w[m][r][c], r < out_rows, c < out_cols; total = M * out_rows * out_cols
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256)
    conv2d_crop_kernel(const cpx<T>* w, int log2P, int log2Q, cpx<T>* y, long long y_pitch, int out_rows, int out_cols, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long t = i / out_cols;
        const int c = (int)(i - t * out_cols);
        const long long m = t / out_rows;
        const int r = (int)(t - m * out_rows);
        y[m * y_pitch + (long long)r * out_cols + c] = w[(((m << log2P) + r) << log2Q) + c];
    }
}

}  // namespace fftk
