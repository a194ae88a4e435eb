// fft_kernels_real2d.h -- the kernels of the real 2D transform plan (fft_plans_ext.h Real2DPlan): rfft2 / irfft2 of row-major images.
//
//   tile_fft_colpass_kernel   one run of the radix-8 column stages on a P x C tile: the column transforms of the L + 1 one-sided
//                             columns of a real image's row spectra, forward or inverse
//   real2d_copy_kernel        matrices between an image of the plan's own and a caller's buffer that a transform cannot read or write
//                             directly (a matrix pitch of the caller's own, or a base that is not 16-byte aligned)
//   real2d_real_ends_kernel   fallback inverse: the imaginary parts of bins 0 and cols/2 of every row, which a c2r ignores, set to zero
//
// tile_fft_colpass_kernel is tile_fft_colround_kernel's simpler sibling (fft_kernels_conv2d.h): the same register layout on the tile
// of Pow2Plan::build_columns (E = 8 values per thread, at most 512 threads; slot e of thread (j, r) loads row l = r + TPC * e and
// holds frequency K = r + TPC * e after the stages, of the thread's V columns c0 + V * j ...), but no product and no second run.
//   direction  the inverse is the forward transform between two re <-> im swaps (on the way into and out of the registers)
//   scale      applied at the store
//   rows       in_ld / out_ld elements apart, matrices in_b / out_b apart: the two sides have pitches of their own, because one of
//              them is the caller's [rows][L + 1] spectrum (rows only sizeof(cpx<T>)-aligned in fp32) and the other the plan's image
//   in_vec / out_vec   1: base, row pitch and matrix pitch of that side are multiples of 16 bytes and a thread's V columns move as
//              one 16-byte access; 0: value by value
//   n_cols     live columns.  A column at or beyond n_cols (the last tile of a matrix) is dead on both sides: zeros in, nothing
//              read, nothing stored -- a 16-byte access that would straddle n_cols is done value by value under that predicate, so
//              the padding behind a row of the plan's image is never read either
// Every matrix has tiles of its own, and the columns of a tile never mix: a NaN stays in its matrix and column.
// The next tile's loads are issued before the stages of the current one.
#pragma once

#include "fft_kernels.h"
#include "fft_kernels_chain.h"

namespace fftk {

template <typename T>
struct ColPassParams {
    const cpx<T>* in;      // [matrices][P][in_ld]
    cpx<T>* out;           // [matrices][P][out_ld]
    const cpx<T>* tables;  // the column pass's blob [ sa | sb ] (no inter-pass twiddle)
    int group_bytes, tables_bytes, off_tables, o_sb, sa_bits;
    int log2L, log2C;      // L = P rows, C columns per tile
    int n_ct;              // column tiles per matrix
    int n_cols;            // live columns
    long long in_b, out_b;    // elements between matrices
    long long in_ld, out_ld;  // elements between rows
    long long n_tiles;     // matrices * n_ct
    int in_vec, out_vec;   // 16-byte accesses on that side
    int inverse;
    int nt;                // non-temporal hint on the 16-byte accesses: bit 0 loads, bit 1 stores (TileParams::nt)
    T scale;
};

template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS2(512, FFT_CHAIN_WAVES_PER_SIMD) tile_fft_colpass_kernel(ColPassParams<T> p) {
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
        const int c = c0 + V * j;
        const bool whole = p.in_vec && c + V <= p.n_cols;  // all V columns live, 16-byte aligned
        const cpx<T>* src = p.in + m * p.in_b + c;
        FFT_UNROLL
        for (int e = 0; e < E; e++) {
            const long long l = r + ((long long)e << log2TPC);
            if (whole) {
                nxt[e] = fft_ld16<NTL>(reinterpret_cast<const vec16<T>*>(src + l * p.in_ld));
            } else {
                FFT_UNROLL
                for (int vv = 0; vv < V; vv++) {
                    nxt[e].c[vv] = mk<T>((T)0, (T)0);
                    if (c + vv < p.n_cols) nxt[e].c[vv] = src[l * p.in_ld + vv];
                }
            }
        }
    };
    auto prefetch = [&](long long tile) __attribute__((always_inline)) {  // one wave-uniform branch per tile
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
        const int c = c0 + V * j;

        if (p.inverse) {
            FFT_UNROLL
            for (int e = 0; e < E; e++) {
                FFT_UNROLL
                for (int vv = 0; vv < V; vv++) x[0][e][vv] = cswap(nxt[e].c[vv]);
            }
        } else {
            FFT_UNROLL
            for (int e = 0; e < E; e++) {
                FFT_UNROLL
                for (int vv = 0; vv < V; vv++) x[0][e][vv] = nxt[e].c[vv];
            }
        }
        FFT_SCHED_BARRIER();
        if (tile + tile_step < n_tiles) prefetch(tile + tile_step);  // behind the stages and the store
        FFT_SCHED_BARRIER();

        FFT_SYNC_LDS();  // the previous tile's last exchange is fully consumed
        stockham_all_stages<T, E, FAM_SR16, V, H>(x, smem, p.group_bytes, tw, r, j, log2J, log2TPC, log2L, []() {});

        // slot e holds frequency K = r + TPC * e
        cpx<T>* outp = p.out + m * p.out_b + c;
        const bool whole = p.out_vec && c + V <= p.n_cols;
        auto store_as = [&](auto nt_tag) __attribute__((always_inline)) {
            constexpr int NTS = decltype(nt_tag)::value;
            FFT_UNROLL
            for (int e = 0; e < E; e++) {
                const long long K = r + ((long long)e << log2TPC);
                vec16<T> v;
                FFT_UNROLL
                for (int vv = 0; vv < V; vv++) v.c[vv] = cscale(p.inverse ? cswap(x[0][e][vv]) : x[0][e][vv], p.scale);
                if (whole) {
                    fft_st16<NTS>(reinterpret_cast<vec16<T>*>(outp + K * p.out_ld), v);
                } else {
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++)
                        if (c + vv < p.n_cols) outp[K * p.out_ld + vv] = v.c[vv];
                }
            }
        };
        if (nt_store) store_as(std::integral_constant<int, 1>{});
        else store_as(std::integral_constant<int, 0>{});
    }
}

// y[m * y_pitch + i] = w[m * w_pitch + i], i < per values of type E (T or cpx<T>), value by value; total = matrices * per
template <typename E>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) real2d_copy_kernel(const E* w, long long w_pitch, E* y, long long y_pitch, long long per, long long total) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < total; i += stride) {
        const long long m = i / per;
        y[m * y_pitch + (i - m * per)] = w[m * w_pitch + (i - m * per)];
    }
}

// X[i][0].im = 0 and -- last != 0 -- X[i][hb - 1].im = 0 for the n_rows one-sided rows of hb bins: the fallback's c2r (RealPlan) reads
// the imaginary parts of those bins, numpy.fft.irfft ignores them
template <typename T>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) real2d_real_ends_kernel(cpx<T>* X, int hb, int last, long long n_rows) {
    const long long stride = FFT_NBLOCKS * FFT_NTHREADS;
    for (long long i = FFT_BID * FFT_NTHREADS + FFT_TID; i < n_rows; i += stride) {
        X[i * hb].im = (T)0;
        if (last) X[i * hb + hb - 1].im = (T)0;
    }
}

}  // namespace fftk
