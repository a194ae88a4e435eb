// fft_kernels_plane.h -- plane_fft_kernel: the 2D transform of whole contiguous P x Q planes (P rows, Q = cols, both powers of two >= 8)
// inside LDS, the first launch of the 3D plan (fft_plans_ext.h Plan3D): one HBM round trip transforms two of a volume's three axes.
//
// Algebra.  A 2D transform of a P x Q plane is the four-step transform of P * Q points without the inter-step twiddle and without the
// last transpose: Q-point transforms along the rows, then P-point transforms along the columns, on one image that never leaves LDS.
//
// Tile.  A workgroup walks tiles with a grid stride; a tile is G = 2^log2G whole planes (G > 1 only for small planes, so that a
// workgroup has at least a few waves of work), TR = G * P rows of Q values, ONE contiguous stretch of G * P * Q values in memory.  It
// is loaded with 16-byte accesses, every byte once: chunk g = tid + i * nthreads is row g / (Q / V), position g % (Q / V).  Planes at
// or past n_planes (the last tile's padding) are neither read nor written.  A tile is loaded completely before any of it is stored and
// tiles are disjoint: in == out works, and planes never mix.
//
// LDS layout:   [ image: TR rows, Q * sizeof(cpx<T>) + 16 bytes apart | exchange area of one strip | W_Q^m, m < Q | W_P^m, m < P ]
// The 16 bytes of padding per row are the tile kernels': the row step reads a thread's V rows (adjacent lanes: rows V apart), the
// column step reads 16 bytes of V adjacent columns (adjacent lanes: adjacent chunks of a row, rows by the lane's r), both without a
// systematic bank conflict.
//
// Strips.  Both steps run on strips that have the register layout of the stage code (stockham_all_stages, E = 4 values per thread,
// radix-4 stages, thread (r, j): j = tid mod J picks V adjacent transforms, r = tid div J the elements r + TPC * e).
//   row step     strip s = rows s * SR ... of the tile (SR = nthreads * 4 V / Q): slot e of thread (r, j) <- image[s SR + V j + vv][r + Q/4 e]
//   column step  strip s = tile columns s * SC ... (SC = nthreads * 4 V / P; tile column cc = plane cc / Q, column cc % Q):
//                slot e <- the 16 bytes image[plane][r + P/4 e][c .. c + V)
// A strip's values live in registers during its stages, which exchange through the exchange area (nthreads * 4 V values); afterwards
// slot e holds frequency r + TPC * e, the shape it was loaded in, and goes back to the same place of the image.  A strip touches only
// its own rows / columns of the image, so the only barriers between strips are those that hand over the exchange area.
// Strip rule (Plan3D::choose_plane): nthreads = the largest power of two <= min(512, G P Q / 4V) for which image + exchange + tables
// fit the LDS budget; nthreads >= max(P, Q) / 4, or the plan takes its composition.  The plan takes only tiles of at most two strips per
// step (NPF > 0 below): measured, the many-strip tiles lose to the composition (Plan3D::take_unprefetched).
//
// Prefetch.  NPF > 0: the tile is NPF 16-byte chunks per thread (NPF = 4 one strip per step, 8 two), and the second image lives in
// registers: the next tile's loads are issued into `nxt` right after this tile's chunks moved to LDS and fly during both steps and the
// store (every barrier in between is LDS-only).  NPF = 0 (more chunks per thread than registers should hold): the loads are issued
// after the last read of the image -- the store loop of the previous tile -- and go to LDS as they land, wide_row_kernel's INPLACE rule.
//
// Inverse: the forward transform between two re <-> im swaps, one on the way into the row step's registers, one at the store, where the
// scale 1 / (P * Q) is applied too.
#pragma once

#include "fft_kernels.h"

namespace fftk {

template <typename T>
struct PlaneParams {
    const cpx<T>* in;
    cpx<T>* out;
    const cpx<T>* tables;  // [ W_Q^m, m < Q | W_P^m, m < P ]
    int log2P, log2Q;      // rows and cols of a plane
    int log2G;             // planes per tile
    int log2SR, log2SC;    // rows of a row-step strip, tile columns of a column-step strip
    int off_exch, off_tables, tables_bytes;
    long long n_planes, n_tiles;
    int inverse;
    T scale;               // applied at the store of the inverse
};

template <typename T, int NPF>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(512) plane_fft_kernel(PlaneParams<T> p) {
    constexpr int E = 4, H = 1;
    constexpr int V = vec16<T>::V;
    constexpr int log2V = Log2<V>::value;
    constexpr int log2E = Log2<E>::value;
    constexpr int SZ = (int)sizeof(cpx<T>);
    FFT_DYN_SMEM(smem);

    const int tid = FFT_TID;
    const int nthreads = FFT_NTHREADS;
    const int log2P = p.log2P, log2Q = p.log2Q;
    const int Q = 1 << log2Q;
    const int pitch = Q * SZ + 16;      // bytes between the rows of the LDS image
    const int log2CPR = log2Q - log2V;  // 16-byte chunks per row
    const int cpr_mask = (1 << log2CPR) - 1;
    const int log2TR = p.log2G + log2P;  // rows of a tile
    const int n_chunks = 1 << (log2TR + log2CPR);
    const long long total_rows = p.n_planes << log2P;
    const long long tile_step = FFT_NBLOCKS;
    const bool inverse = p.inverse != 0;
    unsigned char* exch = smem + p.off_exch;

    {  // stage tables -> LDS
        const vec16<T>* src = reinterpret_cast<const vec16<T>*>(p.tables);
        vec16<T>* dst = reinterpret_cast<vec16<T>*>(smem + p.off_tables);
        for (int i = tid; i < (p.tables_bytes >> 4); i += nthreads) dst[i] = src[i];
    }
    const cpx<T>* tab = reinterpret_cast<const cpx<T>*>(smem + p.off_tables);
    StageTw<T> twq, twp;  // single-level tables
    twq.sa = tab; twq.sb = tab; twq.sa_bits = log2Q; twq.log2L = log2Q;
    twp.sa = tab + Q; twp.sb = tab + Q; twp.sa_bits = log2P; twp.log2L = log2P;

    // chunk g of tile `tile`: global chunk index and whether its plane exists
    auto chunk_live = [&](long long tile, int g) __attribute__((always_inline)) -> bool {
        return (tile << log2TR) + (g >> log2CPR) < total_rows;
    };
    auto image_chunk = [&](int g) __attribute__((always_inline)) -> vec16<T>* {
        return reinterpret_cast<vec16<T>*>(smem + (size_t)(g >> log2CPR) * pitch + (size_t)(g & cpr_mask) * 16);
    };

    vec16<T> nxt[NPF > 0 ? NPF : 1];
    auto prefetch = [&](long long tile) __attribute__((always_inline)) {
        const vec16<T>* src = reinterpret_cast<const vec16<T>*>(p.in) + (tile << (log2TR + log2CPR));
        FFT_UNROLL
        for (int i = 0; i < NPF; i++) {
            const int g = tid + i * nthreads;
            FFT_UNROLL
            for (int vv = 0; vv < V; vv++) nxt[i].c[vv] = mk<T>((T)0, (T)0);
            if (chunk_live(tile, g)) nxt[i] = fft_ld16<0>(src + g);
        }
    };

    const long long tile0 = FFT_BID;
    if (NPF > 0 && tile0 < p.n_tiles) prefetch(tile0);
    FFT_SYNC();  // tables visible

    for (long long tile = tile0; tile < p.n_tiles; tile += tile_step) {
        cpx<T> x[H][E][V];

        // ---- the tile -> its LDS image
        FFT_SYNC_LDS();  // the previous tile's image is consumed
        if (NPF > 0) {
            FFT_UNROLL
            for (int i = 0; i < NPF; i++) *image_chunk(tid + i * nthreads) = nxt[i];
            FFT_SCHED_BARRIER();
            if (tile + tile_step < p.n_tiles) prefetch(tile + tile_step);  // flies during both steps and the store
            FFT_SCHED_BARRIER();
        } else {
            const vec16<T>* src = reinterpret_cast<const vec16<T>*>(p.in) + (tile << (log2TR + log2CPR));
            for (int g = tid; g < n_chunks; g += nthreads) {
                vec16<T> v;
                FFT_UNROLL
                for (int vv = 0; vv < V; vv++) v.c[vv] = mk<T>((T)0, (T)0);
                if (chunk_live(tile, g)) v = fft_ld16<0>(src + g);
                *image_chunk(g) = v;
            }
        }
        FFT_SYNC_LDS();

        {  // ---- row step: TR transforms of length Q, SR rows at a time
            const int log2J = p.log2SR - log2V;
            const int log2TPC = log2Q - log2E;
            const int j = tid & ((1 << log2J) - 1), r = tid >> log2J;
            const int n_strips = 1 << (log2TR - p.log2SR);
            for (int s = 0; s < n_strips; s++) {
                unsigned char* rows = smem + (size_t)((s << p.log2SR) + V * j) * pitch;
                FFT_UNROLL
                for (int e = 0; e < E; e++) {
                    const int l = r + (e << log2TPC);
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++) {
                        const cpx<T> v = *reinterpret_cast<const cpx<T>*>(rows + (size_t)vv * pitch + (size_t)l * SZ);
                        x[0][e][vv] = inverse ? cswap(v) : v;
                    }
                }
                stockham_all_stages<T, E, FAM_R4, V, H>(x, exch, 0, twq, r, j, log2J, log2TPC, log2Q, []() {});
                FFT_SYNC_LDS();  // the last exchange is consumed (the next strip's first stage writes it)
                FFT_UNROLL
                for (int e = 0; e < E; e++) {
                    const int K = r + (e << log2TPC);
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++) *reinterpret_cast<cpx<T>*>(rows + (size_t)vv * pitch + (size_t)K * SZ) = x[0][e][vv];
                }
            }
        }
        FFT_SYNC_LDS();  // every row of the image is transformed

        {  // ---- column step: G * Q transforms of length P, SC tile columns at a time
            const int log2J = p.log2SC - log2V;
            const int log2TPC = log2P - log2E;
            const int j = tid & ((1 << log2J) - 1), r = tid >> log2J;
            const int n_strips = 1 << (p.log2G + log2Q - p.log2SC);
            for (int s = 0; s < n_strips; s++) {
                const int cc = (s << p.log2SC) + V * j;  // the first of the thread's V tile columns: plane cc / Q, column cc % Q
                unsigned char* col = smem + (size_t)((cc >> log2Q) << log2P) * pitch + (size_t)(cc & (Q - 1)) * SZ;
                FFT_UNROLL
                for (int e = 0; e < E; e++) {
                    const vec16<T> v = *reinterpret_cast<const vec16<T>*>(col + (size_t)(r + (e << log2TPC)) * pitch);
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++) x[0][e][vv] = v.c[vv];
                }
                stockham_all_stages<T, E, FAM_R4, V, H>(x, exch, 0, twp, r, j, log2J, log2TPC, log2P, []() {});
                FFT_SYNC_LDS();  // the last exchange is consumed
                FFT_UNROLL
                for (int e = 0; e < E; e++) {
                    vec16<T> v;
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++) v.c[vv] = x[0][e][vv];
                    *reinterpret_cast<vec16<T>*>(col + (size_t)(r + (e << log2TPC)) * pitch) = v;
                }
            }
        }
        FFT_SYNC_LDS();  // the image holds the tile's spectra

        // ---- the image -> the tile's own place in out
        {
            vec16<T>* dst = reinterpret_cast<vec16<T>*>(p.out) + (tile << (log2TR + log2CPR));
            for (int g = tid; g < n_chunks; g += nthreads) {
                if (!chunk_live(tile, g)) continue;
                vec16<T> v = *image_chunk(g);
                if (inverse) {
                    FFT_UNROLL
                    for (int vv = 0; vv < V; vv++) v.c[vv] = mk<T>(v.c[vv].im * p.scale, v.c[vv].re * p.scale);
                }
                fft_st16<0>(dst + g, v);
            }
        }
    }
}

// The instantiations -- NPF = 0, 4, 8 in both precisions -- are compiled in a translation unit of their own (fft_plane.hip), so that the
// backend's device code is what it was without this kernel; the planner (fft_plans_ext.h) sees extern declarations.
#define FFT_PLANE_INSTANCES(X) X(float, 0) X(float, 4) X(float, 8) X(double, 0) X(double, 4) X(double, 8)
#if !defined(FFT_EMU) && !defined(FFT_PLANE_DEFINE_HERE)
#define FFT_PLANE_EXTERN(T, NPF) extern template __global__ void plane_fft_kernel<T, NPF>(PlaneParams<T>);
FFT_PLANE_INSTANCES(FFT_PLANE_EXTERN)
#undef FFT_PLANE_EXTERN
#endif

}  // namespace fftk
