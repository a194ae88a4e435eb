// fft_mixed_radix.h -- Stockham mixed-radix tile kernel for 7-smooth lengths n = 2^a 3^b 5^c 7^d.
//
// One kernel, three uses (ffteng::MixedRadixPlan, fft_engine.h):
//   single pass   n <= 4096        a tile = C whole transforms (rows of length L = n), rows in, rows out
//   pass A        n = n1 * n2      a tile = C adjacent columns j2 of one transform, sub-transform length L = n1 over
//                                  stride n2, result times W_n^(k1 j2), stored in the same [k1][j2] shape into scratch
//   pass B                         a tile = C adjacent rows k1 of the scratch image, L = n2, stored transposed
//                                  (out[k2 n1 + k1]: C contiguous values per k2), which leaves natural order
// A tile lives in LDS as [c][l] with an ODD pitch P (L or L + 1): lanes that walk along l and lanes that walk along c
// both spread over the banks.  Stages are Stockham autosort steps between two LDS images, radix 2, 3, 4, 5, 7 or 8 with
// the butterfly in registers; the host hands over the schedule as (radix, Ns = product of the earlier radices,
// m = L / radix).  Butterfly u of a tile splits as c = u / m, j = u % m, k = j % Ns: neither m nor Ns is a power of two,
// so the host also passes ceil(2^32 / d) for each and the kernel takes a multiply-high (exact for u < 2^16, d <= 4096:
// u (M d - 2^32) < u d < 2^32).  Twiddles W_L^i come from an LDS table: one level for L <= 1024, hi[i >> 6] * lo[i & 63]
// above; the inter-pass twiddle W_n^m of pass A from two or three LDS tables of 256 entries (m split into bytes).
// Skeleton as in tile_fft_kernel: persistent workgroups walk the tiles, the next tile's loads are issued into registers
// before this tile's stages, the barriers order LDS traffic only, the inverse is the re<->im swap on the first load and the
// last store, the 1/n rides on the last store.  16-byte global accesses where the host found every access aligned
// (in_vec / out_vec), 8-byte ones otherwise (fp32 at odd pitches); every access is predicated on the tile's valid range.
#pragma once

#include "fft_codelets.h"
#include "fft_device.h"

namespace fftk {

constexpr int MR_MAX_STAGES = 8;
enum { MR_ROWS = 0, MR_COLS = 1 };  // which index is contiguous in global memory: l (rows) or c (columns)

struct MrStage {
    int radix, Ns, m, tws;    // tws = L / (Ns * radix): W_(Ns radix)^(q k) = W_L^(q k tws)
    unsigned mag_Ns, mag_m;   // ceil(2^32 / Ns), ceil(2^32 / m) (unused where the divisor is 1)
};

template <typename T>
struct MixedParams {
    const cpx<T>* in;
    cpx<T>* out;
    const cpx<T>* tables;     // [ W_L: one level, or lo(64) | hi ] [ W_n bytes 0 | 1 | 2 ]
    MrStage st[MR_MAX_STAGES];
    int nst;
    int L, P, C, log2C;       // sub-transform length, LDS pitch, sub-transforms per tile (a power of two where a side is MR_COLS)
    unsigned mag_L;
    int in_mode, out_mode, in_vec, out_vec;
    int n_sub;                // sub-transforms per transform
    int tpt;                  // tiles per transform
    long long ntiles;
    long long tr_stride;      // elements between transforms
    long long in_stride, out_stride;  // MR_COLS: elements between successive l / k
    int tables_elems, tw_two, o_hi;
    int ptw_levels, o_p0, o_p1, o_p2;  // pass A: levels of the W_n table (0: no inter-pass twiddle)
    int swap_in, swap_out;
    T scale;
};

FFT_DEVICE unsigned mr_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
FFT_DEVICE unsigned mr_div(unsigned x, int d, unsigned mag) { return d == 1 ? x : mr_mulhi(x, mag); }

// cos / sin of 2 pi i / R for the odd radices
template <int R>
FFT_DEVICE constexpr double mr_cos(int i) {
    const int j = i > R / 2 ? R - i : i;
    if (R == 3) return j == 0 ? 1.0 : -0.5;
    if (R == 5) return j == 0 ? 1.0 : j == 1 ? 0.30901699437494742410 : -0.80901699437494742410;
    return j == 0 ? 1.0 : j == 1 ? 0.62348980185873353053 : j == 2 ? -0.22252093395631440429 : -0.90096886790241912624;
}
template <int R>
FFT_DEVICE constexpr double mr_sin(int i) {
    const int j = i > R / 2 ? R - i : i;
    const double sg = i > R / 2 ? -1.0 : 1.0;
    if (R == 3) return j == 0 ? 0.0 : sg * 0.86602540378443864676;
    if (R == 5) return j == 0 ? 0.0 : sg * (j == 1 ? 0.95105651629515357212 : 0.58778525229247312917);
    return j == 0 ? 0.0 : sg * (j == 1 ? 0.78183148246802980871 : j == 2 ? 0.97492791218182360702 : 0.43388373911755812048);
}

// forward DFT of odd length R in registers: X_k = x_0 + sum_q (a_q cos(2 pi q k / R) - i b_q sin(2 pi q k / R)) with
// a_q = x_q + x_(R-q), b_q = x_q - x_(R-q); X_(R-k) takes the other sign
template <typename T, int R>
FFT_DEVICE void mr_dft_odd(cpx<T>* v) {
    constexpr int H = (R - 1) / 2;
    cpx<T> a[H + 1], b[H + 1], y[R];
    FFT_UNROLL
    for (int q = 1; q <= H; q++) {
        a[q] = cadd(v[q], v[R - q]);
        b[q] = csub(v[q], v[R - q]);
    }
    y[0] = v[0];
    FFT_UNROLL
    for (int q = 1; q <= H; q++) y[0] = cadd(y[0], a[q]);
    FFT_UNROLL
    for (int k = 1; k <= H; k++) {
        cpx<T> p = v[0], s = mk<T>((T)0, (T)0);
        FFT_UNROLL
        for (int q = 1; q <= H; q++) {
            const T c = (T)mr_cos<R>((q * k) % R), sn = (T)mr_sin<R>((q * k) % R);
            p = mk<T>(p.re + a[q].re * c, p.im + a[q].im * c);
            s = mk<T>(s.re + b[q].re * sn, s.im + b[q].im * sn);
        }
        y[k] = cadd_mni(p, s);
        y[R - k] = csub_mni(p, s);
    }
    FFT_UNROLL
    for (int k = 0; k < R; k++) v[k] = y[k];
}

template <typename T, int R>
FFT_DEVICE void mr_dft(cpx<T>* v) {
    if constexpr (R == 3 || R == 5 || R == 7) mr_dft_odd<T, R>(v);
    else dft_inplace<T, R>(v);
}

template <typename T>
FFT_DEVICE cpx<T> mr_tw(const cpx<T>* tab, int tw_two, int o_hi, unsigned i) {
    if (tw_two) return cmul(tab[o_hi + (i >> 6)], tab[i & 63u]);
    return tab[i];
}

// one Stockham stage of radix R over the `total` = (valid sub-transforms) * m butterflies of the tile
template <typename T, int R>
FFT_DEVICE void mr_stage(const MrStage& s, const cpx<T>* src, cpx<T>* dst, const cpx<T>* tab, int tw_two, int o_hi, int P, int total) {
    const int nt = FFT_NTHREADS;
    for (int idx = FFT_TID; idx < total; idx += nt) {
        const unsigned c = mr_div((unsigned)idx, s.m, s.mag_m);
        const unsigned j = (unsigned)idx - c * (unsigned)s.m;
        const unsigned k = s.Ns == 1 ? 0u : j - mr_mulhi(j, s.mag_Ns) * (unsigned)s.Ns;
        const cpx<T>* a = src + c * (unsigned)P + j;
        cpx<T> v[R];
        FFT_UNROLL
        for (int q = 0; q < R; q++) v[q] = a[q * s.m];
        if (s.Ns > 1) {
            const unsigned ti = k * (unsigned)s.tws;
            unsigned acc = ti;
            FFT_UNROLL
            for (int q = 1; q < R; q++) {
                v[q] = cmul(v[q], mr_tw<T>(tab, tw_two, o_hi, acc));
                acc += ti;
            }
        }
        mr_dft<T, R>(v);
        cpx<T>* d = dst + c * (unsigned)P + (j - k) * R + k;
        FFT_UNROLL
        for (int q = 0; q < R; q++) d[q * s.Ns] = v[q];
    }
}

// element x of a tile on a global side: its (c, l), its offset from the tile's base, and whether it exists
template <typename T>
FFT_DEVICE bool mr_decode(const MixedParams<T>& p, int mode, long long stride, unsigned x, int cv, unsigned& c, unsigned& l, long long& off) {
    if (mode == MR_ROWS) {
        c = mr_div(x, p.L, p.mag_L);
        l = x - c * (unsigned)p.L;
        off = (long long)x;
        return x < (unsigned)(cv * p.L);
    }
    l = x >> p.log2C;
    c = x & (unsigned)(p.C - 1);
    off = (long long)l * stride + c;
    return l < (unsigned)p.L && c < (unsigned)cv;
}

template <typename T, int NE>
FFT_DEVICE void mr_load(const MixedParams<T>& p, const cpx<T>* src, int cv, cpx<T>* r) {
    constexpr int V = 16 / (int)sizeof(cpx<T>);
    const int tid = FFT_TID, nt = FFT_NTHREADS;
    unsigned c, l;
    long long off, off1;
    if (V == 2 && p.in_vec) {
        FFT_UNROLL
        for (int i = 0; i < NE / 2; i++) {
            const unsigned x = 2u * (unsigned)(tid + i * nt);
            const bool ok0 = mr_decode(p, p.in_mode, p.in_stride, x, cv, c, l, off);
            const bool ok1 = mr_decode(p, p.in_mode, p.in_stride, x + 1, cv, c, l, off1);
            if (ok0 && ok1) {
                const vec16<T> v = *reinterpret_cast<const vec16<T>*>(src + off);
                r[2 * i] = v.c[0];
                r[2 * i + 1] = v.c[V - 1];
            } else if (ok0) {
                r[2 * i] = src[off];
            }
        }
    } else {
        FFT_UNROLL
        for (int i = 0; i < NE; i++) {
            const unsigned x = (unsigned)(tid + i * nt);
            if (mr_decode(p, p.in_mode, p.in_stride, x, cv, c, l, off)) r[i] = src[off];
        }
    }
}

template <typename T, int NE>
FFT_DEVICE void mr_to_lds(const MixedParams<T>& p, cpx<T>* buf, int cv, const cpx<T>* r) {
    constexpr int V = 16 / (int)sizeof(cpx<T>);
    const int tid = FFT_TID, nt = FFT_NTHREADS;
    const bool paired = V == 2 && p.in_vec;
    unsigned c, l;
    long long off;
    FFT_UNROLL
    for (int i = 0; i < NE; i++) {
        const unsigned x = paired ? 2u * (unsigned)(tid + (i >> 1) * nt) + (unsigned)(i & 1) : (unsigned)(tid + i * nt);
        if (mr_decode(p, p.in_mode, p.in_stride, x, cv, c, l, off)) buf[c * (unsigned)p.P + l] = p.swap_in ? cswap(r[i]) : r[i];
    }
}

template <typename T>
FFT_DEVICE cpx<T> mr_result(const MixedParams<T>& p, const cpx<T>* fin, const cpx<T>* tab, unsigned c, unsigned k, unsigned col0) {
    cpx<T> v = fin[c * (unsigned)p.P + k];
    if (p.ptw_levels) {
        const unsigned m = k * (col0 + c);
        cpx<T> w = cmul(tab[p.o_p0 + (m & 255u)], tab[p.o_p1 + ((m >> 8) & 255u)]);
        if (p.ptw_levels > 2) w = cmul(w, tab[p.o_p2 + (m >> 16)]);
        v = cmul(v, w);
    }
    v = cscale(v, p.scale);
    return p.swap_out ? cswap(v) : v;
}

template <typename T>
FFT_DEVICE void mr_store(const MixedParams<T>& p, const cpx<T>* fin, const cpx<T>* tab, cpx<T>* dst, int cv, unsigned col0) {
    constexpr int V = 16 / (int)sizeof(cpx<T>);
    const int tid = FFT_TID, nt = FFT_NTHREADS;
    const unsigned total = (unsigned)(p.C * p.L);
    unsigned c, k, c1, k1;
    long long off, off1;
    if (V == 2 && p.out_vec) {
        for (unsigned x = 2u * (unsigned)tid; x < total; x += 2u * (unsigned)nt) {
            const bool ok0 = mr_decode(p, p.out_mode, p.out_stride, x, cv, c, k, off);
            const bool ok1 = mr_decode(p, p.out_mode, p.out_stride, x + 1, cv, c1, k1, off1);
            if (ok0 && ok1) {
                vec16<T> v;
                v.c[0] = mr_result(p, fin, tab, c, k, col0);
                v.c[V - 1] = mr_result(p, fin, tab, c1, k1, col0);
                *reinterpret_cast<vec16<T>*>(dst + off) = v;
            } else if (ok0) {
                dst[off] = mr_result(p, fin, tab, c, k, col0);
            }
        }
    } else {
        for (unsigned x = (unsigned)tid; x < total; x += (unsigned)nt)
            if (mr_decode(p, p.out_mode, p.out_stride, x, cv, c, k, off)) dst[off] = mr_result(p, fin, tab, c, k, col0);
    }
}

// NE: tile elements a thread carries in registers from the prefetch to the LDS image (NE * threads >= C * L)
template <typename T, int NE>
FFT_KERNEL void FFT_LAUNCH_BOUNDS(256) mixed_tile_kernel(MixedParams<T> p) {
    FFT_DYN_SMEM(smem);
    const int tid = FFT_TID, nt = FFT_NTHREADS;
    const int D = (p.C * p.P + 1) & ~1;  // elements of one LDS image (16-byte multiple)
    cpx<T>* buf0 = reinterpret_cast<cpx<T>*>(smem);
    cpx<T>* buf1 = buf0 + D;
    cpx<T>* tab = buf1 + D;
    for (int i = tid; i < p.tables_elems; i += nt) tab[i] = p.tables[i];

    const long long nblocks = FFT_NBLOCKS;
    long long t = FFT_BID;
    int b = (int)(t / p.tpt), ct = (int)(t - (long long)b * p.tpt);
    const int db = (int)(nblocks / p.tpt), dct = (int)(nblocks - (long long)db * p.tpt);
    const long long in_tile = p.in_mode == MR_ROWS ? (long long)p.C * p.L : (long long)p.C;
    const long long out_tile = p.out_mode == MR_ROWS ? (long long)p.C * p.L : (long long)p.C;

    cpx<T> r[NE];
    if (t < p.ntiles) {
        const int cv = p.n_sub - ct * p.C < p.C ? p.n_sub - ct * p.C : p.C;
        mr_load<T, NE>(p, p.in + (long long)b * p.tr_stride + ct * in_tile, cv, r);
    }
    while (t < p.ntiles) {
        const int cv = p.n_sub - ct * p.C < p.C ? p.n_sub - ct * p.C : p.C;
        const int b_now = b, ct_now = ct;
        mr_to_lds<T, NE>(p, buf0, cv, r);
        FFT_SYNC_LDS();
        // the next tile's loads fly during this tile's stages
        t += nblocks;
        b += db;
        ct += dct;
        if (ct >= p.tpt) { ct -= p.tpt; b++; }
        if (t < p.ntiles) {
            const int cvn = p.n_sub - ct * p.C < p.C ? p.n_sub - ct * p.C : p.C;
            mr_load<T, NE>(p, p.in + (long long)b * p.tr_stride + ct * in_tile, cvn, r);
        }
        cpx<T>* src = buf0;
        cpx<T>* dst = buf1;
        FFT_NOUNROLL
        for (int s = 0; s < p.nst; s++) {
            const MrStage& st = p.st[s];
            const int total = cv * st.m;
            switch (st.radix) {
                case 2: mr_stage<T, 2>(st, src, dst, tab, p.tw_two, p.o_hi, p.P, total); break;
                case 3: mr_stage<T, 3>(st, src, dst, tab, p.tw_two, p.o_hi, p.P, total); break;
                case 4: mr_stage<T, 4>(st, src, dst, tab, p.tw_two, p.o_hi, p.P, total); break;
                case 5: mr_stage<T, 5>(st, src, dst, tab, p.tw_two, p.o_hi, p.P, total); break;
                case 7: mr_stage<T, 7>(st, src, dst, tab, p.tw_two, p.o_hi, p.P, total); break;
                default: mr_stage<T, 8>(st, src, dst, tab, p.tw_two, p.o_hi, p.P, total); break;
            }
            FFT_SYNC_LDS();
            cpx<T>* sw = src;
            src = dst;
            dst = sw;
        }
        mr_store<T>(p, src, tab, p.out + (long long)b_now * p.tr_stride + ct_now * out_tile, cv, (unsigned)(ct_now * p.C));
        FFT_SYNC_LDS();  // the next tile's image overwrites what the store has just read
    }
}

}  // namespace fftk
