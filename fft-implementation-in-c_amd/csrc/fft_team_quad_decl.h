// fft_team_quad_decl.h -- declaration of team_quad_kernel (fft_team_quad.h).  The device build compiles the kernel in a
// translation unit of its own (fft_team_quad.hip: seconds instead of the backend's minutes); the planner (fft_engine.h) only
// needs the declaration to launch it.  The CPU emulation includes the body directly.
#pragma once

#include <type_traits>

#include "fft_team.h"

namespace fftk {

#if defined(FFT_EMU)
#define FFT_QUAD_BOUNDS(LOG2RA, LOG2L2, LOG2TS)
#else
// NTHR = (L2 / TS) * RA threads, all resident on one CU: NTHR / 256 waves per SIMD
#define FFT_QUAD_BOUNDS(LOG2RA, LOG2L2, LOG2TS) __launch_bounds__((((1 << (LOG2L2)) >> (LOG2TS)) << (LOG2RA)), ((((1 << (LOG2L2)) >> (LOG2TS)) << (LOG2RA))) / 256)
#endif
template <typename T, int E, int LOG2RA, int LOG2RB, int LOG2L1, int LOG2L2, int LOG2TS, int SLOTS>
FFT_KERNEL void FFT_QUAD_BOUNDS(LOG2RA, LOG2L2, LOG2TS) team_quad_kernel(TeamParams<T> p);

// THE list of built shapes: <T, E, log2 RA, log2 RB, log2 L1, log2 L2, log2 TS, SLOTS (the exchange protocol: 1 / 2 window slots with the
// team's arrival counter, 3 = one image per seat and the pair protocol)>.  The instantiations (fft_team_quad.hip), their extern declarations
// (below), what the planner takes for built (quad_E, quad_slots) and its dispatch (Pow2Plan::launch_team_quad) all come from it: a new
// instantiation is one row here.  Where a shape has several protocols, its FIRST row is what a request for one that is not built falls back to.
#if defined(FFT_EMU)
// the emulation: E = 4, both precisions; n = 2^12 (teams of 4), 2^11 (of 2 and 4), 2^10 (of 1, 2 and 4)
#define FFT_QUAD_EMU_ROW(X, ...) X(float, __VA_ARGS__) X(double, __VA_ARGS__)
#define FFT_QUAD_INSTANCES(X)                  \
    FFT_QUAD_EMU_ROW(X, 4, 2, 2, 6, 6, 2, 2)   \
    FFT_QUAD_EMU_ROW(X, 4, 2, 2, 6, 6, 2, 3) /* the pair protocol (the device's n = 2^20) on teams of 4 and of 2 */ \
    FFT_QUAD_EMU_ROW(X, 4, 2, 1, 6, 5, 1, 2)   \
    FFT_QUAD_EMU_ROW(X, 4, 2, 1, 6, 5, 1, 3)   \
    FFT_QUAD_EMU_ROW(X, 4, 2, 1, 6, 5, 2, 1)   \
    FFT_QUAD_EMU_ROW(X, 4, 2, 1, 6, 5, 2, 3)   \
    FFT_QUAD_EMU_ROW(X, 4, 1, 1, 5, 5, 0, 1)   \
    FFT_QUAD_EMU_ROW(X, 4, 1, 1, 5, 5, 1, 1)   \
    FFT_QUAD_EMU_ROW(X, 4, 1, 1, 5, 5, 1, 3)   \
    FFT_QUAD_EMU_ROW(X, 4, 1, 1, 5, 5, 2, 1)   \
    FFT_QUAD_EMU_ROW(X, 4, 1, 1, 5, 5, 2, 3)
#else
#define FFT_QUAD_INSTANCES(X)                                                                                         \
    X(float, 16, 4, 4, 10, 10, 5, 2) /* n = 2^20: 1024 x 1024, teams of 32 (a whole XCD), two window slots */          \
    X(float, 16, 4, 4, 10, 10, 5, 1) /* ... with one (experiments: FFT_HIP_QUAD_SLOTS=1; traffic 1.08 x, but -20 %) */ \
    X(float, 16, 4, 4, 10, 10, 5, 3) /* ... ONE image per seat and the pair protocol (per-seat counters, no team-wide wait) */ \
    X(float, 16, 4, 3, 10, 9, 4, 2)  /* n = 2^19: 1024 x 512, teams of 16 */                                           \
    X(float, 16, 4, 3, 10, 9, 4, 1)                                                                                    \
    X(float, 16, 4, 3, 10, 9, 4, 3)                                                                                    \
    X(float, 16, 3, 3, 9, 9, 3, 1)   /* n = 2^18: 512 x 512, teams of 8, one window slot */                            \
    X(float, 16, 3, 3, 9, 9, 3, 2)   /* ... two (experiments) */                                                       \
    X(float, 16, 3, 3, 9, 9, 3, 3)   /* ... pair protocol */                                                           \
    X(float, 16, 3, 2, 9, 8, 2, 1)   /* n = 2^17: 512 x 256, teams of 4 */                                             \
    X(float, 16, 3, 2, 9, 8, 2, 3)                                                                                     \
    X(float, 16, 2, 2, 8, 8, 1, 1)   /* n = 2^16: 256 x 256, teams of 2 */                                             \
    X(float, 16, 2, 1, 8, 7, 0, 1)   /* n = 2^15: 256 x 128, one CU per transform */                                   \
    X(double, 8, 3, 1, 8, 6, 0, 1)   /* fp64 n = 2^14: 256 x 64, one CU per transform */                               \
    X(double, 8, 3, 2, 8, 7, 1, 1)   /* fp64 n = 2^15: 256 x 128, teams of 2 */                                        \
    X(double, 8, 3, 3, 8, 8, 2, 1)   /* fp64 n = 2^16: 256 x 256, teams of 4 */
// Measured and NOT instantiated (round 4, profiles/r4_ab_fp64_quad_e16.txt): fp64 n = 2^17 ... 2^19 with 16 values per thread and chunk on
// 256-thread workgroups (one wave per SIMD, 512 registers per wave: <double, 16, 4, 3, 10, 9, 5, 2>, <double, 16, 3, 3, 9, 9, 4, 1 / 2>,
// <double, 16, 3, 2, 9, 8, 3, 1>).  Correct (parity-green on the device), but 41 - 73 registers still spill and one wave per SIMD hides no
// latency: 75 / 75 / 84 Gpoint/s against 88 - 91 / 97 - 101 / 103 - 107 of round 2's team_defer_kernel, which keeps those sizes.
#define FFT_QUAD_EXTERN(T, ...) extern template __global__ void team_quad_kernel<T, __VA_ARGS__>(TeamParams<T>);
FFT_QUAD_INSTANCES(FFT_QUAD_EXTERN)
#undef FFT_QUAD_EXTERN
#endif

// values per thread and chunk of the shapes built for <T, log2 n>; 0: none
template <typename T>
constexpr int quad_E(int log2n) {
#define FFT_QUAD_ROW(TT, E, RA, RB, L1, L2, TS, SLOTS) \
    if (std::is_same<T, TT>::value && log2n == (L1) + (L2)) return E;
    FFT_QUAD_INSTANCES(FFT_QUAD_ROW)
#undef FFT_QUAD_ROW
    return 0;
}
// the protocol that runs <T, log2 n, log2 TS> when `want` is asked for: `want` itself if that row is built (so == want is the "is it built"
// query), else the shape's first row; 0: no row of that shape
template <typename T>
constexpr int quad_slots(int log2n, int log2TS, int want) {
    int first = 0;
#define FFT_QUAD_ROW(TT, E, RA, RB, L1, L2, TS, SLOTS)                             \
    if (std::is_same<T, TT>::value && log2n == (L1) + (L2) && log2TS == (TS)) {  \
        if (want == (SLOTS)) return want;                                          \
        if (!first) first = SLOTS;                                                 \
    }
    FFT_QUAD_INSTANCES(FFT_QUAD_ROW)
#undef FFT_QUAD_ROW
    return first;
}
#if !defined(FFT_EMU)
static_assert(quad_slots<float>(17, 2, 2) == 1 && quad_slots<float>(16, 1, 3) == 1 && quad_slots<float>(15, 0, 2) == 1 && quad_slots<double>(16, 2, 3) == 1 &&
                  quad_slots<float>(18, 3, 1) == 1 && quad_slots<float>(20, 5, 2) == 2 && quad_slots<float>(19, 4, 2) == 2,
              "what a protocol request resolves to where it is not built");
#endif

}  // namespace fftk
