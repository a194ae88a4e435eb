// fft_rows_list.h -- the rows-in / rows-out (single-pass) instantiations of tile_fft_kernel.
// They live in their own translation unit (fft_rows_o2.hip) because hipcc -O2 schedules this kernel shape
// measurably better than -O3 (N = 1024 x 65536 fp32: 236 vs 205 Gpoint/s) while the multi-pass shapes prefer -O3.
#pragma once
#include "fft_kernels.h"
// X(T, E, FAM)
#define FFT_ROWS_LIST(X)        \
    X(float, 2, FAM_R2)         \
    X(float, 4, FAM_R4)         \
    X(float, 4, FAM_R2)         \
    X(float, 8, FAM_SR16)       \
    X(float, 8, FAM_R4)         \
    X(float, 8, FAM_R2)         \
    X(double, 2, FAM_R2)        \
    X(double, 4, FAM_R4)        \
    X(double, 4, FAM_R2)        \
    X(double, 8, FAM_SR16)      \
    X(double, 8, FAM_R4)        \
    X(double, 8, FAM_R2)
// the same kernel (E = 4, radix-4: AUTO's single-pass choice) with L and C baked in for the full 64 KiB tile, where that measured
// faster (profiles/r2_ab_rows_fixed.txt: n = 128, 256 fp32 +10...12 %; n >= 512 and every fp64 size LOSE 10...30 % -- the unrolled
// stage loop no longer fits the 128-VGPR budget of this kernel)
// X(T, LOG2L, LOG2C)
#define FFT_ROWS_FIXED_LIST(X) X(float, 7, 6) X(float, 8, 5)
// E = 8, radix-8 (AUTO's single-pass choice from n = 512 up), L and C baked in: fp32 only (profiles/r2_ab_rows_fixed.txt: fp32 +12...14 %
// over the generic E = 8 kernel, +14...26 % over E = 4 radix-4; the fp64 ones lose 30 %, generic E = 8 radix-8 is fp64's best).
// X(T, LOG2L, LOG2C)
#define FFT_ROWS_FIXED8_LIST(X) X(float, 9, 4) X(float, 10, 3) X(float, 11, 2) X(float, 12, 1)
// the variants of the HOOKED single-pass rows kernel (E = 4, radix-4, shape from the parameters): every set of HOOKBIT_* (fft_kernels.h)
// that tile_fft_kernel<T, 4, 1, FAM_R4, LOAD_LCONTIG, STORE_LCONTIG, false, 0, HOOK> is built with.  Pow2Plan::launch_rows_hooked
// (fft_engine.h) expands the list into its dispatch; the entry point that asks for a variant: PLAIN execute_hooked, ROUND
// execute_round, the four FRAMES ones execute_frames (R: real_frames, _POWER: power_out), HERM_ROWS execute_iframes, FILTER
// execute_filter.
// Translation units: FILTER is explicitly instantiated in fft_rows_o2.hip (-O2, FFT_ROWS_FILTER_LIST below) and declared `extern template`
// in the backend; the other seven are implicitly instantiated in the backend unit (-O3) by that dispatch.  A variant that moves between
// the units is compiled differently and runs at another speed.
// X(NAME, bits)
#define FFT_ROWS_HOOK_LIST(X)                                                                        \
    X(PLAIN, HOOKBIT_LOAD | HOOKBIT_STORE)                                                           \
    X(ROUND, HOOKBIT_LOAD | HOOKBIT_STORE | HOOKBIT_ROUND)                                           \
    X(FRAMES, HOOKBIT_LOAD | HOOKBIT_STORE | HOOKBIT_FRAMES)                                         \
    X(FRAMES_POWER, HOOKBIT_LOAD | HOOKBIT_STORE | HOOKBIT_FRAMES | HOOKBIT_POWER)                   \
    X(RFRAMES, HOOKBIT_LOAD | HOOKBIT_STORE | HOOKBIT_FRAMES | HOOKBIT_REAL)                         \
    X(RFRAMES_POWER, HOOKBIT_LOAD | HOOKBIT_STORE | HOOKBIT_FRAMES | HOOKBIT_POWER | HOOKBIT_REAL)   \
    X(HERM_ROWS, HOOKBIT_LOAD | HOOKBIT_HERM)                                                        \
    X(FILTER, HOOKBIT_LOAD | HOOKBIT_STORE | HOOKBIT_ROUND | HOOKBIT_FRAMES | HOOKBIT_BOUND | HOOKBIT_VALID)
namespace fftk {
#define FFT_ROWS_HOOK_ENUM(NAME, bits) ROWS_HOOK_##NAME,
enum RowsHook { FFT_ROWS_HOOK_LIST(FFT_ROWS_HOOK_ENUM) };
#undef FFT_ROWS_HOOK_ENUM
#define FFT_ROWS_HOOK_ENUM(NAME, bits) ROWS_HOOK_BITS_##NAME = (bits),
enum { FFT_ROWS_HOOK_LIST(FFT_ROWS_HOOK_ENUM) };
#undef FFT_ROWS_HOOK_ENUM
// HOOK is a template argument of the kernel, so these values are part of every variant's symbol name: they stay what they were
static_assert(ROWS_HOOK_BITS_PLAIN == 3, "hooked rows kernel, plain: HOOK = 3");
static_assert(ROWS_HOOK_BITS_ROUND == 11, "hooked rows kernel, round trip: HOOK = 11");
static_assert(ROWS_HOOK_BITS_FRAMES == 19, "hooked rows kernel, frames: HOOK = 19");
static_assert(ROWS_HOOK_BITS_FRAMES_POWER == 51, "hooked rows kernel, frames + power: HOOK = 51");
static_assert(ROWS_HOOK_BITS_RFRAMES == 83, "hooked rows kernel, real frames: HOOK = 83");
static_assert(ROWS_HOOK_BITS_RFRAMES_POWER == 115, "hooked rows kernel, real frames + power: HOOK = 115");
static_assert(ROWS_HOOK_BITS_HERM_ROWS == 129, "hooked rows kernel, Hermitian rows: HOOK = 129");
static_assert(ROWS_HOOK_BITS_FILTER == 795, "hooked rows kernel, filter: HOOK = 795");
}  // namespace fftk
// the FILTER variant's explicit instantiations (the overlap-save filter kernel: FilterPlan, fft_plans_ext.h)
// X(T)
#define FFT_ROWS_FILTER_LIST(X) X(float) X(double)
