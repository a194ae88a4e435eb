// fft_team_quad.hip -- the device instantiations of team_quad_kernel (fft_team_quad.h; the list: fft_team_quad_decl.h) and of
// wide_row_kernel (fft_wide_row.h, with its list): 512-thread workgroups, one per CU.
#include "fft_team_quad.h"
#include "fft_wide_row.h"

namespace fftk {
#define FFT_QUAD_DEFINE(T, ...) template __global__ void team_quad_kernel<T, __VA_ARGS__>(TeamParams<T>);
FFT_QUAD_INSTANCES(FFT_QUAD_DEFINE)
#undef FFT_QUAD_DEFINE
#define FFT_WIDE_DEFINE(T, LOG2L, E) template __global__ void wide_row_kernel<T, LOG2L, E>(WideParams<T>);
FFT_WIDE_INSTANCES(FFT_WIDE_DEFINE)
#undef FFT_WIDE_DEFINE
}
