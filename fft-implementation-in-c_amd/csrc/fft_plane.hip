// fft_plane.hip -- the device instantiations of plane_fft_kernel (fft_kernels_plane.h, with its list), the first launch of the 3D plan.
#define FFT_PLANE_DEFINE_HERE
#include "fft_kernels_plane.h"

namespace fftk {
#define FFT_PLANE_DEFINE(T, NPF) template __global__ void plane_fft_kernel<T, NPF>(PlaneParams<T>);
FFT_PLANE_INSTANCES(FFT_PLANE_DEFINE)
#undef FFT_PLANE_DEFINE
}
