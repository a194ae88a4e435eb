// emu_dct.cpp -- the cosine / sine transform plans (fft_plans_ext.h DctPlan, Dct2DPlan; fft_kernels_dct.h) under the CPU emulation, as a
// library of its own.  TEST INFRASTRUCTURE ONLY.  The emulation's runtime is emu_fft.cpp's.
#include "emu_fft.cpp"

// What fft_gpu_plan_dct_hip builds and fft_gpu_execute_dct_hip runs: one execute of `in` into `out` (in == out: in place).  Pitches in
// reals between rows, 0: dense.  flags: bit 0 no_fusion.  Returns 0, -1 the plan was refused, -2 the execute was (nothing was launched).
// info: [0] fused (1 / 0), [1] kernel launches of the execute, [2] rows per tile of the fused kernel (0: none)
template <typename T>
static int run_dct(const void* in, long long in_pitch, void* out, long long out_pitch, int n, int batch, int type, int norm, int flags, int* info) {
    emu::Runtime rt;
    ffteng::DctPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, n, batch, type, norm)) return -1;
    plan.set_no_fusion((flags & 1) != 0);
    if (info) {
        info[0] = plan.fused() ? 1 : 0;
        info[2] = plan.fused() ? 1 << plan.core.passes[0].log2C : 0;
    }
    const long long before = rt.launches;
    if (plan.execute((const T*)in, in_pitch, (T*)out, out_pitch) != 0) return -2;
    if (info) info[1] = (int)(rt.launches - before);
    return 0;
}

extern "C" int emu_dct(const void* in, long long in_pitch, void* out, long long out_pitch, int n, int batch, int type, int norm, int prec, int flags,
                       int* info) {
    return prec == 1 ? run_dct<float>(in, in_pitch, out, out_pitch, n, batch, type, norm, flags, info)
                     : run_dct<double>(in, in_pitch, out, out_pitch, n, batch, type, norm, flags, info);
}

// What fft_gpu_plan_dct_2d_hip builds: pitches in reals between matrices.  info: [0] fused, [1] launches
template <typename T>
static int run_dct2d(const void* in, long long in_pitch, void* out, long long out_pitch, int rows, int cols, int nm, int type, int norm, int flags,
                     int* info) {
    emu::Runtime rt;
    ffteng::Dct2DPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, rows, cols, nm, type, norm)) return -1;
    plan.set_no_fusion((flags & 1) != 0);
    if (info) info[0] = plan.fused() ? 1 : 0;
    const long long before = rt.launches;
    if (plan.execute((const T*)in, in_pitch, (T*)out, out_pitch) != 0) return -2;
    if (info) info[1] = (int)(rt.launches - before);
    return 0;
}

extern "C" int emu_dct2d(const void* in, long long in_pitch, void* out, long long out_pitch, int rows, int cols, int nm, int type, int norm, int prec,
                         int flags, int* info) {
    return prec == 1 ? run_dct2d<float>(in, in_pitch, out, out_pitch, rows, cols, nm, type, norm, flags, info)
                     : run_dct2d<double>(in, in_pitch, out, out_pitch, rows, cols, nm, type, norm, flags, info);
}
