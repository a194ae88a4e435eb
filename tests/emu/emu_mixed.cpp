// emu_mixed.cpp -- the mixed-radix plan (fft_mixed_radix.h, ffteng::MixedRadixPlan) under the CPU emulation, as a
// library of its own.  TEST INFRASTRUCTURE ONLY.  The emulation's runtime (workgroups as host threads) is emu_fft.cpp's.
#include "emu_fft.cpp"

// What fft_gpu_plan_1d_ex_hip does with FFT_GPU_ALGO_MIXED_RADIX: the mixed-radix plan for a 7-smooth n that is no power of
// two, the plan AUTO builds for a power of two, chirp-z for any other n.
// info: [0] 1 mixed radix / 2 power of two / 3 chirp-z, [1] passes, [2] factor 0, [3] factor 1, [4] launch-group size,
//       [5] sub-transforms per tile of the first pass
template <typename T>
static int run_mixed(const void* in, void* out, int n, int batch, int dir, int lds_budget, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    using C = fftk::cpx<T>;
    if (n >= 1 && (n & (n - 1)) != 0 && ffteng::mr_passes(n) > 0) {
        ffteng::MixedRadixPlan<T, emu::Runtime> plan;
        if (plan.build(&rt, n, batch)) {
            if (info) {
                info[0] = 1;
                info[1] = (int)plan.passes.size();
                info[2] = plan.n1;
                info[3] = plan.n2;
                info[4] = plan.chunk;
                info[5] = plan.passes[0].p.C;
            }
            plan.execute((const C*)in, (C*)out, batch, dir > 0);
            return 0;
        }
    }
    int sub[8] = {0};
    const int rc = run<T>(in, out, n, batch, dir, 0, lds_budget, sub);
    if (info) {
        info[0] = (n & (n - 1)) == 0 ? 2 : 3;
        info[1] = sub[0];
    }
    return rc;
}

extern "C" int emu_mixed(const void* in, void* out, int n, int batch, int dir, int prec, int lds_budget, int* info) {
    return prec == 1 ? run_mixed<float>(in, out, n, batch, dir, lds_budget, info) : run_mixed<double>(in, out, n, batch, dir, lds_budget, info);
}

extern "C" int emu_mixed_passes(int n) { return ffteng::mr_passes(n); }
