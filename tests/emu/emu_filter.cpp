// emu_filter.cpp -- the overlap-save FIR filter plan (fft_plans_ext.h FilterPlan) under the CPU emulation, as a library of its own.
// TEST INFRASTRUCTURE ONLY.  The emulation's runtime is emu_fft.cpp's.
#include "emu_fft.cpp"

// What fft_gpu_plan_filter_hip builds and fft_gpu_execute_filter_hip runs: one execute of x into y, then -- if y2 is given -- a second
// of the same plan, of x2 (x where x2 is NULL) into y2.  lds_budget > 0 forces multi-pass cores at small n.
// flags: bit 0 no_fusion, bit 1 no_chain.
// Returns 0, -1 the plan was refused, -2 the execute was refused (nothing was launched).
// info: [0] passes of the core, [1] the path (3 one launch; fallback: 2 / 1 / 0 by what the middle runs), [2] blocks per signal,
//       [3] kernel launches of ONE execute, [4] blocks per tile of the first pass, [5] the block length n, [6] out_len
template <typename T>
static int run_filter(const void* x, void* y, const void* x2, void* y2, int n_taps, const void* h, int signal_len, int n_signals, int n, int out_kind,
                      long long x_pitch, long long y_pitch, int lds_budget, int flags, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::FilterPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, n_taps, (const fftk::cpx<T>*)h, signal_len, n_signals, n, out_kind)) return -1;
    plan.no_fusion = (flags & 1) != 0;
    plan.no_chain = (flags & 2) != 0;
    if (info) {
        info[0] = (int)plan.core.passes.size();
        info[1] = plan.path();
        info[2] = plan.nb;
        info[4] = plan.core.passes.empty() ? 0 : 1 << plan.core.passes[0].log2C;
        info[5] = plan.n;
        info[6] = plan.out_len;
    }
    const long long before = rt.launches;
    if (plan.execute((const fftk::cpx<T>*)x, x_pitch, (fftk::cpx<T>*)y, y_pitch) != 0) return -2;
    if (info) info[3] = (int)(rt.launches - before);
    if (y2 && plan.execute((const fftk::cpx<T>*)(x2 ? x2 : x), x_pitch, (fftk::cpx<T>*)y2, y_pitch) != 0) return -2;
    return 0;
}

extern "C" int emu_filter(const void* x, void* y, const void* x2, void* y2, int n_taps, const void* h, int signal_len, int n_signals, int n, int out_kind,
                          long long x_pitch, long long y_pitch, int prec, int lds_budget, int flags, int* info) {
    return prec == 1 ? run_filter<float>(x, y, x2, y2, n_taps, h, signal_len, n_signals, n, out_kind, x_pitch, y_pitch, lds_budget, flags, info)
                     : run_filter<double>(x, y, x2, y2, n_taps, h, signal_len, n_signals, n, out_kind, x_pitch, y_pitch, lds_budget, flags, info);
}
