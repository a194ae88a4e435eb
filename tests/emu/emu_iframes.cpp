// emu_iframes.cpp -- the inverse STFT plan (fft_plans_ext.h IFramesPlan: one-sided rows back to real signals by overlap-add) under
// the CPU emulation, as a library of its own.  TEST INFRASTRUCTURE ONLY.  emu_rframes.cpp comes along: its runtime, and emu_rframes --
// the real frames plan whose STFT rows the round trip feeds back.
#include "emu_rframes.cpp"

// What fft_gpu_plan_iframes_real_hip builds and fft_gpu_execute_iframes_hip runs: one execute into y, a second of the same plan
// into y2 if it is given.  X: [signals][frames][n/2 + 1] complex; signal_pitch in reals (0: out_len).  lds_budget > 0 forces
// multi-pass cores at small n.  Returns 0, -1 the plan was refused, -2 the execute was refused (nothing was launched).
// info: [0] passes of the (half-length) core, [1] 1 the one-launch transform path / 0 the fallback, [2] out_len,
//       [3] kernel launches of ONE execute, [4] frames per tile of the first pass, [5] unrecoverable samples per signal
template <typename T>
static int run_iframes(const void* X, void* y, void* y2, int n, int hop, int n_frames, int n_signals, long long signal_pitch, int window,
                       const void* w_host, int lds_budget, int no_fusion, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::IFramesPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, n, hop, n_frames, n_signals, window, (const T*)w_host)) return -1;
    plan.no_fusion = no_fusion != 0;
    if (info) {
        info[0] = (int)plan.core.passes.size();
        info[1] = plan.fused() ? 1 : 0;
        info[2] = (int)plan.out_len();
        info[4] = plan.core.passes.empty() ? 0 : 1 << plan.core.passes[0].log2C;
        info[5] = plan.unrecoverable;
    }
    const long long before = rt.launches;
    if (plan.execute((const fftk::cpx<T>*)X, (T*)y, signal_pitch) != 0) return -2;
    if (info) info[3] = (int)(rt.launches - before);
    if (y2 && plan.execute((const fftk::cpx<T>*)X, (T*)y2, signal_pitch) != 0) return -2;
    return 0;
}

extern "C" int emu_iframes(const void* X, void* y, void* y2, int n, int hop, int n_frames, int n_signals, long long signal_pitch, int window,
                           const void* w_host, int prec, int lds_budget, int no_fusion, int* info) {
    return prec == 1 ? run_iframes<float>(X, y, y2, n, hop, n_frames, n_signals, signal_pitch, window, w_host, lds_budget, no_fusion, info)
                     : run_iframes<double>(X, y, y2, n, hop, n_frames, n_signals, signal_pitch, window, w_host, lds_budget, no_fusion, info);
}
