// emu_frames.cpp -- the STFT / spectrogram / Welch plan on overlapping frames (fft_plans_ext.h FramesPlan) under the CPU
// emulation, as a library of its own.  TEST INFRASTRUCTURE ONLY.  The emulation's runtime is emu_fft.cpp's, and so is emu_fused,
// whose periodogram plan the Welch plan is compared with (ladder case i).
#include "emu_fft.cpp"

// What fft_gpu_plan_frames_hip builds and fft_gpu_execute_frames_hip runs: one execute into out, a second of the same plan into
// out2 if it is given.  lds_budget > 0 forces multi-pass cores at small n.
// Returns 0, -1 the plan was refused, -2 the execute was refused (nothing was launched).
// info: [0] passes of the core, [1] 1 the framed load and the stores ride on the pass / 0 the fallback, [2] frames per signal,
//       [3] kernel launches of ONE execute, [4] frames per tile of the first pass
template <typename T>
static int run_frames(const void* x, void* out, void* out2, int n, int hop, int signal_len, int n_signals, long long signal_pitch, int window,
                      const void* w_host, int out_kind, int lds_budget, int no_fusion, double fs, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::FramesPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, n, hop, signal_len, n_signals, window, (const T*)w_host, out_kind)) return -1;
    plan.no_fusion = no_fusion != 0;
    if (info) {
        info[0] = (int)plan.core.passes.size();
        info[1] = plan.fused() ? 1 : 0;
        info[2] = plan.nw;
        info[4] = plan.core.passes.empty() ? 0 : 1 << plan.core.passes[0].log2C;
    }
    const long long before = rt.launches;
    if (plan.execute((const fftk::cpx<T>*)x, signal_pitch, out, fs) != 0) return -2;
    if (info) info[3] = (int)(rt.launches - before);
    if (out2 && plan.execute((const fftk::cpx<T>*)x, signal_pitch, out2, fs) != 0) return -2;
    return 0;
}

extern "C" int emu_frames(const void* x, void* out, void* out2, int n, int hop, int signal_len, int n_signals, long long signal_pitch, int window,
                          const void* w_host, int out_kind, int prec, int lds_budget, int no_fusion, double fs, int* info) {
    return prec == 1 ? run_frames<float>(x, out, out2, n, hop, signal_len, n_signals, signal_pitch, window, w_host, out_kind, lds_budget, no_fusion, fs, info)
                     : run_frames<double>(x, out, out2, n, hop, signal_len, n_signals, signal_pitch, window, w_host, out_kind, lds_budget, no_fusion, fs, info);
}
