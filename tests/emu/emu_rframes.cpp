// emu_rframes.cpp -- the STFT / spectrogram / Welch plan on overlapping frames of REAL signals (fft_plans_ext.h FramesPlan with
// real_input) under the CPU emulation, as a library of its own.  TEST INFRASTRUCTURE ONLY.  emu_frames.cpp comes along: its runtime,
// and emu_frames -- the complex frames plan the real plan's rows are compared with.
#include "emu_frames.cpp"

namespace {

// the emulation's runtime, which also notes what the launcher decided for a framed launch: TileHooks::in_vec_ok
struct SpyRuntime : emu::Runtime {
    int frames_in_vec_ok = -1;  // of the last launch with a framed load; -1: there was none
    template <class T>
    void spy(const fftk::TileParams<T>& tp) {
        if (tp.hk.frames_per_signal > 0) frames_in_vec_ok = tp.hk.in_vec_ok;
    }
    template <class... A>
    void spy(const A&...) {}
    template <class K, class... A>
    void launch(K kernel, long long grid, int block, size_t smem, A... args) {
        spy(args...);
        emu::Runtime::launch(kernel, grid, block, smem, args...);
    }
};

}  // namespace

// What fft_gpu_plan_frames_real_hip builds and fft_gpu_execute_frames_hip runs: one execute into out, a second of the same plan
// into out2 if it is given.  x: real samples, signal_pitch in reals.  lds_budget > 0 forces multi-pass cores at small n.
// Returns 0, -1 the plan was refused, -2 the execute was refused (nothing was launched).
// info: [0] passes of the (half-length) core, [1] 1 the one-launch path / 0 the fallback, [2] frames per signal,
//       [3] kernel launches of ONE execute, [4] frames per tile of the first pass, [5] in_vec_ok of the framed launch (-1: none)
template <typename T>
static int run_rframes(const void* x, void* out, void* out2, int n, int hop, int signal_len, int n_signals, long long signal_pitch, int window,
                       const void* w_host, int out_kind, int lds_budget, int no_fusion, double fs, int* info) {
    SpyRuntime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::FramesPlan<T, SpyRuntime> plan;
    if (!plan.build(&rt, n, hop, signal_len, n_signals, window, (const T*)w_host, out_kind, true)) return -1;
    plan.no_fusion = no_fusion != 0;
    if (info) {
        info[0] = (int)plan.core.passes.size();
        info[1] = plan.fused() ? 1 : 0;
        info[2] = plan.nw;
        info[4] = plan.core.passes.empty() ? 0 : 1 << plan.core.passes[0].log2C;
    }
    const long long before = rt.launches;
    if (plan.execute((const fftk::cpx<T>*)x, signal_pitch, out, fs) != 0) return -2;
    if (info) {
        info[3] = (int)(rt.launches - before);
        info[5] = rt.frames_in_vec_ok;
    }
    if (out2 && plan.execute((const fftk::cpx<T>*)x, signal_pitch, out2, fs) != 0) return -2;
    return 0;
}

extern "C" int emu_rframes(const void* x, void* out, void* out2, int n, int hop, int signal_len, int n_signals, long long signal_pitch, int window,
                           const void* w_host, int out_kind, int prec, int lds_budget, int no_fusion, double fs, int* info) {
    return prec == 1 ? run_rframes<float>(x, out, out2, n, hop, signal_len, n_signals, signal_pitch, window, w_host, out_kind, lds_budget, no_fusion, fs, info)
                     : run_rframes<double>(x, out, out2, n, hop, signal_len, n_signals, signal_pitch, window, w_host, out_kind, lds_budget, no_fusion, fs, info);
}
