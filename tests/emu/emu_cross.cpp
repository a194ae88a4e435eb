// emu_cross.cpp -- the cross frames plan (fft_plans_ext.h CrossFramesPlan: cross-spectral density, coherence and transfer estimate
// of signal pairs; frames_cross_partial_kernel, frames_cross_finish_kernel) under the CPU emulation, as a library of its own.
// TEST INFRASTRUCTURE ONLY.  emu_rframes.cpp comes along: its runtime, and emu_rframes / emu_frames -- the Welch plans whose rows
// the cross plan's Pxx is compared with.
#include "emu_rframes.cpp"

// What fft_gpu_plan_cross_frames[_real]_hip builds and fft_gpu_execute_cross_frames_hip runs: one execute into out, a second of the
// same plan into out2 if it is given.  Pitches in elements (reals for real_input).  lds_budget > 0 forces multi-pass cores at small n;
// max_grid / block > 0 replace the launch geometry of the two reduction kernels.
// Returns 0, -1 the plan was refused, -2 the execute was refused (nothing was launched).
// info: [0] passes of the inner core, [1] 1 the inner plan's one-launch path / 0 its fallback, [2] frames per signal,
//       [3] kernel launches of ONE execute, [4] C (frames per chunk), [5] chunks, [6] bytes of the partial-sum workspace,
//       [7] bytes of ONE row workspace
template <typename T>
static int run_cross(const void* x, long long x_pitch, const void* y, long long y_pitch, void* out, void* out2, int n, int hop, int signal_len,
                     int n_signals, int window, const void* w_host, int out_kind, int real_input, int lds_budget, int no_fusion, int max_grid, int block,
                     double fs, long long* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::CrossFramesPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, n, hop, signal_len, n_signals, window, (const T*)w_host, out_kind, real_input != 0)) return -1;
    plan.inner.no_fusion = no_fusion != 0;
    if (max_grid > 0) plan.max_grid = max_grid;
    if (block > 0) plan.block = block;
    if (info) {
        info[0] = (long long)plan.inner.core.passes.size();
        info[1] = plan.inner.fused() ? 1 : 0;
        info[2] = plan.inner.nw;
        info[4] = plan.C;
        info[5] = plan.chunks;
        info[6] = (long long)plan.part_bytes();
        info[7] = (long long)plan.rows_bytes();
    }
    const long long before = rt.launches;
    if (plan.execute(x, x_pitch, y, y_pitch, out, fs) != 0) return -2;
    if (info) info[3] = rt.launches - before;
    if (out2 && plan.execute(x, x_pitch, y, y_pitch, out2, fs) != 0) return -2;
    return 0;
}

extern "C" int emu_cross(const void* x, long long x_pitch, const void* y, long long y_pitch, void* out, void* out2, int n, int hop, int signal_len,
                         int n_signals, int window, const void* w_host, int out_kind, int real_input, int prec, int lds_budget, int no_fusion,
                         int max_grid, int block, double fs, long long* info) {
    return prec == 1 ? run_cross<float>(x, x_pitch, y, y_pitch, out, out2, n, hop, signal_len, n_signals, window, w_host, out_kind, real_input, lds_budget,
                                        no_fusion, max_grid, block, fs, info)
                     : run_cross<double>(x, x_pitch, y, y_pitch, out, out2, n, hop, signal_len, n_signals, window, w_host, out_kind, real_input, lds_budget,
                                         no_fusion, max_grid, block, fs, info);
}

// the plan-time chunk rule on its own (no plan is built): C for nw frames per signal, n_signals pairs, hb bins
extern "C" int emu_cross_chunk_len(int nw, int n_signals, int hb) { return ffteng::CrossFramesPlan<float, emu::Runtime>::chunk_len(nw, n_signals, hb); }
