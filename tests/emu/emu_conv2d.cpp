// emu_conv2d.cpp -- the 2D convolution / spectrum-filtering plan (fft_plans_ext.h Conv2DPlan; fft_kernels_conv2d.h) under the CPU
// emulation, as a library of its own.  TEST INFRASTRUCTURE ONLY.  The emulation's runtime is emu_fft.cpp's.
#include "emu_fft.cpp"

// What fft_gpu_plan_conv2d_hip builds and fft_gpu_execute_conv2d_hip runs: one execute of x into y, then -- if y2 is given -- a second
// of the same plan, of x2 (x where x2 is NULL) into y2.  lds_budget > 0 narrows the column tile; min_seg > 0 replaces the fused path's
// 64-byte row-segment criterion, so that tiles of C = V and C = 2 V columns run the column round.  flags: bit 0 no_fusion.
// Returns 0, -1 the plan was refused, -2 the execute was refused (nothing was launched).
// info: [0] fused (1 / 0), [1] HBM round trips (3 / 5), [2] P, [3] Q, [4] out_rows, [5] out_cols, [6] columns per tile of the column
//       round (0: none), [7] kernel launches of ONE execute
template <typename T>
static int run_conv2d(const void* x, void* y, const void* x2, void* y2, int rows, int cols, int krows, int kcols, const void* k, int n_matrices, int mode,
                      long long x_pitch, long long y_pitch, int lds_budget, int flags, int min_seg, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::Conv2DPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, rows, cols, krows, kcols, (const fftk::cpx<T>*)k, n_matrices, mode, min_seg > 0 ? min_seg : 64)) return -1;
    plan.no_fusion = (flags & 1) != 0;
    if (info) {
        info[0] = plan.fused() ? 1 : 0;
        info[1] = plan.passes();
        info[2] = plan.P;
        info[3] = plan.Q;
        info[4] = plan.out_rows;
        info[5] = plan.out_cols;
        info[6] = plan.round.tile_cols();
    }
    const long long before = rt.launches;
    if (plan.execute((const fftk::cpx<T>*)x, x_pitch, (fftk::cpx<T>*)y, y_pitch) != 0) return -2;
    if (info) info[7] = (int)(rt.launches - before);
    if (y2 && plan.execute((const fftk::cpx<T>*)(x2 ? x2 : x), x_pitch, (fftk::cpx<T>*)y2, y_pitch) != 0) return -2;
    return 0;
}

extern "C" int emu_conv2d(const void* x, void* y, const void* x2, void* y2, int rows, int cols, int krows, int kcols, const void* k, int n_matrices,
                          int mode, long long x_pitch, long long y_pitch, int prec, int lds_budget, int flags, int min_seg, int* info) {
    return prec == 1 ? run_conv2d<float>(x, y, x2, y2, rows, cols, krows, kcols, k, n_matrices, mode, x_pitch, y_pitch, lds_budget, flags, min_seg, info)
                     : run_conv2d<double>(x, y, x2, y2, rows, cols, krows, kcols, k, n_matrices, mode, x_pitch, y_pitch, lds_budget, flags, min_seg, info);
}

// The column round alone (ffteng::ColRoundStep), for row lengths the plan never makes: Q any multiple of the 16-byte lane access, so
// that the last tile of a row is partial.  in: [nm][rows_in][Q], H: [P][Q], out: [nm][rows_out][Q].
// Returns 0 / -1 (no one-pass column tile).  info: [0] columns per tile, [1] tiles per matrix
template <typename T>
static int run_colround(const void* in, const void* H, void* out, int log2P, int Q, int rows_in, int rows_out, int nm, int lds_budget, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::ColRoundStep<T, emu::Runtime> step;
    if (!step.build(&rt, log2P, Q, nm, 0)) return -1;
    if (info) {
        info[0] = step.tile_cols();
        info[1] = step.colp.passes[0].n_ct;
    }
    step.run((const fftk::cpx<T>*)in, rows_in, (const fftk::cpx<T>*)H, (fftk::cpx<T>*)out, rows_out, nm);
    return 0;
}

extern "C" int emu_colround(const void* in, const void* H, void* out, int log2P, int Q, int rows_in, int rows_out, int nm, int prec, int lds_budget,
                            int* info) {
    return prec == 1 ? run_colround<float>(in, H, out, log2P, Q, rows_in, rows_out, nm, lds_budget, info)
                     : run_colround<double>(in, H, out, log2P, Q, rows_in, rows_out, nm, lds_budget, info);
}
