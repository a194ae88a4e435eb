// emu_real2d.cpp -- the real 2D transform plan (fft_plans_ext.h Real2DPlan; fft_kernels_real2d.h) under the CPU emulation, as a library
// of its own.  TEST INFRASTRUCTURE ONLY.  The emulation's runtime is emu_fft.cpp's.
#include "emu_fft.cpp"

// What fft_gpu_plan_r2c_2d_hip / fft_gpu_plan_c2r_2d_hip build and fft_gpu_execute_real2d_hip runs: one execute of `in` into `out`
// (forward: reals -> one-sided spectra; inverse: the way back).  lds_budget > 0 narrows the column tile; min_seg > 0 replaces the fused
// path's 64-byte row-segment criterion, so that tiles of C = V and C = 2 V columns run the column pass.  flags: bit 0 no_fusion.
// Returns 0, -1 the plan was refused, -2 the execute was refused (nothing was launched).
// info: [0] fused (1 / 0), [1] passes (2 fused; the fallback's steps), [2] bins = cols/2 + 1, [3] columns per tile of the column pass
//       (0: none), [4] column tiles per matrix, [5] kernel launches of the execute, [6] elements between the rows of the work image
template <typename T>
static int run_real2d(const void* in, long long in_pitch, void* out, long long out_pitch, int rows, int cols, int n_matrices, int forward, int lds_budget,
                      int flags, int min_seg, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::Real2DPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, rows, cols, n_matrices, forward != 0, min_seg > 0 ? min_seg : 64)) return -1;
    plan.no_fusion = (flags & 1) != 0;
    if (info) {
        info[0] = plan.fused() ? 1 : 0;
        info[1] = plan.passes();
        info[2] = plan.hb;
        info[3] = plan.fused() ? plan.cstep.tile_cols() : 0;
        info[4] = plan.fused() ? plan.cstep.n_ct : 0;
        info[6] = (int)plan.ld;
    }
    const long long before = rt.launches;
    if (plan.execute(in, in_pitch, out, out_pitch) != 0) return -2;
    if (info) info[5] = (int)(rt.launches - before);
    return 0;
}

extern "C" int emu_real2d(const void* in, long long in_pitch, void* out, long long out_pitch, int rows, int cols, int n_matrices, int forward, int prec,
                          int lds_budget, int flags, int min_seg, int* info) {
    return prec == 1 ? run_real2d<float>(in, in_pitch, out, out_pitch, rows, cols, n_matrices, forward, lds_budget, flags, min_seg, info)
                     : run_real2d<double>(in, in_pitch, out, out_pitch, rows, cols, n_matrices, forward, lds_budget, flags, min_seg, info);
}

// The column pass alone (ffteng::ColPassStep): in [nm][P][in_ld] -> out [nm][P][out_ld], n_cols live columns, value-by-value accesses
// unless vec bit 0 (input side) / bit 1 (output side) asks for 16-byte ones.  out = scale * (forward or inverse) column transforms.
// Returns 0 / -1 (no one-pass column tile).  info: [0] columns per tile, [1] tiles per matrix
template <typename T>
static int run_colpass(const void* in, long long in_ld, void* out, long long out_ld, int log2P, int n_cols, int nm, int inverse, double scale, int vec,
                       int lds_budget, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::ColPassStep<T, emu::Runtime> step;
    if (!step.build(&rt, log2P, n_cols, nm, 0)) return -1;
    if (info) {
        info[0] = step.tile_cols();
        info[1] = step.n_ct;
    }
    step.run((const fftk::cpx<T>*)in, in_ld, in_ld << log2P, (vec & 1) != 0, (fftk::cpx<T>*)out, out_ld, out_ld << log2P, (vec & 2) != 0, nm, inverse != 0,
             (T)scale);
    return 0;
}

extern "C" int emu_colpass(const void* in, long long in_ld, void* out, long long out_ld, int log2P, int n_cols, int nm, int inverse, double scale, int vec,
                           int prec, int lds_budget, int* info) {
    return prec == 1 ? run_colpass<float>(in, in_ld, out, out_ld, log2P, n_cols, nm, inverse, scale, vec, lds_budget, info)
                     : run_colpass<double>(in, in_ld, out, out_ld, log2P, n_cols, nm, inverse, scale, vec, lds_budget, info);
}
