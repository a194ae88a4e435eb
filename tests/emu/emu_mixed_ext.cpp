// emu_mixed_ext.cpp -- the 2D and real plans (fft_plans_ext.h) with their 7-smooth lengths on the mixed-radix engine, under the
// CPU emulation, as a library of its own.  TEST INFRASTRUCTURE ONLY.  The emulation's runtime is emu_fft.cpp's.
#include "emu_fft.cpp"

// which engine a batched 1D transform inside a plan runs on: 1 mixed radix / 2 power of two / 3 chirp-z (0: there is none)
template <class Any>
static int kind_of(const Any* a) {
    return !a ? 0 : a->mr ? 1 : a->p2 ? 2 : a->bl ? 3 : 0;
}

// What fft_gpu_plan_2d_algo_hip builds: smooth = 1 is FFT_GPU_ALGO_MIXED_RADIX (or AUTO under the smooth policy), 0 plain AUTO.
// info: [0] columns: 0 none (one row) / 1 direct power-of-two pass / 2 transposed image / 3 two strided passes
//       [1] engine of the rows, [2] engine of the transposed-image columns (kind_of), [3] passes of a mixed-radix transposed-image
//       core, [4] its rows per tile, [5] passes of mixed-radix rows
template <typename T>
static int run2d_mixed(const void* in, void* out, int rows, int cols, int nm, int dir, int lds_budget, int smooth, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::Plan2D<T, emu::Runtime> plan;
    if (!plan.build(&rt, rows, cols, dir, nm, smooth != 0)) return -1;
    if (info) {
        info[0] = plan.colp ? (plan.colp->passes.size() == 2 ? 3 : 1) : plan.colt ? 2 : 0;
        info[1] = kind_of(&plan.rowp);
        info[2] = kind_of(plan.colt);
        info[3] = plan.colt && plan.colt->mr ? (int)plan.colt->mr->passes.size() : 0;
        info[4] = plan.colt && plan.colt->mr ? plan.colt->mr->passes[0].p.C : 0;
        info[5] = plan.rowp.mr ? (int)plan.rowp.mr->passes.size() : 0;
    }
    plan.execute((const fftk::cpx<T>*)in, (fftk::cpx<T>*)out, nm);
    return 0;
}
extern "C" int emu_mixed_fft2d(const void* in, void* out, int rows, int cols, int nm, int dir, int prec, int lds_budget, int smooth, int* info) {
    return prec == 1 ? run2d_mixed<float>(in, out, rows, cols, nm, dir, lds_budget, smooth, info)
                     : run2d_mixed<double>(in, out, rows, cols, nm, dir, lds_budget, smooth, info);
}

// What fft_gpu_plan_r2c_1d_algo_hip / fft_gpu_plan_c2r_1d_algo_hip build.
// info: [0] engine of the complex core (kind_of), [1] passes, [2] factor 0, [3] factor 1, [4] launch-group size, [5] rows per
//       tile of the first pass (mixed-radix cores; 0 otherwise)
template <typename T>
static int run_real_mixed(const void* in, void* out, int n, int batch, int r2c, int lds_budget, int smooth, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::RealPlan<T, emu::Runtime> plan;
    if (!plan.build(&rt, n, r2c != 0, batch, smooth != 0)) return -1;
    if (info) {
        info[0] = kind_of(&plan.core);
        if (plan.core.mr) {
            info[1] = (int)plan.core.mr->passes.size();
            info[2] = plan.core.mr->n1;
            info[3] = plan.core.mr->n2;
            info[4] = plan.core.mr->chunk;
            info[5] = plan.core.mr->passes[0].p.C;
        }
    }
    if (r2c) plan.execute_r2c((const T*)in, (fftk::cpx<T>*)out, batch);
    else plan.execute_c2r((const fftk::cpx<T>*)in, (T*)out, batch);
    return 0;
}
extern "C" int emu_mixed_real(const void* in, void* out, int n, int batch, int r2c, int prec, int lds_budget, int smooth, int* info) {
    return prec == 1 ? run_real_mixed<float>(in, out, n, batch, r2c, lds_budget, smooth, info)
                     : run_real_mixed<double>(in, out, n, batch, r2c, lds_budget, smooth, info);
}
