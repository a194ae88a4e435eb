// emu_fft3d.cpp -- the 3D complex transform plan (fft_plans_ext.h Plan3D; fft_kernels_plane.h) under the CPU emulation, as a library of
// its own.  TEST INFRASTRUCTURE ONLY.  The emulation's runtime is emu_fft.cpp's.
#include "emu_fft.cpp"

// What fft_gpu_plan_3d_hip builds and fft_gpu_execute_ptr_hip runs: one execute of `in` into `out` (in == out: in place).  lds_budget > 0
// narrows the LDS the plan may use, so that small planes take the many-strip layout or the composition.  flags: bit 0 no_fusion, bit 1 take_unprefetched (tiles of more than two strips per step, which the
// device plan leaves to the composition).
// Returns 0, -1 the plan was refused, -2 the execute was.
// info: [0] fused (1 / 0), [1] launches the plan reports, [2] kernel launches of the execute, [3] planes per tile, [4] threads, [5] chunks
//       per thread the plane kernel prefetches (0: none), [6] row-step strips, [7] column-step strips, [8] depth route (0 none, 1 one
//       column pass, 2 two, 3 transposes), [9] device allocations of the refused or built plan's workspace in bytes
template <typename T>
static int run_fft3d(const void* in, void* out, int depth, int rows, int cols, int n_volumes, int inverse, int lds_budget, int flags, int* info) {
    emu::Runtime rt;
    if (lds_budget > 0) rt.lds_budget = lds_budget;
    ffteng::Plan3D<T, emu::Runtime> plan;
    plan.take_unprefetched = (flags & 2) != 0;
    if (!plan.build(&rt, depth, rows, cols, inverse ? 1 : -1, n_volumes)) return -1;
    plan.set_no_fusion((flags & 1) != 0);
    const long long before = rt.launches;
    if (plan.execute((const fftk::cpx<T>*)in, (fftk::cpx<T>*)out) != 0) return -2;
    if (info) {
        info[0] = plan.fused() ? 1 : 0;
        info[1] = plan.launches();
        info[2] = (int)(rt.launches - before);
        info[3] = plan.tile_planes();
        info[4] = plan.plane_ok ? plan.pk_threads : 0;
        info[5] = plan.plane_ok ? plan.pk_npf : 0;
        info[6] = plan.plane_ok ? 1 << (plan.pk.log2G + plan.pk.log2P - plan.pk.log2SR) : 0;
        info[7] = plan.plane_ok ? 1 << (plan.pk.log2G + plan.pk.log2Q - plan.pk.log2SC) : 0;
        info[8] = plan.dcol ? (int)plan.dcol->passes.size() : plan.dany ? 3 : 0;
        info[9] = (int)plan.workspace_bytes();
    }
    return 0;
}

extern "C" int emu_fft3d(const void* in, void* out, int depth, int rows, int cols, int n_volumes, int inverse, int prec, int lds_budget, int flags,
                         int* info) {
    return prec == 1 ? run_fft3d<float>(in, out, depth, rows, cols, n_volumes, inverse, lds_budget, flags, info)
                     : run_fft3d<double>(in, out, depth, rows, cols, n_volumes, inverse, lds_budget, flags, info);
}
