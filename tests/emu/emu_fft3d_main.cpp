// emu_fft3d_main.cpp -- the 3D transform plan (fft_plans_ext.h Plan3D, fft_kernels_plane.h) under the CPU emulation as a stand-alone
// program for the sanitizers: both paths and both directions on exactly sized heap buffers, against a direct float64 DFT.
// TEST INFRASTRUCTURE ONLY.  Build: g++ -std=c++17 -DFFT_EMU -DFFT_EXPERIMENTS -fsanitize=address,undefined -pthread -I<csrc> ...
#include "emu_fft3d.cpp"

#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

typedef std::complex<double> cd;

// the separable DFT, axis by axis, O(n (d + r + c))
static void dft_axis(std::vector<cd>& a, int outer, int n, int inner, int sign) {
    std::vector<cd> t((size_t)n);
    const double two_pi = 6.283185307179586476925286766559;
    for (int o = 0; o < outer; o++)
        for (int i = 0; i < inner; i++) {
            for (int k = 0; k < n; k++) {
                cd s = 0;
                for (int l = 0; l < n; l++) s += a[((size_t)o * n + l) * inner + i] * std::polar(1.0, sign * two_pi * (double)((long long)k * l % n) / n);
                t[(size_t)k] = s;
            }
            for (int k = 0; k < n; k++) a[((size_t)o * n + k) * inner + i] = t[(size_t)k];
        }
}

template <typename T>
static int one(int depth, int rows, int cols, int nv, int inverse, int lds_budget, int flags, int want_fused, bool in_place) {
    const size_t n = (size_t)depth * rows * cols, total = n * nv;
    std::vector<std::complex<T>>* in = new std::vector<std::complex<T>>(total);   // exactly sized: one value past either end is a report
    std::vector<std::complex<T>>* out = in_place ? in : new std::vector<std::complex<T>>(total);
    std::vector<cd> ref(total);
    unsigned s = 12345u + (unsigned)(depth * 131 + rows * 17 + cols);
    for (size_t i = 0; i < total; i++) {
        s = s * 1664525u + 1013904223u;
        const double re = (double)(s >> 8) / (1 << 24) - 0.5;
        s = s * 1664525u + 1013904223u;
        const double im = (double)(s >> 8) / (1 << 24) - 0.5;
        (*in)[i] = std::complex<T>((T)re, (T)im);
        ref[i] = cd((double)(T)re, (double)(T)im);
    }
    const int sign = inverse ? 1 : -1;
    dft_axis(ref, nv * depth * rows, cols, 1, sign);
    dft_axis(ref, nv * depth, rows, cols, sign);
    dft_axis(ref, nv, depth, rows * cols, sign);
    int info[12] = {0};
    const int rc = emu_fft3d(in->data(), out->data(), depth, rows, cols, nv, inverse, sizeof(T) == 4 ? 1 : 0, lds_budget, flags, info);
    double worst = 0, rms = 0;
    for (size_t i = 0; i < total; i++) {
        const cd r = inverse ? ref[i] / (double)n : ref[i];
        worst = std::max(worst, std::abs(cd((*out)[i].real(), (*out)[i].imag()) - r));
        rms += std::norm(r);
    }
    rms = std::sqrt(rms / total);
    const double u = sizeof(T) == 4 ? std::ldexp(1.0, -24) : std::ldexp(1.0, -53);
    const double e = worst / rms / (u * std::max(1.0, std::log2((double)n)));
    printf("%dx%dx%d x%d %s %s lds %d flags %d%s: rc %d fused %d launches %d strips %d/%d prefetch %d, %.3f u log2 n\n", depth, rows, cols, nv,
           sizeof(T) == 4 ? "fp32" : "fp64", inverse ? "inverse" : "forward", lds_budget, flags, in_place ? " in place" : "", rc, info[0], info[2], info[6],
           info[7], info[5], e);
    if (out != in) delete out;
    delete in;
    return (rc == 0 && info[0] == want_fused && e <= 8.0) ? 0 : 1;
}

int main() {
    int bad = 0;
    for (int inverse = 0; inverse < 2; inverse++) {
        bad += one<float>(2, 8, 8, 3, inverse, 0, 0, 1, false);
        bad += one<double>(4, 16, 8, 3, inverse, 0, 0, 1, true);
        bad += one<float>(3, 16, 16, 2, inverse, 0, 0, 1, true);            // the transpose route along depth
        bad += one<double>(2, 64, 64, 1, inverse, 0, 0, 1, false);          // two strips per step
        bad += one<float>(2, 32, 32, 3, inverse, 20 * 1024, 2, 1, true);    // a small budget: many strips, no prefetch
        bad += one<float>(2, 32, 32, 1, inverse, 8 * 1024, 0, 0, false);    // ... and one that leaves the composition
        bad += one<double>(5, 6, 7, 2, inverse, 0, 0, 0, false);            // the composition, no power of two anywhere
        bad += one<float>(4, 16, 16, 2, inverse, 0, 1, 0, true);            // no_fusion
        bad += one<float>(1, 1, 1, 1, inverse, 0, 0, 0, false);
    }
    if (bad) {
        printf("%d cases FAILED\n", bad);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
