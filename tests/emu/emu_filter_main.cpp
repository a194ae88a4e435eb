// emu_filter_main.cpp -- the emulated overlap-save filter plan on EXACTLY sized heap buffers, as a stand-alone program meant to be built
// with -fsanitize=address,undefined: one signal of signal_len values in, out_len values out, no padding, so any read or write the
// kernels' predicates let through outside them is a heap overflow.  Both paths (the one-launch kernel and the gather / scatter
// fallback), all three output modes, the edge cases of tests/filter_ladder.py.  TEST INFRASTRUCTURE ONLY.
#include <stdio.h>

#include <complex>

#include "emu_filter.cpp"

template <typename T>
static int one(int n, int M, int slen, int mode, int flags, int expect_fused) {
    typedef std::complex<T> Z;
    const int ol = mode == 0 ? slen + M - 1 : slen, off = mode == 2 ? (M - 1) / 2 : 0;
    Z* x = new Z[slen];
    Z* h = new Z[M];
    Z* y = new Z[ol];
    unsigned s = 12345u + (unsigned)(n * 131 + M * 17 + slen);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((int)(s >> 20) % 17 - 8); };  // small integers: the direct sum is exact
    for (int i = 0; i < slen; i++) x[i] = Z(rnd(), rnd());
    for (int i = 0; i < M; i++) h[i] = Z(rnd(), rnd());
    for (int i = 0; i < ol; i++) y[i] = Z((T)777, (T)777);
    int info[8] = {0};
    const int rc = emu_filter(x, y, nullptr, nullptr, M, h, slen, 1, n, mode, 0, 0, sizeof(T) == 4 ? 1 : 0, 0, flags, info);
    int bad = rc != 0 || (expect_fused >= 0 && (info[1] == 3) != (expect_fused == 1));
    double worst = 0, scale = 0;
    for (int p = 0; p < ol && !bad; p++) {
        std::complex<double> acc(0, 0);
        for (int j = 0; j < M; j++) {
            const int q = p + off - j;
            if (q >= 0 && q < slen) acc += std::complex<double>(h[j]) * std::complex<double>(x[q]);
        }
        const double d = std::abs(std::complex<double>(y[p]) - acc);
        if (d > worst) worst = d;
        if (std::abs(acc) > scale) scale = std::abs(acc);
    }
    const double tol = (sizeof(T) == 4 ? 1e-4 : 1e-12) * (scale > 1 ? scale : 1);
    if (worst > tol) bad = 1;
    printf("%s n=%d M=%d len=%d mode=%d flags=%d: rc=%d path=%d n=%d worst=%.3g %s\n", sizeof(T) == 4 ? "fp32" : "fp64", n, M, slen, mode, flags, rc, info[1],
           info[5], worst, bad ? "FAILED" : "ok");
    delete[] x;
    delete[] h;
    delete[] y;
    return bad;
}

int main() {
    static const int cases[][3] = {{4, 1, 9}, {4, 2, 7}, {4, 3, 6}, {8, 8, 20}, {8, 5, 13}, {8, 4, 1}, {64, 1, 130}, {64, 2, 189}, {64, 3, 187}, {64, 3, 185},
                                   {64, 32, 300}, {64, 33, 129}, {64, 5, 17}, {64, 17, 136}, {256, 17, 500}, {0, 31, 300}};
    int bad = 0;
    for (const auto& c : cases)
        for (int mode = 0; mode < 3; mode++)
            for (int flags = 0; flags < 2; flags++) {
                bad += one<float>(c[0], c[1], c[2], mode, flags, flags ? 0 : 1);
                bad += one<double>(c[0], c[1], c[2], mode, flags, flags ? 0 : 1);
            }
    bad += one<float>(1024, 255, 1700, 0, 0, 1);
    bad += one<double>(256, 17, 500, 0, 2, 0);  // no_chain
    if (bad) {
        printf("%d case(s) FAILED\n", bad);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
