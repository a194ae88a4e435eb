// emu_conv2d_main.cpp -- the emulated 2D convolution plan on EXACTLY sized heap buffers, as a stand-alone program meant to be built
// with -fsanitize=address,undefined: rows * cols values in, out_rows * out_cols values out, no padding, so any read or write the
// kernels' predicates let through outside them is a heap overflow.  Both paths (the column round and the padded fallback), the five
// modes, the small shapes of tests/conv2d_ladder.py.  TEST INFRASTRUCTURE ONLY.
#include <stdio.h>

#include <complex>

#include "emu_conv2d.cpp"

template <typename T>
static int one(int rows, int cols, int krows, int kcols, int mode, int flags, int min_seg, int lds_budget) {
    typedef std::complex<T> Z;
    typedef std::complex<double> D;
    int P, Q, orows, ocols;
    if (!ffteng::Conv2DPlan<T, emu::Runtime>::sizes(rows, cols, krows, kcols, mode, P, Q, orows, ocols)) return 1;
    Z* x = new Z[rows * cols];
    Z* k = new Z[krows * kcols];
    Z* y = new Z[orows * ocols];
    unsigned s = 12345u + (unsigned)(rows * 131 + cols * 17 + krows * 7 + kcols);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((int)(s >> 20) % 9 - 4); };  // small integers: the direct sum is exact
    for (int i = 0; i < rows * cols; i++) x[i] = Z(rnd(), rnd());
    for (int i = 0; i < krows * kcols; i++) k[i] = Z(rnd(), rnd());
    for (int i = 0; i < orows * ocols; i++) y[i] = Z((T)777, (T)777);
    int info[8] = {0};
    const int rc = emu_conv2d(x, y, nullptr, nullptr, rows, cols, krows, kcols, k, 1, mode, 0, 0, sizeof(T) == 4 ? 1 : 0, lds_budget, flags, min_seg, info);
    int bad = rc != 0 || ((flags & 1) && info[0] != 0);
    const int sr = mode == 1 ? (krows - 1) / 2 : mode == 2 ? krows - 1 : 0, sc = mode == 1 ? (kcols - 1) / 2 : mode == 2 ? kcols - 1 : 0;
    double worst = 0, scale = 0;
    for (int u = 0; u < orows && !bad; u++)
        for (int v = 0; v < ocols; v++) {
            D acc(0, 0);
            for (int i = 0; i < krows; i++)
                for (int j = 0; j < kcols; j++) {
                    int a = u + sr - i, b = v + sc - j;
                    if (mode == 3) { a = ((a % rows) + rows) % rows; b = ((b % cols) + cols) % cols; }
                    if (a >= 0 && a < rows && b >= 0 && b < cols) acc += D(k[i * kcols + j]) * D(x[a * cols + b]);
                }
            const double d = std::abs(D(y[u * ocols + v]) - acc);
            if (d > worst) worst = d;
            if (std::abs(acc) > scale) scale = std::abs(acc);
        }
    const double tol = (sizeof(T) == 4 ? 1e-4 : 1e-12) * (scale > 1 ? scale : 1);
    if (worst > tol) bad = 1;
    printf("%s %dx%d * %dx%d mode=%d flags=%d min_seg=%d lds=%d: rc=%d fused=%d P=%d Q=%d C=%d worst=%.3g %s\n", sizeof(T) == 4 ? "fp32" : "fp64", rows, cols,
           krows, kcols, mode, flags, min_seg, lds_budget, rc, info[0], info[2], info[3], info[6], worst, bad ? "FAILED" : "ok");
    delete[] x;
    delete[] k;
    delete[] y;
    return bad;
}

int main() {
    static const int linear[][4] = {{5, 6, 3, 3}, {2, 3, 2, 2}, {1, 7, 8, 2}, {7, 1, 2, 1}, {3, 3, 6, 5}, {6, 20, 3, 9}, {20, 6, 9, 3}, {15, 9, 2, 8}, {8, 8, 1, 1}};
    int bad = 0;
    for (const auto& c : linear)
        for (int mode = 0; mode < 3; mode++) {
            if (mode == 2 && (c[2] > c[0] || c[3] > c[1])) continue;
            for (int flags = 0; flags < 2; flags++) {  // the precisions take turns: every shape and mode runs both paths, each in one of them
                if ((mode + flags) & 1) bad += one<float>(c[0], c[1], c[2], c[3], mode, flags, 0, 0);
                else bad += one<double>(c[0], c[1], c[2], c[3], mode, flags, 0, 0);
            }
        }
    for (int flags = 0; flags < 2; flags++) {
        bad += one<float>(8, 16, 3, 5, 3, flags, 0, 0);
        bad += one<double>(16, 8, 16, 1, 3, flags, 0, 0);
        bad += one<float>(50, 27, 3, 3, 1, flags, 16, 2000);   // P = 64, Q = 32 in narrow tiles of C = V columns: sixteen per matrix
        bad += one<double>(50, 27, 3, 3, 1, flags, 16, 3500);  // C = 2 V
    }
    if (bad) {
        printf("%d case(s) FAILED\n", bad);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
