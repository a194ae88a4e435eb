// emu_real2d_main.cpp -- the emulated real 2D transform plan on EXACTLY sized heap buffers, as a stand-alone program meant to be built
// with -fsanitize=address,undefined: rows * cols reals on one side, rows * (cols/2 + 1) complex values on the other, no padding, so
// any read or write the kernels' predicates let through outside them is a heap overflow.  Both paths (the column pass, whose last
// tile of every matrix has dead columns, and the transposing fallback), both directions, a matrix pitch of the caller's own, the
// column pass alone with a ragged last tile.  TEST INFRASTRUCTURE ONLY.
#include <stdio.h>

#include <complex>
#include <vector>

#include "emu_real2d.cpp"

typedef std::complex<double> D;

// X[m][k][c] of rfft2, c <= cols/2, by the direct sum
static void direct_rfft2(const std::vector<double>& x, int rows, int cols, std::vector<D>& X) {
    const int hb = cols / 2 + 1;
    const double two_pi = 6.283185307179586476925286766559;
    X.assign((size_t)rows * hb, D(0, 0));
    for (int k = 0; k < rows; k++)
        for (int c = 0; c < hb; c++) {
            D acc(0, 0);
            for (int r = 0; r < rows; r++)
                for (int q = 0; q < cols; q++) {
                    const double a = -two_pi * ((double)((long long)k * r % rows) / rows + (double)((long long)c * q % cols) / cols);
                    acc += x[(size_t)r * cols + q] * D(cos(a), sin(a));
                }
            X[(size_t)k * hb + c] = acc;
        }
}

template <typename T>
static int one(int rows, int cols, int M, int flags, int min_seg, int lds_budget, int extra_pitch) {
    typedef std::complex<T> Z;
    const int hb = cols / 2 + 1;
    const long long rm = (long long)rows * cols, sm = (long long)rows * hb;
    const long long rp = rm + extra_pitch, sp = sm + extra_pitch;
    const size_t nreal = (size_t)((M - 1) * rp + rm), nspec = (size_t)((M - 1) * sp + sm);
    T* x = new T[nreal];
    Z* X = new Z[nspec];
    T* y = new T[nreal];
    unsigned s = 4321u + (unsigned)(rows * 131 + cols * 17 + M);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((int)(s >> 20) % 9 - 4); };  // small integers: the direct sum is nearly exact
    for (size_t i = 0; i < nreal; i++) { x[i] = rnd(); y[i] = (T)777; }
    for (size_t i = 0; i < nspec; i++) X[i] = Z((T)777, (T)777);
    int info[8] = {0}, info2[8] = {0};
    const int prec = sizeof(T) == 4 ? 1 : 0;
    const int rc = emu_real2d(x, extra_pitch ? rp : 0, X, extra_pitch ? sp : 0, rows, cols, M, 1, prec, lds_budget, flags, min_seg, info);
    const int rc2 = rc == 0 ? emu_real2d(X, extra_pitch ? sp : 0, y, extra_pitch ? rp : 0, rows, cols, M, 0, prec, lds_budget, flags, min_seg, info2) : -9;
    int bad = rc != 0 || rc2 != 0 || ((flags & 1) && (info[0] != 0 || info2[0] != 0));
    double worst = 0, scale = 1, back = 0;
    for (int m = 0; m < M && !bad; m++) {
        std::vector<double> xm((size_t)rm);
        for (long long i = 0; i < rm; i++) xm[(size_t)i] = (double)x[m * rp + i];
        std::vector<D> ref;
        direct_rfft2(xm, rows, cols, ref);
        for (long long i = 0; i < sm; i++) {
            const double d = std::abs(D(X[m * sp + i]) - ref[(size_t)i]);
            if (d > worst) worst = d;
            if (std::abs(ref[(size_t)i]) > scale) scale = std::abs(ref[(size_t)i]);
        }
        for (long long i = 0; i < rm; i++) {
            const double d = fabs((double)y[m * rp + i] - xm[(size_t)i]);
            if (d > back) back = d;
        }
    }
    const double eps = sizeof(T) == 4 ? 1e-5 : 1e-13;
    if (worst > eps * scale || back > eps * 16) bad = 1;
    printf("%s %dx%d M=%d flags=%d min_seg=%d lds=%d pitch+%d: rc=%d/%d fused=%d/%d C=%d tiles=%d worst=%.3g back=%.3g %s\n", sizeof(T) == 4 ? "fp32" : "fp64", rows,
           cols, M, flags, min_seg, lds_budget, extra_pitch, rc, rc2, info[0], info2[0], info[3], info[4], worst, back, bad ? "FAILED" : "ok");
    delete[] x;
    delete[] X;
    delete[] y;
    return bad;
}

// the column pass alone: n_cols live columns of [P][in_ld] into [P][out_ld], exactly sized, both directions
template <typename T>
static int colpass(int log2P, int n_cols, int in_ld, int out_ld, int inverse) {
    typedef std::complex<T> Z;
    const int P = 1 << log2P, nm = 2;
    // the last row of the last matrix ends with its last live column: nothing behind it belongs to the buffer
    const size_t nin = (size_t)(nm * P - 1) * in_ld + n_cols, nout = (size_t)(nm * P - 1) * out_ld + n_cols;
    Z* a = new Z[nin];
    Z* b = new Z[nout];
    unsigned s = 99u + (unsigned)(n_cols * 7 + in_ld);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((int)(s >> 20) % 9 - 4); };
    for (size_t i = 0; i < nin; i++) a[i] = Z(rnd(), rnd());
    for (size_t i = 0; i < nout; i++) b[i] = Z((T)777, (T)777);
    int info[4] = {0};
    const int rc = emu_colpass(a, in_ld, b, out_ld, log2P, n_cols, nm, inverse, 1.0, 0, sizeof(T) == 4 ? 1 : 0, 0, info);
    int bad = rc != 0;
    double worst = 0;
    const double two_pi = 6.283185307179586476925286766559;
    for (int m = 0; m < nm && !bad; m++)
        for (int c = 0; c < n_cols; c++)
            for (int k = 0; k < P; k++) {
                D acc(0, 0);
                for (int l = 0; l < P; l++) {
                    const double ang = (inverse ? two_pi : -two_pi) * (double)(k * l % P) / P;
                    acc += D(a[(size_t)(m * P + l) * in_ld + c]) * D(cos(ang), sin(ang));
                }
                const double d = std::abs(D(b[(size_t)(m * P + k) * out_ld + c]) - acc);
                if (d > worst) worst = d;
            }
    if (worst > (sizeof(T) == 4 ? 1e-3 : 1e-11)) bad = 1;
    for (int m = 0; m < nm && !bad; m++)  // the gaps between the rows stay untouched
        for (int k = 0; k < P; k++)
            for (int c = n_cols; c < out_ld && (size_t)(m * P + k) * out_ld + c < nout; c++)
                if (b[(size_t)(m * P + k) * out_ld + c] != Z((T)777, (T)777)) bad = 1;
    printf("%s colpass P=%d n_cols=%d in_ld=%d out_ld=%d inverse=%d: rc=%d C=%d tiles=%d worst=%.3g %s\n", sizeof(T) == 4 ? "fp32" : "fp64", P, n_cols, in_ld, out_ld,
           inverse, rc, info[0], info[1], worst, bad ? "FAILED" : "ok");
    delete[] a;
    delete[] b;
    return bad;
}

int main() {
    int bad = 0;
    for (int flags = 0; flags < 2; flags++) {
        bad += one<float>(8, 16, 3, flags, 0, 0, 0);    // the smallest fused shape: one whole tile and one with a single live column
        bad += one<double>(8, 16, 3, flags, 0, 0, 0);
        bad += one<float>(8, 16, 2, flags, 0, 0, 3);    // odd pitches: the second matrix is only 4- / 8-byte aligned
        bad += one<double>(16, 8, 2, flags, 0, 0, 5);
        bad += one<float>(64, 64, 1, flags, 16, 2000, 0);   // narrow tiles of C = V columns
        bad += one<double>(64, 64, 1, flags, 16, 3500, 0);  // C = 2 V
    }
    static const int fb[][2] = {{1, 16}, {2, 8}, {4, 4}, {8, 1}, {8, 2}, {8, 4}, {5, 9}, {12, 12}, {8, 12}, {12, 16}, {1, 1}, {1, 7}};
    for (const auto& c : fb) {
        bad += one<float>(c[0], c[1], 2, 0, 0, 0, 0);
        bad += one<double>(c[0], c[1], 2, 0, 0, 0, 1);
    }
    for (int inverse = 0; inverse < 2; inverse++) {
        bad += colpass<float>(3, 5, 7, 5, inverse);
        bad += colpass<double>(3, 9, 9, 12, inverse);
        bad += colpass<float>(4, 17, 20, 17, inverse);
    }
    if (bad) {
        printf("%d case(s) FAILED\n", bad);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
