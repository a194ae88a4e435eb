// emu_dct_main.cpp -- the emulated cosine / sine transform plans on EXACTLY sized heap buffers, as a stand-alone program meant to be built
// with -fsanitize=address,undefined: (batch - 1) * pitch + n reals on either side, no padding behind the last row, so any read or write
// the kernels' predicates let through outside them is a heap overflow.  The fused path (whose last tile has padding rows) and the
// fallback, all four types, dense and odd pitches (component accesses at element-aligned rows), in place, and the 2D composition.
// Every result is compared with the direct sums of the definitions.  TEST INFRASTRUCTURE ONLY.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "emu_dct.cpp"

static const double kPi = 3.14159265358979323846;

// the definitions, unnormalised (fft_hip.h)
static void direct(const std::vector<double>& x, int n, int type, std::vector<double>& y) {
    y.assign((size_t)n, 0.0);
    for (int k = 0; k < n; k++) {
        double acc = 0;
        for (int m = 0; m < n; m++) {
            double c;
            if (type == 0) c = 2 * cos(kPi * (double)((long long)k * (2 * m + 1) % (4 * n)) / (2.0 * n));
            else if (type == 2) c = 2 * sin(kPi * (double)((long long)(k + 1) * (2 * m + 1) % (4 * n)) / (2.0 * n));
            else if (type == 1) c = m == 0 ? 1.0 : 2 * cos(kPi * (double)((long long)m * (2 * k + 1) % (4 * n)) / (2.0 * n));
            else c = m == n - 1 ? ((k & 1) ? -1.0 : 1.0) : 2 * sin(kPi * (double)((long long)(2 * k + 1) * (m + 1) % (4 * n)) / (2.0 * n));
            acc += c * x[(size_t)m];
        }
        y[(size_t)k] = acc;
    }
}

template <typename T>
static int one(int n, int batch, int type, int flags, int ipad, int opad, bool inplace, int want_fused) {
    const long long ip = n + ipad, op = inplace ? ip : n + opad;
    const size_t ni = (size_t)((batch - 1) * ip + n), no = (size_t)((batch - 1) * op + n);
    T* x = new T[ni];
    T* y = inplace ? x : new T[no];
    unsigned s = 99u + (unsigned)(n * 31 + batch * 7 + type);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((int)(s >> 20) % 9 - 4); };  // small integers: the direct sum is nearly exact
    std::vector<T> keep(ni);
    for (size_t i = 0; i < ni; i++) keep[i] = x[i] = rnd();
    if (!inplace) for (size_t i = 0; i < no; i++) y[i] = (T)777;
    int info[4] = {0};
    const int rc = emu_dct(x, ipad ? ip : 0, y, (inplace ? ipad : opad) ? op : 0, n, batch, type, 0, sizeof(T) == 4 ? 1 : 0, flags, info);
    int bad = rc != 0 || info[0] != want_fused;
    double worst = 0, scale = 1;
    for (int b = 0; b < batch && !bad; b++) {
        std::vector<double> xb((size_t)n), ref;
        for (int i = 0; i < n; i++) xb[(size_t)i] = (double)keep[(size_t)(b * ip + i)];
        direct(xb, n, type, ref);
        for (int i = 0; i < n; i++) {
            const double d = fabs((double)y[b * op + i] - ref[(size_t)i]);
            if (d > worst) worst = d;
            if (fabs(ref[(size_t)i]) > scale) scale = fabs(ref[(size_t)i]);
        }
        if (!inplace)  // the gap behind the row is untouched
            for (int i = n; i < op && b + 1 < batch; i++) bad |= y[b * op + i] != (T)777;
    }
    const double tol = (sizeof(T) == 4 ? 1e-5 : 1e-13) * scale * (n > 1 ? log2((double)n) : 1);
    if (worst > tol) bad = 1;
    printf("%s n=%d batch=%d type=%d flags=%d pads=%d,%d%s: rc %d fused %d worst %.3g (tol %.3g) %s\n", sizeof(T) == 4 ? "fp32" : "fp64", n, batch, type, flags, ipad,
           opad, inplace ? " in place" : "", rc, info[0], worst, tol, bad ? "FAILED" : "ok");
    delete[] x;
    if (!inplace) delete[] y;
    return bad;
}

template <typename T>
static int one2d(int rows, int cols, int M, int type, int pad) {
    const long long rm = (long long)rows * cols, ip = rm + pad, op = rm + pad;
    const size_t nn = (size_t)((M - 1) * ip + rm);
    T* x = new T[nn];
    T* y = new T[nn];
    unsigned s = 7u + (unsigned)(rows * 31 + cols);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((int)(s >> 20) % 9 - 4); };
    for (size_t i = 0; i < nn; i++) { x[i] = rnd(); y[i] = (T)777; }
    int info[4] = {0};
    const int rc = emu_dct2d(x, pad ? ip : 0, y, pad ? op : 0, rows, cols, M, type, 0, sizeof(T) == 4 ? 1 : 0, 0, info);
    int bad = rc != 0;
    double worst = 0, scale = 1;
    for (int m = 0; m < M && !bad; m++) {
        std::vector<double> t((size_t)rm), u((size_t)rm), row, res;
        for (int r = 0; r < rows; r++) {  // rows, then columns
            row.assign(x + m * ip + (long long)r * cols, x + m * ip + (long long)(r + 1) * cols);
            direct(row, cols, type, res);
            for (int c = 0; c < cols; c++) t[(size_t)r * cols + c] = res[(size_t)c];
        }
        for (int c = 0; c < cols; c++) {
            row.resize((size_t)rows);
            for (int r = 0; r < rows; r++) row[(size_t)r] = t[(size_t)r * cols + c];
            direct(row, rows, type, res);
            for (int r = 0; r < rows; r++) u[(size_t)r * cols + c] = res[(size_t)r];
        }
        for (long long i = 0; i < rm; i++) {
            const double d = fabs((double)y[m * op + i] - u[(size_t)i]);
            if (d > worst) worst = d;
            if (fabs(u[(size_t)i]) > scale) scale = fabs(u[(size_t)i]);
        }
    }
    const double tol = (sizeof(T) == 4 ? 1e-5 : 1e-13) * scale * log2((double)rm + 1);
    if (worst > tol) bad = 1;
    printf("%s 2D %dx%d M=%d type=%d pad=%d: rc %d fused %d worst %.3g (tol %.3g) %s\n", sizeof(T) == 4 ? "fp32" : "fp64", rows, cols, M, type, pad, rc, info[0],
           worst, tol, bad ? "FAILED" : "ok");
    delete[] x;
    delete[] y;
    return bad;
}

template <typename T>
static int all() {
    int bad = 0;
    const int nf = sizeof(T) == 4 ? 16 : 8;  // the shortest fused rows
    for (int type = 0; type < 4; type++) {
        bad |= one<T>(nf, 3, type, 0, 0, 0, false, 1);       // padding rows in the only tile
        bad |= one<T>(64, 5, type, 0, 3, 5, false, 1);       // element-aligned rows: component accesses
        bad |= one<T>(64, 5, type, 0, 1, 0, true, 1);        // in place
        bad |= one<T>(64, 5, type, 1, 3, 5, false, 0);       // NO_FUSION
        bad |= one<T>(12, 4, type, 0, 1, 2, false, 0);       // the fallback: Bluestein behind it
        bad |= one<T>(1, 3, type, 0, 0, 0, false, 0);
        bad |= one<T>(9, 2, type, 0, 0, 0, true, 0);
    }
    bad |= one<T>(16, sizeof(T) == 4 ? 257 : 129, 0, 0, 0, 0, false, 1);  // one tile plus one row
    bad |= one2d<T>(8, 16, 2, 0, 3);
    bad |= one2d<T>(5, 9, 2, 3, 1);
    bad |= one2d<T>(1, 1, 1, 1, 0);
    return bad;
}

int main() {
    const int bad = all<float>() | all<double>();
    printf(bad ? "SOME CASES FAILED\n" : "all cases passed\n");
    return bad ? 1 : 0;
}
