// Host evaluation of kid_amd/csrc/fastmath.h on given operands (no GPU): the counterpart of kidmp_math_probe_ex, with the
// same function codes (include/kidmp.h) and the same narrowing to float for binary32.
//   fastmath_eval IN OUT
// IN:  int32 fn, int32 binary32, int64 n, then x[n], y[n], z[n] as raw doubles.   OUT: n raw doubles.
// KIDMP_MATH_RCP_SEED is a hardware instruction and has no host form (exit status 2); the plain divisions are IEEE here.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fastmath.h"
#include "kidmp.h"

namespace fm = kidmp::fm;

template <class T> static bool eval(int fn, T x, T y, T z, T &r)
{
    switch (fn) {
    case KIDMP_MATH_LOG:      r = fm::log(x); return true;
    case KIDMP_MATH_LOG10:    r = fm::log10(x); return true;
    case KIDMP_MATH_EXP:      r = fm::exp(x); return true;
    case KIDMP_MATH_EXP10:    r = fm::exp10(x); return true;
    case KIDMP_MATH_SQRT:     r = fm::sqrt_pos(x); return true;
    case KIDMP_MATH_CBRT:     r = fm::cbrt_pos(x); return true;
    case KIDMP_MATH_POW:      r = fm::pow(x, y); return true;
    case KIDMP_MATH_POW10_TIMES_POW: r = fm::pow10_times_pow(x, fm::log2_parts(y), z); return true;
    case KIDMP_MATH_PLAIN_DIV: r = x / y; return true;
    case KIDMP_MATH_PLAIN_RCP: r = T(1) / y; return true;
    }
    return false;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: fastmath_eval IN OUT\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    int32_t head[2];
    int64_t n;
    if (!f || fread(head, sizeof head, 1, f) != 1 || fread(&n, sizeof n, 1, f) != 1 || n < 0) return 1;
    const int fn = head[0];
    const bool b32 = head[1] != 0;
    std::vector<double> x(n), y(n), z(n), out(n);
    for (std::vector<double> *v : {&x, &y, &z})
        if (n && fread(v->data(), sizeof(double), size_t(n), f) != size_t(n)) return 1;
    fclose(f);
    for (int64_t i = 0; i < n; ++i) {
        bool ok = true;
        switch (fn) {
        case KIDMP_MATH_DIV:      ok = !b32; out[i] = fm::div(x[i], y[i]); break;
        case KIDMP_MATH_RCP:      ok = !b32; out[i] = fm::rcp(y[i]); break;
        case KIDMP_MATH_IEEE_DIV: ok = !b32; out[i] = x[i] / y[i]; break;
        case KIDMP_MATH_POW_DF:   ok = !b32; out[i] = fm::pow(x[i], float(y[i])); break;
        case KIDMP_MATH_POW_FD:   ok = !b32; out[i] = fm::pow(float(x[i]), y[i]); break;
        default:
            if (b32) { float r = 0.f; ok = eval<float>(fn, float(x[i]), float(y[i]), float(z[i]), r); out[i] = double(r); }
            else ok = eval<double>(fn, x[i], y[i], z[i], out[i]);
        }
        if (!ok) return 2;
    }
    f = fopen(argv[2], "wb");
    if (!f || (n && fwrite(out.data(), sizeof(double), size_t(n), f) != size_t(n)) || fclose(f) != 0) return 1;
    return 0;
}
