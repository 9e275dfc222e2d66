// kidmp_mathprobe.hip -- kidmp_math_probe_ex: device evaluation of every function of fastmath.h, binary64 and binary32,
// and of the plain binary32 division, for the accuracy tests.
// Built with HIPFLAGS + COLFLAGS, the flags of the three column objects (-fapprox-func -freciprocal-math): what this
// unit's `x / y` and `1 / y` compile to is what the column kernel's REAL operands get (operator/(A, Qden<B>) and
// frcp<float> of thompson_column.hip).  kidmp_math_probe (kidmp_diag.hip, plain HIPFLAGS) stays as the reference point.
#include "kidmp_ctx.h"
#include "fastmath.h"
#include "limit_bracket.h"

using namespace kidmp;

namespace {
// IEEE binary64 division inside a unit whose flags turn `a / b` into a reciprocal and Newton steps: the scale / fmas /
// fixup sequence that the compiler emits for a plain fp64 quotient without those flags, written out
__device__ inline double ieee_div(double a, double b)
{
    bool scaled_den, vcc;
    const double d = __builtin_amdgcn_div_scale(a, b, false, &scaled_den);
    const double n = __builtin_amdgcn_div_scale(a, b, true, &vcc);
    double y = __builtin_amdgcn_rcp(d);
    y = __builtin_fma(y, __builtin_fma(-d, y, 1.0), y);
    y = __builtin_fma(y, __builtin_fma(-d, y, 1.0), y);
    const double q = n * y;
    return __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(__builtin_fma(-d, q, n), y, q, vcc), b, a);
}

__device__ inline double rcp_seed(double b) { return __builtin_amdgcn_rcp(b); }    // raw v_rcp_f64
__device__ inline float rcp_seed(float b) { return __builtin_amdgcn_rcpf(b); }     // raw v_rcp_f32

// the codes that exist in both arithmetics, T = double or float (operands narrowed exactly: the caller passes
// binary32-representable values)
template <class T> __device__ inline T eval(int fn, T x, T y, T z)
{
    switch (fn) {
    case KIDMP_MATH_LOG:      return fm::log(x);
    case KIDMP_MATH_LOG10:    return fm::log10(x);
    case KIDMP_MATH_EXP:      return fm::exp(x);
    case KIDMP_MATH_EXP10:    return fm::exp10(x);
    case KIDMP_MATH_SQRT:     return fm::sqrt_pos(x);
    case KIDMP_MATH_CBRT:     return fm::cbrt_pos(x);
    case KIDMP_MATH_POW:      return fm::pow(x, y);
    case KIDMP_MATH_RCP_SEED: return rcp_seed(y);
    case KIDMP_MATH_POW10_TIMES_POW: return fm::pow10_times_pow(x, fm::log2_parts(y), z);
    case KIDMP_MATH_PLAIN_DIV: return x / y;                                       // as the column objects compile it
    case KIDMP_MATH_PLAIN_RCP: return T(1) / y;
    }
    return T(0);
}

// one size-limit test by limit_bracket.h and by the column kernel's original expression (the ice test multiplies by the
// kernel's reciprocal, the other two divide): decide() + 4 * original + 16 * certainly_inside() (what the kernel votes on)
__device__ inline double limit_both_ways(double num, double den, int site)
{
    const double lam = fm::cbrt_pos(fm::div(num, den));
    int b, o;
    bool in;
    if (site == 0) {
        b = lb::decide(num, den, lb::F_ICE);
        in = lb::certainly_inside(num, den, lb::F_ICE);
        const double xD = lb::SITE_ICE.c * fm::rcp(lam);
        o = xD < lb::SITE_ICE.D_lo ? lb::BELOW : xD > lb::SITE_ICE.D_hi ? lb::ABOVE : lb::INSIDE;
    } else if (site == 1) {
        b = lb::decide(num, den, lb::F_RAIN);
        in = lb::certainly_inside(num, den, lb::F_RAIN);
        const double xD = fm::div(lb::SITE_RAIN.c, lam);
        o = xD > lb::SITE_RAIN.D_hi ? lb::ABOVE : xD < lb::SITE_RAIN.D_lo ? lb::BELOW : lb::INSIDE;
    } else {
        const double c = lb::cloud_c(site);
        b = lb::decide_scaled(num, den, c * c * c, lb::F_CLOUD);
        in = lb::certainly_inside_scaled(num, den, c * c * c, lb::F_CLOUD);
        const double xD = fm::div(c, lam);
        o = xD < lb::SITE_CLOUD.D_lo ? lb::BELOW : xD > lb::SITE_CLOUD.D_hi ? lb::ABOVE : lb::INSIDE;
    }
    return double(b + 4 * o + 16 * int(in));
}

__global__ void k_math_probe_ex(int fn, int binary32, int64_t n, const double *x, const double *y, const double *z, double *out)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), int(blockDim.x));
    __syncthreads();
#endif
    if (i >= n) return;
    double r;
    switch (fn) {
    case KIDMP_MATH_DIV:    r = fm::div(x[i], y[i]); break;                        // binary64 only (refused otherwise)
    case KIDMP_MATH_RCP:    r = fm::rcp(y[i]); break;
    case KIDMP_MATH_IEEE_DIV: r = ieee_div(x[i], y[i]); break;
    case KIDMP_MATH_POW_DF: r = fm::pow(x[i], float(y[i])); break;                 // DOUBLE**REAL
    case KIDMP_MATH_POW_FD: r = fm::pow(float(x[i]), y[i]); break;                 // REAL**DOUBLE
    case KIDMP_MATH_LIMIT_BRACKET: r = limit_both_ways(x[i], y[i], int(z[i])); break;
    default:
        r = binary32 ? double(eval<float>(fn, float(x[i]), float(y[i]), float(z[i]))) : eval<double>(fn, x[i], y[i], z[i]);
    }
    out[i] = r;
}
}  // namespace

int kidmp_math_probe_ex(kidmp_ctx *ctx, int32_t fn, int32_t binary32, int64_t n, const double *x, const double *y, const double *z,
                        double *out)
{
    if (int rc = require_ready(ctx)) return rc;
    if (n < 0 || !x || !y || !z || !out || fn < 0 || (fn > KIDMP_MATH_POW_FD && fn != KIDMP_MATH_LIMIT_BRACKET))
        return fail(ctx, KIDMP_EINVAL, "kidmp_math_probe_ex: bad argument");
    const bool only64 = fn == KIDMP_MATH_DIV || fn == KIDMP_MATH_IEEE_DIV || fn == KIDMP_MATH_RCP || fn == KIDMP_MATH_POW_DF ||
                        fn == KIDMP_MATH_POW_FD || fn == KIDMP_MATH_LIMIT_BRACKET;
    if (binary32 && only64)
        return fail(ctx, KIDMP_EINVAL, "kidmp_math_probe_ex: the three fp64 divisions, the mixed-type powers and the limit bracket have no binary32 form");
    if (fn == KIDMP_MATH_LIMIT_BRACKET)
        for (int64_t i = 0; i < n; ++i)
            if (!(z[i] >= 0. && z[i] <= 15.) || z[i] != double(int(z[i])))
                return fail(ctx, KIDMP_EINVAL, "kidmp_math_probe_ex: the limit bracket's site is an integer 0 .. 15");
    if (n == 0) return KIDMP_OK;
    GUARD(ctx);
    double *d = nullptr;
    HIPTRY(ctx, hipMalloc(&d, size_t(n) * 4 * sizeof(double)));
    hipError_t e = hipMemcpy(d, x, size_t(n) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, y, size_t(n) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * n, z, size_t(n) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_math_probe_ex, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, fn, binary32 != 0, n, d, d + n,
                           d + 2 * n, d + 3 * n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d + 3 * n, size_t(n) * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPTRY(ctx, e);
    return KIDMP_OK;
}
