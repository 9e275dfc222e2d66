// kidmp_diag.hip -- the small kernels around the column step (aerosol defaults, domain reductions, the sanity scan,
// effective radii, the fastmath probe) and the entries of include/kidmp.h that wrap them.
// Built with the plain HIPFLAGS (no -fapprox-func): case 9 of k_math_probe relies on it.
#include "kidmp_ctx.h"
#include "fastmath.h"

using namespace kidmp;

namespace {
// the non-aerosol defaults of M:958-964 in the state's own arithmetic (REAL expressions of the reference)
template <class T>
__global__ void k_default_aerosols(int64_t n, T Nt_c, const T *__restrict__ qv, const T *__restrict__ t,
                                   const T *__restrict__ p, T *__restrict__ nc, T *__restrict__ nwfa, T *__restrict__ nifa)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T rho = T(0.622) * p[i] / (T(Rgas) * t[i] * (qv[i] + T(0.622)));   // M:959
    nc[i] = Nt_c / rho;                                                      // M:960
    nwfa[i] = T(11.1E6) / rho;                                               // M:961
    nifa[i] = T(naIN1) * T(0.01) / rho;                                      // M:962
}

// out4[s] = sum over columns of ppt[col][s]; one block, fixed order => reproducible
__global__ void k_reduce_ppt(int64_t ncol, const double *__restrict__ ppt, double *__restrict__ out4)
{
    __shared__ double sh[256][4];
    double acc[4] = {0., 0., 0., 0.};
    for (int64_t c = threadIdx.x; c < ncol; c += blockDim.x)
        for (int s = 0; s < 4; ++s) acc[s] += ppt[c * 4 + s];
    for (int s = 0; s < 4; ++s) sh[threadIdx.x][s] = acc[s];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (int(threadIdx.x) < w)
            for (int s = 0; s < 4; ++s) sh[threadIdx.x][s] += sh[threadIdx.x + w][s];
        __syncthreads();
    }
    if (threadIdx.x < 4) out4[threadIdx.x] = sh[0][threadIdx.x];
}

// Exact domain sums of ppt[col][0..3] (the nx-means of W:248-303 are these / nx), independent of the order of the
// additions and therefore of how the columns are sharded over devices or chunks: every value is cut into 32-bit
// pieces on a fixed-point grid (least significant bit 2**-128, six 64-bit limbs per species, limb j weighs
// 2**(32 j - 128)) and the pieces are added with integer atomics.  Integer addition is associative, so one GPU, eight
// GPUs or two contexts on one GPU end with the same 24 limbs, bit for bit; an all-reduce(SUM) of int64 limbs over the
// devices keeps that.  Range: |x| < 2**32; bits below 2**-128 (3e-39) are dropped; non-finite values are ignored.
template <class T>
__global__ void k_ppt_exact(int64_t ncol, const T *__restrict__ ppt, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long sh[ACC_N];
    if (threadIdx.x < ACC_N) sh[threadIdx.x] = 0ull;
    __syncthreads();
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < 4 * ncol; i += int64_t(gridDim.x) * blockDim.x) {
        const double x = double(ppt[i]);
        const int sp = int(i & 3);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
        const int e = int((bits >> 52) & 0x7ff);
        if (e == 0 || e >= 1023 + 32) continue;                       // zero / subnormal: below the grid; >= 2**32, inf, nan: ignored
        unsigned long long m = (bits & ((1ull << 52) - 1)) | (1ull << 52);   // x = m * 2**(e - 1075)
        int shft = e - 1075 + 128;                                    // position of m's bit 0 on the grid
        if (shft < 0) {
            if (shft <= -53) continue;
            m >>= -shft;
            shft = 0;
        }
        const int j = shft >> 5, r = shft & 31;                       // shft <= 107: j <= 3, pieces land in limbs j .. j+2 <= 5
        const unsigned long long lo = m << r, hi = r ? (m >> (64 - r)) : 0ull;
        unsigned long long pc[3] = {lo & 0xffffffffull, lo >> 32, hi};
        const bool neg = (bits >> 63) != 0;
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (pc[q]) atomicAdd(&sh[sp * ACC_LIMBS + j + q], neg ? (0ull - pc[q]) : pc[q]);   // two's complement
    }
    __syncthreads();
    if (threadIdx.x < ACC_N && sh[threadIdx.x]) atomicAdd(&acc[threadIdx.x], sh[threadIdx.x]);
}

// Domain sums of the rate diagnostics: part[chunk][r*nz+k] = sum over the chunk's columns (fixed order), then
// out[r*nz+k] = sum over chunks (fixed order) => bitwise reproducible for a given ncol.
__global__ void k_reduce_rates_part(int64_t ncol, int n, const double *__restrict__ rates, double *__restrict__ part)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // r*nz + k
    if (i >= n) return;
    const int64_t per = (ncol + RED_CHUNKS - 1) / RED_CHUNKS;
    const int64_t c0 = int64_t(blockIdx.y) * per, c1 = c0 + per < ncol ? c0 + per : ncol;
    double acc = 0.;
    for (int64_t c = c0; c < c1; ++c) acc += rates[c * n + i];
    part[int64_t(blockIdx.y) * n + i] = acc;
}
__global__ void k_reduce_rates_final(int n, const double *__restrict__ part, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double acc = 0.;
    for (int c = 0; c < RED_CHUNKS; ++c) acc += part[int64_t(c) * n + i];
    out[i] = acc;
}

// The sanity scan the scheme's own 3-D driver runs after every column (M:1025-1094): running maxima of
// qc, qr, nr, qs, qi, qg, ni and a look-out for negative values (there: WARNING strings; here: counts).
// out[0..SANITY_MAX-1] = maxima (>= 0), then SANITY_NEG numbers of negative entries of qc,qr,nr,qs,qi,qg,ni,qv.
// Maxima of non-negative doubles order like their bit patterns, so both halves are exact integer atomics.
struct SanityPtrs { const double *v[SANITY_NEG]; };
__global__ void k_sanity(int64_t n, SanityPtrs p, unsigned long long *acc)
{
    __shared__ unsigned long long sh[SANITY_N];
    if (threadIdx.x < SANITY_N) sh[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long mx[SANITY_MAX] = {};
    unsigned neg[SANITY_NEG] = {};
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
#pragma unroll
        for (int a = 0; a < SANITY_NEG; ++a) {
            const double x = p.v[a][i];
            if (x < 0.) ++neg[a];
            else if (a < SANITY_MAX && x > 0.) {                       // +-0 and NaN are no candidates (-0.0 has the largest bit pattern)
                const unsigned long long b = (unsigned long long)__double_as_longlong(x);
                mx[a] = b > mx[a] ? b : mx[a];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < SANITY_MAX; ++a) atomicMax(&sh[a], mx[a]);
#pragma unroll
    for (int a = 0; a < SANITY_NEG; ++a) if (neg[a]) atomicAdd(&sh[SANITY_MAX + a], (unsigned long long)neg[a]);
    __syncthreads();
    if (threadIdx.x < SANITY_MAX) atomicMax(&acc[threadIdx.x], sh[threadIdx.x]);
    else if (threadIdx.x < SANITY_N && sh[threadIdx.x]) atomicAdd(&acc[threadIdx.x], sh[threadIdx.x]);
}
__global__ void k_sanity_final(const unsigned long long *acc, double *out15)
{
    const int i = threadIdx.x;
    if (i < SANITY_MAX) out15[i] = __longlong_as_double((long long)acc[i]);
    else if (i < SANITY_N) out15[i] = double(acc[i]);
}

// calc_effectRad, M:4834-4935: effective radii of cloud water, cloud ice and snow for radiation coupling.  Pointwise in
// (column, level); re_* are INOUT (a level without the species keeps the caller's value, M:4873/4888/4897).  The
// reference's column-wide has_qc/has_qi/has_qs flags only skip loops whose bodies test the level again.
struct RadConsts { double Nt_c, cig2, oig1, oams, cse1, sa[10], sb[10]; int aero; };
__global__ void k_effective_radii(int64_t n, RadConsts c, const double *__restrict__ t, const double *__restrict__ p,
                                  const double *__restrict__ qv, const double *__restrict__ qc, const double *__restrict__ nc1,
                                  const double *__restrict__ qi, const double *__restrict__ ni1, const double *__restrict__ qs,
                                  double *__restrict__ re_qc, double *__restrict__ re_qi, double *__restrict__ re_qs)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), int(blockDim.x));           // the snow moment below is a fastmath.h power
    __syncthreads();
#endif
    if (i >= n) return;
    const double am_r_ = PI * rho_w / 6.0, am_i_ = PI * rho_i / 6.0;
    const double rho = 0.622 * p[i] / (Rgas * t[i] * (qv[i] + 0.622));
    const double rc = fmax(R1, qc[i] * rho);
    double nc = fmax(R2, nc1[i] * rho);
    if (!c.aero) nc = c.Nt_c;                                           // .NOT. is_aerosol_aware, M:4863
    const double ri = fmax(R1, qi[i] * rho), ni = fmax(R2, ni1[i] * rho), rs = fmax(R1, qs[i] * rho);
    if (!(rc <= R1 || nc <= R2)) {                                      // M:4873-4884
        int inu_c;
        if (nc < 100.) inu_c = 15;
        else if (nc > 1.E10) inu_c = 2;
        else { inu_c = int(lround(1000.E6 / nc)) + 2; inu_c = inu_c < 15 ? inu_c : 15; }
        const double g_ratio = double((inu_c + 1) * (inu_c + 2) * (inu_c + 3));   // 24, 60, 120 ... 4896 = (n+1)(n+2)(n+3)
        const double lamc = fm::cbrt_pos(nc * am_r_ * g_ratio / rc);
        re_qc[i] = fmax(2.51E-6, fmin(0.5 * double(3. + inu_c) / lamc, 50.E-6));
    }
    if (!(ri <= R1 || ni <= R2)) {                                      // M:4887-4893
        const double lami = fm::cbrt_pos(am_i_ * c.cig2 * c.oig1 * ni / ri);
        re_qi[i] = fmax(5.01E-6, fmin(0.5 * double(3. + mu_i) / lami, 125.E-6));
    }
    if (!(rs <= R1)) {                                                  // M:4896-4930 (bm_s = 2: smo2 = smob)
        const double tc0 = fmin(-0.1, t[i] - 273.15), x = c.cse1;
        const double smob = rs * c.oams;
        const double *a = c.sa, *b = c.sb;
        const double loga_ = a[0] + a[1] * tc0 + a[2] * x + a[3] * tc0 * x + a[4] * tc0 * tc0 + a[5] * x * x
                           + a[6] * tc0 * tc0 * x + a[7] * tc0 * x * x + a[8] * tc0 * tc0 * tc0 + a[9] * x * x * x;
        const double b_ = b[0] + b[1] * tc0 + b[2] * x + b[3] * tc0 * x + b[4] * tc0 * tc0 + b[5] * x * x
                        + b[6] * tc0 * tc0 * x + b[7] * tc0 * x * x + b[8] * tc0 * tc0 * tc0 + b[9] * x * x * x;
        const double smoc = fm::pow10_times_pow(loga_, fm::log2_parts(smob), b_);
        re_qs[i] = fmax(10.E-6, fmin(0.5 * (smoc / smob), 999.E-6));
    }
}

// device evaluation of the kernel's math helpers (fastmath.h) for the accuracy test
__global__ void k_math_probe(int fn, int64_t n, const double *x, const double *y, double *out)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), int(blockDim.x));
    __syncthreads();
#endif
    if (i >= n) return;
    double r = 0.;
    switch (fn) {
    case KIDMP_MATH_LOG:   r = fm::log(x[i]); break;
    case KIDMP_MATH_LOG10: r = fm::log10(x[i]); break;
    case KIDMP_MATH_EXP:   r = fm::exp(x[i]); break;
    case KIDMP_MATH_EXP10: r = fm::exp10(x[i]); break;
    case KIDMP_MATH_SQRT:  r = fm::sqrt_pos(x[i]); break;
    case KIDMP_MATH_CBRT:  r = fm::cbrt_pos(x[i]); break;
    case KIDMP_MATH_POW:   r = fm::pow(x[i], y[i]); break;
    case 7: r = __builtin_amdgcn_rcp(y[i]); break;                                   // raw v_rcp_f64
    case 8: r = fm::div(x[i], y[i]); break;                                          // the kernel's division
    case 9: r = x[i] / y[i]; break;                                                  // IEEE division (this file is built without -fapprox-func)
    case 10: r = fm::rcp(y[i]); break;                                               // the kernel's reciprocal
    }
    out[i] = r;
}
}  // namespace

template <class T> void kidmp::launch_default_aerosols(int64_t n, T Nt_c, const T *qv, const T *t, const T *p, T *nc, T *nwfa, T *nifa, hipStream_t s)
{
    hipLaunchKernelGGL(k_default_aerosols<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, Nt_c, qv, t, p, nc, nwfa, nifa);
}
template void kidmp::launch_default_aerosols<double>(int64_t, double, const double *, const double *, const double *, double *, double *, double *, hipStream_t);
template void kidmp::launch_default_aerosols<float>(int64_t, float, const float *, const float *, const float *, float *, float *, float *, hipStream_t);

template <class T> hipError_t kidmp::launch_ppt_exact(int64_t ncol, const T *ppt, unsigned long long *acc, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    int64_t g = (4 * ncol + 255) / 256;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(k_ppt_exact<T>, dim3((unsigned)g), dim3(256), 0, s, ncol, ppt, acc);
    return hipGetLastError();
}
template hipError_t kidmp::launch_ppt_exact<double>(int64_t, const double *, unsigned long long *, hipStream_t);
template hipError_t kidmp::launch_ppt_exact<float>(int64_t, const float *, unsigned long long *, hipStream_t);

void kidmp::launch_sanity(int64_t n, const double *const (&v)[SANITY_NEG], unsigned long long *acc, hipStream_t s)
{
    SanityPtrs p;
    for (int a = 0; a < SANITY_NEG; ++a) p.v[a] = v[a];
    int64_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(k_sanity, dim3((unsigned)g), dim3(256), 0, s, n, p, acc);
}

extern "C" {
int kidmp_default_aerosols_device(kidmp_ctx *ctx, int64_t n, const double *qv, const double *t, const double *p,
                                  double *nc, double *nwfa, double *nifa, void *stream)
{
    if (int rc = require_ready(ctx)) return rc;
    if (n < 0 || !qv || !t || !p || !nc || !nwfa || !nifa) return fail(ctx, KIDMP_EINVAL, "kidmp_default_aerosols_device: bad argument");
    if (n == 0) return KIDMP_OK;
    GUARD(ctx);
    if (int rc = check_on_device(ctx, qv, "qv")) return rc;
    if (int rc = check_on_device(ctx, nc, "nc")) return rc;
    launch_default_aerosols<double>(n, ctx->hc.Nt_c, qv, t, p, nc, nwfa, nifa, (hipStream_t)stream);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}

int kidmp_math_probe(kidmp_ctx *ctx, int32_t fn, int64_t n, const double *x, const double *y, double *out)
{
    if (int rc = require_ready(ctx)) return rc;
    if (n < 0 || !x || !y || !out || fn < 0 || fn > 10) return fail(ctx, KIDMP_EINVAL, "kidmp_math_probe: bad argument");
    if (n == 0) return KIDMP_OK;
    GUARD(ctx);
    double *d = nullptr;
    HIPTRY(ctx, hipMalloc(&d, size_t(n) * 3 * sizeof(double)));
    hipError_t e = hipMemcpy(d, x, size_t(n) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, y, size_t(n) * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_math_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, fn, n, d, d + n, d + 2 * n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, size_t(n) * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPTRY(ctx, e);
    return KIDMP_OK;
}

int kidmp_reduce_ppt_device(kidmp_ctx *ctx, int64_t ncol, const double *ppt, double *out4, void *stream)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0 || !ppt || !out4) return fail(ctx, KIDMP_EINVAL, "kidmp_reduce_ppt_device: bad argument");
    GUARD(ctx);
    if (int rc = check_on_device(ctx, ppt, "ppt")) return rc;
    if (int rc = check_on_device(ctx, out4, "out4")) return rc;
    hipLaunchKernelGGL(k_reduce_ppt, dim3(1), dim3(256), 0, (hipStream_t)stream, ncol, ppt, out4);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}

int kidmp_reduce_rates_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *rates, double *out, void *stream)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0 || nz < 2 || nz > KIDMP_MAX_NZ || !rates || !out) return fail(ctx, KIDMP_EINVAL, "kidmp_reduce_rates_device: bad argument");
    GUARD(ctx);
    if (int rc = check_on_device(ctx, rates, "rates")) return rc;
    if (int rc = check_on_device(ctx, out, "out")) return rc;
    const int n = KIDMP_NRATES * nz;
    if (size_t(RED_CHUNKS) * size_t(n) > ctx->red_elems) return fail(ctx, KIDMP_EINVAL, "kidmp_reduce_rates_device: nz beyond KIDMP_MAX_NZ");
    const int T = 128;
    hipLaunchKernelGGL(k_reduce_rates_part, dim3((n + T - 1) / T, RED_CHUNKS), dim3(T), 0, (hipStream_t)stream, ncol, n, rates, ctx->d_red);
    hipLaunchKernelGGL(k_reduce_rates_final, dim3((n + T - 1) / T), dim3(T), 0, (hipStream_t)stream, n, ctx->d_red, out);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}

int kidmp_sanity_device(kidmp_ctx *ctx, int64_t n, const double *qc, const double *qr, const double *nr, const double *qs,
                        const double *qi, const double *qg, const double *ni, const double *qv, double *out15, void *stream)
{
    if (int rc = require_ready(ctx)) return rc;
    if (n < 0 || !qc || !qr || !nr || !qs || !qi || !qg || !ni || !qv || !out15) return fail(ctx, KIDMP_EINVAL, "kidmp_sanity_device: bad argument");
    GUARD(ctx);
    if (int rc = check_on_device(ctx, qc, "qc")) return rc;
    if (int rc = check_on_device(ctx, out15, "out15")) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPTRY(ctx, hipMemsetAsync(ctx->d_sanity, 0, SANITY_N * sizeof(unsigned long long), s));
    if (n > 0) launch_sanity(n, {qc, qr, nr, qs, qi, qg, ni, qv}, ctx->d_sanity, s);
    hipLaunchKernelGGL(k_sanity_final, dim3(1), dim3(64), 0, s, ctx->d_sanity, out15);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}

int kidmp_effective_radii_device(kidmp_ctx *ctx, int64_t n, const double *t, const double *p, const double *qv,
                                 const double *qc, const double *nc, const double *qi, const double *ni, const double *qs,
                                 double *re_qc, double *re_qi, double *re_qs, void *stream)
{
    if (int rc = require_ready(ctx)) return rc;
    if (n < 0 || !t || !p || !qv || !qc || !nc || !qi || !ni || !qs || !re_qc || !re_qi || !re_qs)
        return fail(ctx, KIDMP_EINVAL, "kidmp_effective_radii_device: bad argument");
    if (n == 0) return KIDMP_OK;
    GUARD(ctx);
    if (int rc = check_on_device(ctx, t, "t")) return rc;
    if (int rc = check_on_device(ctx, re_qc, "re_qc")) return rc;
    RadConsts c{};
    c.aero = ctx->cfg.is_aerosol_aware != 0;
    c.Nt_c = ctx->hc.Nt_c; c.cig2 = ctx->hc.cig[1]; c.oig1 = ctx->hc.oig1; c.oams = ctx->hc.oams; c.cse1 = ctx->hc.cse[0];
    for (int i = 0; i < 10; ++i) { c.sa[i] = ctx->hc.sa[i]; c.sb[i] = ctx->hc.sb[i]; }
    hipLaunchKernelGGL(k_effective_radii, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, c,
                       t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}

// the 24 limbs -> four doubles: carries propagated in 128-bit integers, then the digits summed from the top in long
// double (64-bit significand): a pure function of the limbs, so equal limbs give equal sums
int kidmp_ppt_limbs_to_sums(const int64_t *limbs, double *out4)
{
    if (!limbs || !out4) return fail(nullptr, KIDMP_EINVAL, "kidmp_ppt_limbs_to_sums: null argument");
    for (int sp = 0; sp < 4; ++sp) {
        __int128 carry = 0;
        long double v = 0.0L;
        long double digit[ACC_LIMBS + 1];
        for (int j = 0; j < ACC_LIMBS; ++j) {
            const __int128 t = (__int128)limbs[sp * ACC_LIMBS + j] + carry;
            const __int128 lowbits = t & (__int128)0xffffffffLL;           // 0 .. 2**32-1
            carry = (t - lowbits) >> 32;                                   // exact: t - lowbits is a multiple of 2**32
            digit[j] = (long double)(int64_t)lowbits;
        }
        digit[ACC_LIMBS] = (long double)(int64_t)carry;                    // signed top
        for (int j = ACC_LIMBS; j >= 0; --j) v += __builtin_ldexpl(digit[j], 32 * j - 128);
        out4[sp] = (double)v;
    }
    return KIDMP_OK;
}

int kidmp_reduce_ppt_exact_device(kidmp_ctx *ctx, int64_t ncol, const double *ppt, int64_t *limbs, void *stream)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0 || !limbs || (ncol > 0 && !ppt)) return fail(ctx, KIDMP_EINVAL, "kidmp_reduce_ppt_exact_device: bad argument");
    GUARD(ctx);
    if (int rc = check_on_device(ctx, ppt, "ppt")) return rc;
    if (int rc = check_on_device(ctx, limbs, "limbs")) return rc;
    HIPTRY(ctx, hipMemsetAsync(limbs, 0, ACC_N * sizeof(int64_t), (hipStream_t)stream));
    HIPTRY(ctx, launch_ppt_exact<double>(ncol, ppt, reinterpret_cast<unsigned long long *>(limbs), (hipStream_t)stream));
    return KIDMP_OK;
}
}  // extern "C"
