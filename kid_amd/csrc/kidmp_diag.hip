// kidmp_diag.hip -- the small kernels around the column step (aerosol defaults, domain reductions, the sanity scan,
// effective radii, the column outputs, the fastmath probe) and the entries of include/kidmp.h that wrap them.
// Built with the plain HIPFLAGS (no -fapprox-func): case 9 of k_math_probe relies on it.
#include "kidmp_ctx.h"
#include "thompson_levels.h"

using namespace kidmp;

namespace {
// the non-aerosol defaults of M:958-964 in the state's own arithmetic (REAL expressions of the reference)
template <class T>
__global__ void k_default_aerosols(int64_t n, T Nt_c, const T *__restrict__ qv, const T *__restrict__ t,
                                   const T *__restrict__ p, T *__restrict__ nc, T *__restrict__ nwfa, T *__restrict__ nifa,
                                   const double *__restrict__ set_nc_col, int64_t nz_col, int64_t e0)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (set_nc_col) Nt_c = T(set_nc_col[(e0 + i) / nz_col] * 1.e6);          // the column's own, rounded as T(Consts::Nt_c)
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
// (column, level); the arithmetic of a level is thompson_levels.h.  The reference's column-wide has_qc/has_qi/has_qs
// flags only skip loops whose bodies test the level again.
//   T     double, or float: widened on load, computed in binary64, rounded once on store (not the reference's native
//         binary32 arithmetic)
//   KEEP  the subroutine's INOUT (M:4873 / 4888 / 4897): a level without the species is not written.  Otherwise the form of
//         the scheme's driver (M:1111-1116): such a level receives the preset 2.49E-6 / 4.99E-6 / 9.99E-6 m.  The driver's
//         clamps after the call (M:1118-1120) change nothing after the subroutine's own and are not computed.
// nc1 may be null when the context is not aerosol-aware (nc = Nt_c, M:4863); null qi + ni and null qs read as zero; null
// re_qi / re_qs are not formed.  set_nc_col (null: c.Nt_c): the bound per-column set_Nc, element i in column (e0 + i) / nz_col.
template <class T, bool KEEP>
__global__ void k_effective_radii(int64_t n, RadConsts c, const T *__restrict__ t, const T *__restrict__ p,
                                  const T *__restrict__ qv, const T *__restrict__ qc, const T *__restrict__ nc1,
                                  const T *__restrict__ qi, const T *__restrict__ ni1, const T *__restrict__ qs,
                                  T *__restrict__ re_qc, T *__restrict__ re_qi, T *__restrict__ re_qs,
                                  const double *__restrict__ set_nc_col, int64_t nz_col, int64_t e0)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), int(blockDim.x));           // the snow moment below is a fastmath.h power
    __syncthreads();
#endif
    if (i >= n) return;
    const double temp = double(t[i]);
    const double rho = lvl::air_density(double(p[i]), temp, double(qv[i]));
    double re;
    const double Nt_c = set_nc_col ? set_nc_col[(e0 + i) / nz_col] * 1.e6 : c.Nt_c;
    if (lvl::cloud_water_radius(c, Nt_c, rho, double(qc[i]), nc1 ? double(nc1[i]) : 0., re)) re_qc[i] = T(re);
    else if (!KEEP) re_qc[i] = T(lvl::RE_QC_PRESET);
    if (re_qi) {
        if (qi && lvl::cloud_ice_radius(c, rho, double(qi[i]), double(ni1[i]), re)) re_qi[i] = T(re);
        else if (!KEEP) re_qi[i] = T(lvl::RE_QI_PRESET);
    }
    if (re_qs) {
        const double rs = fmax(R1, (qs ? double(qs[i]) : 0.) * rho);
        if (!(rs <= R1)) re_qs[i] = T(lvl::snow_radius(c.sa, c.sb, c.cse1, lvl::snow_level(temp, rs, c.oams)));   // M:4896-4930
        else if (!KEEP) re_qs[i] = T(lvl::RE_QS_PRESET);
    }
}

template <class T>
hipError_t launch_effective_radii(const RadConsts &c, bool keep, int64_t n, const T *t, const T *p, const T *qv, const T *qc,
                                  const T *nc, const T *qi, const T *ni, const T *qs, T *re_qc, T *re_qi, T *re_qs,
                                  hipStream_t s, const double *set_nc_col = nullptr, int64_t nz_col = 1, int64_t e0 = 0)
{
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (keep) hipLaunchKernelGGL((k_effective_radii<T, true>), grid, block, 0, s, n, c, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs, set_nc_col, nz_col, e0);
    else      hipLaunchKernelGGL((k_effective_radii<T, false>), grid, block, 0, s, n, c, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs, set_nc_col, nz_col, e0);
    return hipGetLastError();
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

template <class T> void kidmp::launch_default_aerosols(int64_t n, T Nt_c, const T *qv, const T *t, const T *p, T *nc, T *nwfa, T *nifa, hipStream_t s,
                                                       const double *set_nc_col, int64_t nz_col, int64_t e0)
{
    hipLaunchKernelGGL(k_default_aerosols<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, Nt_c, qv, t, p, nc, nwfa, nifa,
                       set_nc_col, nz_col > 0 ? nz_col : 1, e0);
}
template void kidmp::launch_default_aerosols<double>(int64_t, double, const double *, const double *, const double *, double *, double *, double *, hipStream_t,
                                                     const double *, int64_t, int64_t);
template void kidmp::launch_default_aerosols<float>(int64_t, float, const float *, const float *, const float *, float *, float *, float *, hipStream_t,
                                                    const double *, int64_t, int64_t);

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

// ---- the column outputs: what a host model takes from the state beside the step ----
// One check for the device entries and the host step.  Pairs: qi + ni, qs + qg, both or neither, neither only in an
// iiwarm context (they are zero there); the radii: re_qc with re_qi and re_qs, the latter two optional in an iiwarm
// context; nc only where the context is aerosol-aware (M:4863).
template <class T>
int kidmp::check_outputs_request(kidmp_ctx *ctx, const char *who, const ColumnOutputs<T> &out)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    const bool radii = out.re_qc || out.re_qi || out.re_qs, warm = ctx->cfg.iiwarm != 0;
    if (radii && !out.re_qc) return fail(ctx, KIDMP_EINVAL, w + ": re_qc, re_qi, re_qs must be requested together");
    if ((out.re_qi == nullptr) != (out.re_qs == nullptr) || (radii && !out.re_qi && !warm))
        return fail(ctx, KIDMP_EINVAL, w + ": re_qi and re_qs may be left out only together and only in an iiwarm context");
    if (out.dbz && !refl_consts_supported(ctx->hc)) return fail(ctx, KIDMP_ESTATE, w + ": reflectivity exponents differ from the kernel's");
    return KIDMP_OK;
}
template <class T>
int kidmp::check_outputs_args(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const ColumnState<T> &in,
                              const ColumnOutputs<T> &out)
{
    const std::string w(who);
    if (int rc = check_outputs_request<T>(ctx, who, out)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (int rc = check_nc_count(ctx, who, ncol)) return rc;
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    const bool radii = out.re_qc != nullptr, warm = ctx->cfg.iiwarm != 0;
    if (ncol == 0 || (!radii && !out.dbz)) return KIDMP_OK;
    if (!in.t || !in.p || !in.qv || (radii && !in.qc) || (out.dbz && (!in.qr || !in.nr)))
        return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if ((in.qi == nullptr) != (in.ni == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": qi and ni must be given or left out together");
    if ((in.qs == nullptr) != (in.qg == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": qs and qg must be given or left out together");
    if (!warm && ((radii && !in.qi) || !in.qs)) return fail(ctx, KIDMP_EINVAL, w + ": a mixed-phase context needs qi, ni, qs and qg");
    if (radii && ctx->cfg.is_aerosol_aware && !in.nc) return fail(ctx, KIDMP_EINVAL, w + ": an aerosol-aware context needs nc for the radii");
    return KIDMP_OK;
}

// One launch, chosen by what is wanted: the reflectivity alone, the radii alone (pointwise, preset form), or both from a
// single read of the column.  Arguments as checked above.
template <class T>
hipError_t kidmp::launch_outputs(kidmp_ctx *ctx, int64_t ncol, int nz, const ColumnState<T> &in, const ColumnOutputs<T> &out,
                                 hipStream_t s, int64_t nc_first)
{
    const bool aero = ctx->cfg.is_aerosol_aware != 0;
    const T *nc = aero ? in.nc : nullptr;
    const double *set_nc = ctx->d_nc_col ? ctx->d_nc_col + nc_first : nullptr;   // the batch's share of a bound droplet number
    if (out.dbz && out.re_qc) {
        ColumnState<T> st = in;
        st.nc = nc;
        return launch_column_outputs<T>(refl_consts(ctx->hc), rad_consts(ctx->hc, aero), ncol, nz, st, out, s, set_nc);
    }
    if (out.dbz) return launch_reflectivity<T>(refl_consts(ctx->hc), ncol, nz, in.t, in.p, in.qv, in.qr, in.nr, in.qs, in.qg, out.dbz, s);
    if (out.re_qc)
        return launch_effective_radii<T>(rad_consts(ctx->hc, aero), false, ncol * int64_t(nz), in.t, in.p, in.qv, in.qc, nc, in.qi,
                                         in.ni, in.qs, out.re_qc, out.re_qi, out.re_qs, s, set_nc, nz, 0);
    return hipSuccess;
}
#define KIDMP_INSTANTIATE_OUTPUTS(T) \
    template int kidmp::check_outputs_request<T>(kidmp_ctx *, const char *, const ColumnOutputs<T> &); \
    template int kidmp::check_outputs_args<T>(kidmp_ctx *, const char *, int64_t, int32_t, const ColumnState<T> &, const ColumnOutputs<T> &); \
    template hipError_t kidmp::launch_outputs<T>(kidmp_ctx *, int64_t, int, const ColumnState<T> &, const ColumnOutputs<T> &, hipStream_t, int64_t);
KIDMP_INSTANTIATE_OUTPUTS(double)
KIDMP_INSTANTIATE_OUTPUTS(float)
#undef KIDMP_INSTANTIATE_OUTPUTS

// calc_effectRad in the subroutine's own INOUT form on n = ncol*nz elements: the lenient compatibility entries
// (kidmp_effective_radii_host, kidmp32_effective_radii_*).  Null nc / qi + ni / qs as in check_outputs_args.
template <class T>
int kidmp::check_radii_args(kidmp_ctx *ctx, const char *who, int64_t n, const T *t, const T *p, const T *qv, const T *qc,
                            const T *nc, const T *qi, const T *ni, const T *qs, T *re_qc, T *re_qi, T *re_qs)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (n < 0) return fail(ctx, KIDMP_EINVAL, w + ": n < 0");
    if (n == 0) return KIDMP_OK;                                // an empty batch has nothing to point at
    const bool warm = ctx->cfg.iiwarm != 0;
    if (!t || !p || !qv || !qc || !re_qc) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if ((qi == nullptr) != (ni == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": qi and ni must be given or left out together");
    if (!warm && (!qi || !qs)) return fail(ctx, KIDMP_EINVAL, w + ": a mixed-phase context needs qi, ni and qs");
    if ((re_qi == nullptr) != (re_qs == nullptr) || (!re_qi && !warm))
        return fail(ctx, KIDMP_EINVAL, w + ": re_qi and re_qs may be left out only together and only in an iiwarm context");
    if (ctx->cfg.is_aerosol_aware && !nc) return fail(ctx, KIDMP_EINVAL, w + ": an aerosol-aware context needs nc");
    return KIDMP_OK;
}
template <class T>
hipError_t kidmp::launch_radii_keep(kidmp_ctx *ctx, int64_t n, const T *t, const T *p, const T *qv, const T *qc, const T *nc,
                                    const T *qi, const T *ni, const T *qs, T *re_qc, T *re_qi, T *re_qs, hipStream_t s,
                                    int64_t nz_col, int64_t e0)
{
    const bool aero = ctx->cfg.is_aerosol_aware != 0;
    return launch_effective_radii<T>(rad_consts(ctx->hc, aero), true, n, t, p, qv, qc, aero ? nc : nullptr, qi, ni, qs, re_qc,
                                     re_qi, re_qs, s, nz_col > 0 ? ctx->d_nc_col : nullptr, nz_col > 0 ? nz_col : 1, e0);
}
#define KIDMP_INSTANTIATE_RADII(T) \
    template int kidmp::check_radii_args<T>(kidmp_ctx *, const char *, int64_t, const T *, const T *, const T *, const T *, const T *, \
                                            const T *, const T *, const T *, T *, T *, T *); \
    template hipError_t kidmp::launch_radii_keep<T>(kidmp_ctx *, int64_t, const T *, const T *, const T *, const T *, const T *, \
                                                    const T *, const T *, const T *, T *, T *, T *, hipStream_t, int64_t, int64_t);
KIDMP_INSTANTIATE_RADII(double)
KIDMP_INSTANTIATE_RADII(float)
#undef KIDMP_INSTANTIATE_RADII

namespace {
template <class T, class O>
int column_outputs_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const ColumnState<T> &in, const O *o, void *stream)
{
    const ColumnOutputs<T> out = o ? ColumnOutputs<T>{o->dbz, o->re_qc, o->re_qi, o->re_qs} : ColumnOutputs<T>{};
    if (int rc = check_outputs_args<T>(ctx, who, ncol, nz, in, out)) return rc;
    if (ncol == 0 || (!out.dbz && !out.re_qc)) return KIDMP_OK;
    GUARD(ctx);
    const char *names[] = {"t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg", "dbz", "re_qc", "re_qi", "re_qs"};
    const void *ptrs[] = {in.t, in.p, in.qv, in.qc, in.nc, in.qi, in.ni, in.qr, in.nr, in.qs, in.qg, out.dbz, out.re_qc, out.re_qi, out.re_qs};
    for (int i = 0; i < 15; ++i)
        if (int rc = check_device_array(ctx, who, ptrs[i], names[i])) return rc;
    HIPTRY(ctx, launch_outputs<T>(ctx, ncol, nz, in, out, (hipStream_t)stream));
    return KIDMP_OK;
}
}  // namespace

extern "C" {
int kidmp_default_aerosols_device(kidmp_ctx *ctx, int64_t n, const double *qv, const double *t, const double *p,
                                  double *nc, double *nwfa, double *nifa, void *stream)
{
    if (int rc = require_ready(ctx)) return rc;
    if (n < 0 || !qv || !t || !p || !nc || !nwfa || !nifa) return fail(ctx, KIDMP_EINVAL, "kidmp_default_aerosols_device: bad argument");
    if (n == 0) return KIDMP_OK;
    int64_t nz_col = 0;
    if (int rc = nc_levels_of(ctx, "kidmp_default_aerosols_device", n, nz_col)) return rc;
    GUARD(ctx);
    if (int rc = check_on_device(ctx, qv, "qv")) return rc;
    if (int rc = check_on_device(ctx, nc, "nc")) return rc;
    launch_default_aerosols<double>(n, ctx->hc.Nt_c, qv, t, p, nc, nwfa, nifa, (hipStream_t)stream, nz_col ? ctx->d_nc_col : nullptr, nz_col);
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
    int64_t nz_col = 0;
    if (int rc = nc_levels_of(ctx, "kidmp_effective_radii_device", n, nz_col)) return rc;
    GUARD(ctx);
    if (int rc = check_on_device(ctx, t, "t")) return rc;
    if (int rc = check_on_device(ctx, re_qc, "re_qc")) return rc;
    HIPTRY(ctx, launch_radii_keep<double>(ctx, n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs, (hipStream_t)stream, nz_col));
    return KIDMP_OK;
}

int kidmp32_effective_radii_device(kidmp_ctx *ctx, int64_t n, const float *t, const float *p, const float *qv,
                                   const float *qc, const float *nc, const float *qi, const float *ni, const float *qs,
                                   float *re_qc, float *re_qi, float *re_qs, void *stream)
{
    if (int rc = check_radii_args<float>(ctx, "kidmp32_effective_radii_device", n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs)) return rc;
    if (n == 0) return KIDMP_OK;
    int64_t nz_col = 0;
    if (int rc = nc_levels_of(ctx, "kidmp32_effective_radii_device", n, nz_col)) return rc;
    GUARD(ctx);
    const char *names[] = {"t", "p", "qv", "qc", "nc", "qi", "ni", "qs", "re_qc", "re_qi", "re_qs"};
    const void *ptrs[] = {t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs};
    for (int i = 0; i < 11; ++i)
        if (int rc = check_device_array(ctx, "kidmp32_effective_radii_device", ptrs[i], names[i])) return rc;
    HIPTRY(ctx, launch_radii_keep<float>(ctx, n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs, (hipStream_t)stream, nz_col));
    return KIDMP_OK;
}

int kidmp_column_outputs_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                const double *qc, const double *nc, const double *qi, const double *ni, const double *qr,
                                const double *nr, const double *qs, const double *qg, const kidmp_outputs *out, void *stream)
{
    return column_outputs_device<double>(ctx, "kidmp_column_outputs_device", ncol, nz, {t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg}, out, stream);
}
int kidmp32_column_outputs_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                  const float *qc, const float *nc, const float *qi, const float *ni, const float *qr,
                                  const float *nr, const float *qs, const float *qg, const kidmp32_outputs *out, void *stream)
{
    return column_outputs_device<float>(ctx, "kidmp32_column_outputs_device", ncol, nz, {t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg}, out, stream);
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
