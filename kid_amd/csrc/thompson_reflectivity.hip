// thompson_reflectivity.hip -- calc_refl10cm (M:4946-5244) on gfx950: the 10-cm radar reflectivity the scheme's own size
// distributions give in the Rayleigh approximation, dBZ = 10 log10((ze_rain + ze_snow + ze_graupel) * 1e18) (M:5196).
//
// Only the live part of the reference is computed.  Dead as shipped: rc (qc1d is never read), rhof, smoc, the melting-level
// search k_0/melti (M:5107-5121) and the whole wet-snow/graupel block (M:5140-5192): with nrbins = 0 (M:204) its bin loops
// are empty and its ze_* assignments are commented out, so there is no bright band and none is added here.
//
// Layout: one wavefront per column (four per workgroup), lanes over levels: level k = 64 j + lane in level group j,
// NJ = ceil(nz/64) groups per lane.  Every level is independent except the graupel intercept, which is a top-down running
// minimum over ALL levels of the column (M:5087-5103; levels without graupel enter it with rg = R1): a suffix minimum,
// formed here with a wave scan -- DPP row shifts inside each row of 16 lanes, v_readlane for the three row totals, and the
// level groups chained from the top through a wave-uniform carry.
//
// Arithmetic: binary64 throughout (the reference's P64 build), the fastmath.h helpers the column kernel uses for log10,
// 10**x and x**y, and the same integer powers / roots for the exponents the scheme fixes (cube root for obmr = 1/3, two
// square roots for oge1 = 1/4, multiplies for cre(4) = cge(4) = 7).  Division is IEEE (this file is compiled without the
// column kernel's reciprocal-math flags).  Binary32 storage is widened on load and rounded once on store.
#include "thompson_reflectivity.h"

#include "fastmath.h"

namespace kidmp {
namespace {

constexpr int REFL_WAVES = 4;                        // columns (wavefronts) per workgroup
constexpr int REFL_THREADS = 64 * REFL_WAVES;

// (0.176/0.93) * (6.0/PI)*(6.0/PI) * (am/900.0)*(am/900.0), M:5131-5135, evaluated left to right as the reference does
constexpr double ZE_ICE_FAC = (0.176 / 0.93) * (6.0 / PI) * (6.0 / PI);
constexpr double ZE_SNOW_FAC = ZE_ICE_FAC * (am_s / 900.0) * (am_s / 900.0);
constexpr double ZE_GRAUPEL_FAC = ZE_ICE_FAC * (am_g / 900.0) * (am_g / 900.0);
constexpr double MVD_FAC = 3.0 + mu_r + 0.672;       // M:5004

__device__ inline double pw7(double x) { const double s = x * x; return s * s * s * x; }

// cube root of a positive, finite x.  fm::cbrt_pos covers [1e-37, 1e37] (its seed is taken in binary32); the rain slope's
// argument am_r*crg(3)*org2*nr/rr is unclamped here, as in the reference (M:5001), and leaves that range when nr/rr is
// huge (qr just above R1 with a very large nr).  Outside [1e-36, 1e36] the argument is first scaled into range by an
// exact power of two 2**(-3q) and the root scaled back by 2**q.
__device__ inline double cbrt_any(double x)
{
    if (x >= 1.E-36 && x <= 1.E36) return fm::cbrt_pos(x);
    const int q = ilogb(x) / 3;
    return fm::cbrt_pos(ldexp(x, -3 * q)) * ldexp(1., q);
}

// the Field et al. (2005) fit of M:5066-5080 at x = cse(3): a_ = 10**loga_, moment = a_ * smo2**b_
__device__ inline double snow_moment_z(const ReflConsts &c, double tc0, double smo2)
{
    const double x = c.cse3;
    const double *a = c.sa, *b = c.sb;
    const double loga_ = a[0] + a[1] * tc0 + a[2] * x + a[3] * tc0 * x + a[4] * tc0 * tc0 + a[5] * x * x
                       + a[6] * tc0 * tc0 * x + a[7] * tc0 * x * x + a[8] * tc0 * tc0 * tc0 + a[9] * x * x * x;
    const double b_ = b[0] + b[1] * tc0 + b[2] * x + b[3] * tc0 * x + b[4] * tc0 * tc0 + b[5] * x * x
                    + b[6] * tc0 * tc0 * x + b[7] * tc0 * x * x + b[8] * tc0 * tc0 * tc0 + b[9] * x * x * x;
    return fm::pow10_times_pow(loga_, fm::log2_parts(smo2), b_);
}

// graupel intercept of one level before the running minimum, M:5088-5096 (clamped to [gonv_min, gonv_max])
__device__ inline double graupel_n0_exp(bool slw, double mvd_r, double rg)
{
    const double xslw1 = slw ? 4.01 + fm::log10(mvd_r) : 0.01;
    const double ygra1 = 4.31 + fm::log10(fmax(5.E-5, rg));
    const double zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1));
    const double n0 = fm::exp10(zans1);
    return fmax(gonv_min, fmin(n0, gonv_max));
}

// 64-bit DPP move: lane l receives lane l + D of its row of 16 (row_shl:D); lanes whose source lies past the row end get
// garbage that the caller masks off
template <int D>
__device__ inline double row_shl(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, int(b & 0xffffffffll), 0x100 + D, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, int(b >> 32), 0x100 + D, 0xf, 0xf, false);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}
__device__ inline double readlane(double v, int lane)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(int(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane(int(b >> 32), lane);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

// suffix minimum over the wave: lane l receives min(v[l], v[l+1], ..., v[63]); `tail` receives the minimum of the whole
// wave (lane 0's result), wave-uniform
__device__ inline double wave_suffix_min(double v, int lane, double &tail)
{
    const int r = lane & 15;
    { const double o = row_shl<1>(v); if (r + 1 < 16) v = fmin(v, o); }
    { const double o = row_shl<2>(v); if (r + 2 < 16) v = fmin(v, o); }
    { const double o = row_shl<4>(v); if (r + 4 < 16) v = fmin(v, o); }
    { const double o = row_shl<8>(v); if (r + 8 < 16) v = fmin(v, o); }
    // v = suffix minimum within the row; lane 16 q holds the minimum of row q
    const double m1 = readlane(v, 16), m2 = readlane(v, 32), m3 = readlane(v, 48);
    const double a3 = m3, a2 = fmin(m2, a3), a1 = fmin(m1, a2);          // minima of rows q+1 .. 3
    const int q = lane >> 4;
    const double above = q == 0 ? a1 : q == 1 ? a2 : q == 2 ? a3 : double(__builtin_inf());
    v = fmin(v, above);
    tail = readlane(v, 0);
    return v;
}

}  // namespace

// one wavefront per column; the kernel name rocprofv3 lists is kidmp::k_reflectivity<T, NJ>
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_reflectivity(ReflConsts c, int64_t ncol, int nz, const T *__restrict__ t1d, const T *__restrict__ p1d,
               const T *__restrict__ qv1d, const T *__restrict__ qr1d, const T *__restrict__ nr1d,
               const T *__restrict__ qs1d, const T *__restrict__ qg1d, T *__restrict__ dbz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);            // log10 / 10**x / x**y read their tables from LDS
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scan needs every lane
    const int64_t base = col * int64_t(nz);

    double ze_rs[NJ], n0[NJ], rg[NJ];
    bool lqg[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        const bool in = k < nz;
        ze_rs[j] = 0.;
        rg[j] = R1;
        lqg[j] = false;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (!in) continue;
        const int64_t i = base + k;
        // ---- load, M:4991-5028 ----
        const double temp = double(t1d[i]);
        const double qv = fmax(1.E-10, double(qv1d[i]));
        const double pres = double(p1d[i]);
        const double rho = 0.622 * pres / (Rgas * temp * (qv + 0.622));
        const double qr = double(qr1d[i]);
        const double qs = qs1d ? double(qs1d[i]) : 0.;
        const double qg = qg1d ? double(qg1d[i]) : 0.;
        const bool L_qr = qr > R1, L_qs = qs > R2;
        lqg[j] = qg > R2;
        double ze_rain = 1.E-22, ze_snow = 1.E-22, mvd_r = 50.E-6;
        if (L_qr) {                                                  // no 37.5 um / 2.5 mm limits here (cf. M:1661-1666)
            const double rr = qr * rho;
            const double nr = fmax(R2, double(nr1d[i]) * rho);
            const double lamr = cbrt_any(am_r * c.crg3 * c.org2 * nr / rr);       // **obmr
            const double ilamr = 1. / lamr;
            const double N0_r = nr * c.org2 * lamr;                               // lamr**cre(2), cre(2) = 1
            mvd_r = MVD_FAC * ilamr;
            ze_rain = N0_r * c.crg4 * pw7(ilamr);                                  // ilamr**cre(4), M:5130
        }
        if (L_qs) {                                                  // bm_s = 2: smo2 = smob = rs*oams, M:5033-5038
            const double tc0 = fmin(-0.1, temp - 273.15);
            const double smo2 = qs * rho * c.oams;
            ze_snow = ZE_SNOW_FAC * snow_moment_z(c, tc0, smo2);                   // M:5131-5132
        }
        if (lqg[j]) rg[j] = qg * rho;
        ze_rs[j] = ze_rain + ze_snow;
        // ---- graupel intercept before the running minimum, M:5088-5096 ----
        n0[j] = graupel_n0_exp(temp < 270.65 && L_qr && mvd_r > 100.E-6, mvd_r, rg[j]);
    }

    // ---- N0_min = MIN(N0_exp, N0_min) from kte down to kts (M:5097-5098): a suffix minimum over the levels ----
    double carry = gonv_max;                                         // N0_min = gonv_max, M:5086
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {
        double tail;
        const double s = wave_suffix_min(n0[j], lane, tail);
        n0[j] = fmin(s, carry);
        carry = fmin(carry, tail);
    }

#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        if (k >= nz) continue;
        double ze_graupel = 1.E-22;
        if (lqg[j]) {                                                // M:5099-5102, M:5133-5135
            const double N0_exp = n0[j];
            const double lam_exp = fm::sqrt_pos(fm::sqrt_pos(N0_exp * am_g * c.cgg1 / rg[j]));   // **oge1
            const double lamg = lam_exp * c.lamg_fac;
            const double ilamg = 1. / lamg;
            const double N0_g = N0_exp / (c.cgg2 * lam_exp) * lamg;                            // lamg**cge(2), cge(2) = 1
            ze_graupel = ZE_GRAUPEL_FAC * N0_g * c.cgg4 * pw7(ilamg);                          // ilamg**cge(4)
        }
        dbz[base + k] = T(10. * fm::log10((ze_rs[j] + ze_graupel) * 1.E18));                    // M:5196
    }
}

namespace {

template <class T, int NJ>
hipError_t launch_nj(const ReflConsts &c, int64_t ncol, int nz, const T *t, const T *p, const T *qv, const T *qr,
                     const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t s)
{
    const int64_t nblk = (ncol + REFL_WAVES - 1) / REFL_WAVES;
    hipLaunchKernelGGL((k_reflectivity<T, NJ>), dim3((unsigned)nblk), dim3(REFL_THREADS), 0, s, c, ncol, nz, t, p, qv,
                       qr, nr, qs, qg, dbz);
    return hipGetLastError();
}

}  // namespace

bool refl_consts_supported(const Consts &hc)
{
    // the exponents the kernel takes as roots and integer powers (thompson_init, M:452-553, from bm_*, mu_*)
    return hc.obmr == 1. / 3. && hc.oge1 == 0.25 && hc.cre[1] == 1. && hc.cre[3] == 7. && hc.cge[1] == 1.
           && hc.cge[3] == 7. && bm_s == 2.0;
}

ReflConsts refl_consts(const Consts &hc)
{
    ReflConsts c{};
    c.crg3 = hc.crg[2]; c.crg4 = hc.crg[3]; c.org2 = hc.org2;
    c.cse3 = hc.cse[2]; c.oams = hc.oams;
    for (int i = 0; i < 10; ++i) { c.sa[i] = hc.sa[i]; c.sb[i] = hc.sb[i]; }
    c.cgg1 = hc.cgg[0]; c.cgg2 = hc.cgg[1]; c.cgg4 = hc.cgg[3]; c.lamg_fac = hc.lamg_fac;
    return c;
}

template <class T>
hipError_t launch_reflectivity(const ReflConsts &c, int64_t ncol, int nz, const T *t, const T *p, const T *qv,
                               const T *qr, const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    switch ((nz + 63) / 64) {
    case 1: return launch_nj<T, 1>(c, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    case 2: return launch_nj<T, 2>(c, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    case 3: return launch_nj<T, 3>(c, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    case 4: return launch_nj<T, 4>(c, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    default: return hipErrorInvalidValue;
    }
}

template hipError_t launch_reflectivity<double>(const ReflConsts &, int64_t, int, const double *, const double *,
                                                const double *, const double *, const double *, const double *,
                                                const double *, double *, hipStream_t);
template hipError_t launch_reflectivity<float>(const ReflConsts &, int64_t, int, const float *, const float *,
                                               const float *, const float *, const float *, const float *,
                                               const float *, float *, hipStream_t);

}  // namespace kidmp
