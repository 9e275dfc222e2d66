// thompson_reflectivity.hip -- calc_refl10cm (M:4946-5244) on gfx950: the 10-cm radar reflectivity the scheme's own size
// distributions give in the Rayleigh approximation, dBZ = 10 log10((ze_rain + ze_snow + ze_graupel) * 1e18) (M:5196).
//
// Only the live part of the reference is computed.  Dead as shipped: rc (qc1d is never read), rhof, smoc, the melting-level
// search k_0/melti (M:5107-5121) and the whole wet-snow/graupel block (M:5140-5192): with nrbins = 0 (M:204) its bin loops
// are empty and its ze_* assignments are commented out, so calc_refl10cm has no bright band; k_bright_band
// (kidmp_brightband.hip) is an entry of its own that rebuilds that block (include/kidmp_brightband.h).
//
// Layout: one wavefront per column, lanes over levels (kidmp_column.h, which holds the column body column_dbz: k_column_summary
// of kidmp_summary.hip calls it as well).  Every level is independent except the graupel intercept, which is a top-down
// running minimum over ALL levels of the column (M:5087-5103; levels without graupel enter it with rg = R1): a suffix
// minimum, formed with a wave scan -- DPP row shifts inside each row of 16 lanes, v_readlane for the three row totals, and
// the level groups chained from the top through a wave-uniform carry.
//
// Arithmetic: binary64 throughout (the reference's P64 build), the fastmath.h helpers the column kernel uses for log10,
// 10**x and x**y, and the same integer powers / roots for the exponents the scheme fixes (cube root for obmr = 1/3, two
// square roots for oge1 = 1/4, multiplies for cre(4) = cge(4) = 7).  Division is IEEE (this file is compiled without the
// column kernel's reciprocal-math flags).  Binary32 storage is widened on load and rounded once on store.
//
// k_column_outputs is the same column body with calc_effectRad (M:4834-4935) of every level formed beside it, in the
// form of the scheme's driver (presets first, M:1111-1116): re_qc, re_qi, re_qs and dbz from one read of the state.  The
// per-level arithmetic of both diagnostics is thompson_levels.h, shared with the pointwise k_effective_radii.
#include "thompson_reflectivity.h"

#include <cmath>
#include <type_traits>

#include "thompson_levels.h"
#include "kidmp_column.h"

namespace kidmp {

// what the fused instantiation takes beyond the reflectivity's own arguments; NoRadii selects the reflectivity alone
template <class T>
struct RadiiArgs {
    RadConsts c;
    const T *qc, *nc, *qi, *ni;                      // nc null: not aerosol-aware; qi, ni null: zero
    T *re_qc, *re_qi, *re_qs;                        // re_qi, re_qs null: not wanted (iiwarm)
    const double *set_nc_col;                        // null, or the per-column set_Nc of the batch (kidmp_set_column_nc)
};
struct NoRadii {};

namespace {

// calc_effectRad of one level in the driver's form (M:1111-1116): a level without the species receives the preset.  The
// driver's clamps after the call (M:1118-1120) change nothing after the subroutine's own and are not computed.
// calc_effectRad does not clamp qv (M:4860) where calc_refl10cm does (M:4992): below 1e-10 the radii get a density of
// their own, and only a level whose two densities are one shares the snow moment `sl` (valid when L_qs).
template <class T>
__device__ inline void radii_of_level(const ReflConsts &c, const RadiiArgs<T> &r, double Nt_c, int64_t i, double temp, double pres, double qv_in, double qv,
                                      double rho_z, double qs, bool L_qs, const lvl::SnowLevel &sl)
{
    const bool same = qv_in == qv;
    const double rho = same ? rho_z : lvl::air_density(pres, temp, qv_in);
    double re;
    re = lvl::RE_QC_PRESET;
    lvl::cloud_water_radius(r.c, Nt_c, rho, double(r.qc[i]), r.nc ? double(r.nc[i]) : 0., re);
    r.re_qc[i] = T(re);
    if (r.re_qi) {
        re = lvl::RE_QI_PRESET;
        if (r.qi) lvl::cloud_ice_radius(r.c, rho, double(r.qi[i]), double(r.ni[i]), re);
        r.re_qi[i] = T(re);
    }
    if (r.re_qs) {
        re = lvl::RE_QS_PRESET;
        const double rs = fmax(R1, qs * rho);
        if (!(rs <= R1)) re = lvl::snow_radius(c.sa, c.sb, r.c.cse1, L_qs && same ? sl : lvl::snow_level(temp, rs, c.oams));   // sa, sb, oams: one copy
        r.re_qs[i] = T(re);
    }
}

// One wavefront per column: the body of k_reflectivity and, with RAD = RadiiArgs<T>, of k_column_outputs.
template <class T, int NJ, class RAD>
__device__ __forceinline__ void column_diagnostics(const ReflConsts &c, const RAD &rad, int64_t ncol, int nz,
                                                   const T *__restrict__ t1d, const T *__restrict__ p1d,
                                                   const T *__restrict__ qv1d, const T *__restrict__ qr1d,
                                                   const T *__restrict__ nr1d, const T *__restrict__ qs1d,
                                                   const T *__restrict__ qg1d, T *__restrict__ dbz)
{
    constexpr bool RADII = !std::is_same<RAD, NoRadii>::value;
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    double Nt_c = 0.;                                                // the column's droplet number (radii only)
    if constexpr (RADII) Nt_c = rad.set_nc_col ? rad.set_nc_col[col] * 1.e6 : rad.c.Nt_c;

    double d[NJ];
    column_dbz<T, NJ>(c, nz, lane, base, t1d, p1d, qv1d, qr1d, nr1d, qs1d, qg1d, d,
                      [&](int, int64_t i, double temp, double pres, double qv_in, double qv, double rho, double qs, bool L_qs,
                          const lvl::SnowLevel &sl) __attribute__((always_inline)) {
                          if constexpr (RADII) radii_of_level<T>(c, rad, Nt_c, i, temp, pres, qv_in, qv, rho, qs, L_qs, sl);
                      });
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        if (k < nz) dbz[base + k] = T(d[j]);
    }
}

}  // namespace

// the reflectivity alone; the kernel name rocprofv3 lists is kidmp::k_reflectivity<T, NJ>
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_reflectivity(ReflConsts c, int64_t ncol, int nz, const T *__restrict__ t1d, const T *__restrict__ p1d,
               const T *__restrict__ qv1d, const T *__restrict__ qr1d, const T *__restrict__ nr1d,
               const T *__restrict__ qs1d, const T *__restrict__ qg1d, T *__restrict__ dbz)
{
    column_diagnostics<T, NJ, NoRadii>(c, NoRadii{}, ncol, nz, t1d, p1d, qv1d, qr1d, nr1d, qs1d, qg1d, dbz);
}

// radii and reflectivity of a column from one read of its state (kidmp::k_column_outputs<T, NJ>)
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_column_outputs(ReflConsts c, RadiiArgs<T> rad, int64_t ncol, int nz, const T *__restrict__ t1d,
                 const T *__restrict__ p1d, const T *__restrict__ qv1d, const T *__restrict__ qr1d,
                 const T *__restrict__ nr1d, const T *__restrict__ qs1d, const T *__restrict__ qg1d, T *__restrict__ dbz)
{
    column_diagnostics<T, NJ, RadiiArgs<T>>(c, rad, ncol, nz, t1d, p1d, qv1d, qr1d, nr1d, qs1d, qg1d, dbz);
}

namespace {

// rad null: k_reflectivity; else k_column_outputs
template <class T>
hipError_t launch_any(const ReflConsts &c, const RadiiArgs<T> *rad, int64_t ncol, int nz, const T *t, const T *p,
                      const T *qv, const T *qr, const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t s)
{
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        if (rad)
            hipLaunchKernelGGL((k_column_outputs<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, *rad, ncol, nz, t,
                               p, qv, qr, nr, qs, qg, dbz);
        else
            hipLaunchKernelGGL((k_reflectivity<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, ncol, nz, t, p, qv,
                               qr, nr, qs, qg, dbz);
    });
}

}  // namespace

bool doppler_consts_supported(const Consts &hc)
{
    // beyond refl_consts_supported: n = 7 + mu_r = 7 + mu_g = 7 and bv_r = 1 (rain's integer powers), n = 2 bm_s + 1 = 5 and
    // cse(1) = bm_s + 1 (snow)
    return refl_consts_supported(hc) && mu_r == 0.0 && mu_g == 0.0 && bv_r == 1.0 && bm_s == 2.0 && hc.cse[0] == 3.;
}

DopplerConsts doppler_consts(const Consts &hc)
{
    DopplerConsts d{};
    const double nr_ = 7. + mu_r, ng_ = 7. + mu_g, ns_ = 2. * bm_s + 1.;
    d.cse1 = hc.cse[0];
    d.gr1 = std::tgamma(nr_ + bv_r) / std::tgamma(nr_);
    d.gr2 = std::tgamma(nr_ + 2. * bv_r) / std::tgamma(nr_);
    d.gg1 = std::tgamma(ng_ + bv_g) / std::tgamma(ng_);
    d.gg2 = std::tgamma(ng_ + 2. * bv_g) / std::tgamma(ng_);
    d.ks0_1 = Kap0 * std::tgamma(ns_ + bv_s);
    d.ks1_1 = Kap1 * std::tgamma(ns_ + mu_s + bv_s);
    d.ks0_2 = Kap0 * std::tgamma(ns_ + 2. * bv_s);
    d.ks1_2 = Kap1 * std::tgamma(ns_ + mu_s + 2. * bv_s);
    d.ia00 = 1. / (Kap0 * std::tgamma(ns_) * std::pow(Lam0, -ns_) + Kap1 * std::tgamma(ns_ + mu_s) * std::pow(Lam1, -(ns_ + mu_s)));
    return d;
}

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

RadConsts rad_consts(const Consts &hc, bool aerosol_aware)
{
    RadConsts c{};
    c.aero = aerosol_aware;
    c.Nt_c = hc.Nt_c; c.cig2 = hc.cig[1]; c.oig1 = hc.oig1; c.oams = hc.oams; c.cse1 = hc.cse[0];
    for (int i = 0; i < 10; ++i) { c.sa[i] = hc.sa[i]; c.sb[i] = hc.sb[i]; }
    return c;
}

template <class T>
hipError_t launch_reflectivity(const ReflConsts &c, int64_t ncol, int nz, const T *t, const T *p, const T *qv,
                               const T *qr, const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t s)
{
    return launch_any<T>(c, nullptr, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
}

template <class T>
hipError_t launch_column_outputs(const ReflConsts &c, const RadConsts &rc, int64_t ncol, int nz, const ColumnState<T> &in,
                                 const ColumnOutputs<T> &out, hipStream_t s, const double *set_nc_col)
{
    const RadiiArgs<T> rad{rc, in.qc, in.nc, in.qi, in.ni, out.re_qc, out.re_qi, out.re_qs, set_nc_col};
    return launch_any<T>(c, &rad, ncol, nz, in.t, in.p, in.qv, in.qr, in.nr, in.qs, in.qg, out.dbz, s);
}

template hipError_t launch_reflectivity<double>(const ReflConsts &, int64_t, int, const double *, const double *,
                                                const double *, const double *, const double *, const double *,
                                                const double *, double *, hipStream_t);
template hipError_t launch_reflectivity<float>(const ReflConsts &, int64_t, int, const float *, const float *,
                                               const float *, const float *, const float *, const float *,
                                               const float *, float *, hipStream_t);
template hipError_t launch_column_outputs<double>(const ReflConsts &, const RadConsts &, int64_t, int,
                                                  const ColumnState<double> &, const ColumnOutputs<double> &, hipStream_t, const double *);
template hipError_t launch_column_outputs<float>(const ReflConsts &, const RadConsts &, int64_t, int,
                                                 const ColumnState<float> &, const ColumnOutputs<float> &, hipStream_t, const double *);

}  // namespace kidmp
