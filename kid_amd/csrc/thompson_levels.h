// thompson_levels.h -- the per-level arithmetic of the column diagnostics, calc_effectRad (M:4834-4935), calc_refl10cm
// (M:4946-5244), the fall speeds of block O (M:3206-3354) and the Doppler moments of a vertically pointing radar
// (include/kidmp_doppler.h), as __device__ functions: the pointwise radii kernel
// (kidmp_diag.hip) and the wave-per-column kernels (kidmp_column.h and the units that include it) are built from these,
// so no statement exists twice.
//
// What the two diagnostics share at a level -- rho, the snow content rs = qs*rho, tc0, the snow moment smob = rs*oams and
// its logarithm -- is held in SnowLevel and formed once when both are wanted.
#pragma once
#include <hip/hip_runtime.h>

#include "thompson_params.h"
#include "fastmath.h"

namespace kidmp {

// the values of thompson_init (M:442-602) the live part of calc_refl10cm reads, taken from the context's Consts
struct ReflConsts {
    double crg3, crg4, org2;           // rain: crg(3), crg(4), org2   (obmr = 1/3: cube root; cre(2) = 1, cre(4) = 7)
    double cse3, oams, sa[10], sb[10]; // snow: the Field et al. fit at the bm_s*2 moment (cse(3)); bm_s = 2: smo2 = smob
    double cgg1, cgg2, cgg4, lamg_fac; // graupel: cgg(1), cgg(2), cgg(4), (cgg(3)*ogg2*ogg1)**obmg   (oge1 = 1/4;
                                       //          cge(2) = 1, cge(4) = 7)
};
// what calc_effectRad reads beyond oams, sa, sb: Nt_c (M:4863), cig(2), oig1 (M:4890), cse(1) (M:4920-4929)
struct RadConsts { double Nt_c, cig2, oig1, oams, cse1, sa[10], sb[10]; int aero; };
// what block O (M:3206-3354) and the load it follows (M:1420-1467) read; crg6 is crg(6) and so on
struct FallConsts {
    double crg2, crg3, crg6, crg7, crg12, org2, org3;           // rain
    double cie2, cig1, cig2, cig3, cig6, cig7, oig1, oig2;      // cloud ice
    double cse1, cse4, cse7, cse10, csg1, csg4, csg7, csg10, oams, sa[10], sb[10];   // snow
    double cgg1, cgg6, ogg3, lamg_fac;                          // graupel: lamg_fac = (cgg(3)*ogg2*ogg1)**obmg
};

// the gamma ratios of the Doppler moments (include/kidmp_doppler.h), which are not among thompson_init's c?g arrays:
// formed on the host with tgamma from thompson_params.h (doppler_consts)
struct DopplerConsts {
    double cse1;                       // snow: the order of smoc, cse(1)
    double gr1, gr2;                   // rain: Gamma(n+bv_r)/Gamma(n), Gamma(n+2bv_r)/Gamma(n), n = 7+mu_r
    double gg1, gg2;                   // graupel: the same with bv_g, n = 7+mu_g
    double ks0_1, ks1_1, ks0_2, ks1_2; // snow: Kap0 Gamma(5+b), Kap1 Gamma(5+mu_s+b) at b = bv_s and at b = 2 bv_s
    double ia00;                       // snow: 1/(Kap0 Gamma(5) Lam0**-5 + Kap1 Gamma(5+mu_s) Lam1**-(5+mu_s))
};

namespace lvl {

// the presets of the scheme's 3-D driver, M:1111-1113
constexpr double RE_QC_PRESET = 2.49E-6, RE_QI_PRESET = 4.99E-6, RE_QS_PRESET = 9.99E-6;

// M:4860 / M:4994
__device__ inline double air_density(double pres, double temp, double qv) { return 0.622 * pres / (Rgas * temp * (qv + 0.622)); }

// the Field et al. (2005) moment fit (M:4920-4930, M:5066-5080) at order x: a_ * smob**b_ with a_ = 10**loga_
struct SnowLevel { double tc0, smob; fm::Log2Parts l2; };
__device__ inline SnowLevel snow_level(double temp, double rs, double oams)
{
    SnowLevel s;
    s.tc0 = fmin(-0.1, temp - 273.15);
    s.smob = rs * oams;                                                 // bm_s = 2: smo2 = smob
    s.l2 = fm::log2_parts(s.smob);
    return s;
}
__device__ inline double snow_moment(const double *a, const double *b, double x, const SnowLevel &s)
{
    const double tc0 = s.tc0;
    const double loga_ = a[0] + a[1] * tc0 + a[2] * x + a[3] * tc0 * x + a[4] * tc0 * tc0 + a[5] * x * x
                       + a[6] * tc0 * tc0 * x + a[7] * tc0 * x * x + a[8] * tc0 * tc0 * tc0 + a[9] * x * x * x;
    const double b_ = b[0] + b[1] * tc0 + b[2] * x + b[3] * tc0 * x + b[4] * tc0 * tc0 + b[5] * x * x
                    + b[6] * tc0 * tc0 * x + b[7] * tc0 * x * x + b[8] * tc0 * tc0 * tc0 + b[9] * x * x * x;
    return fm::pow10_times_pow(loga_, s.l2, b_);
}

// nu_c = MIN(15, NINT(1000.E6/nc) + 2) (M:1400, M:1690, M:4876-4880) of a positive nc, without forming an integer out of range
__device__ inline int cloud_nu_c(double nc)
{
    if (nc < 100.) return 15;
    if (nc > 1.E10) return 2;
    const int inu_c = int(lround(1000.E6 / nc)) + 2;
    return inu_c < 15 ? inu_c : 15;
}

// ---- calc_effectRad at one level.  Each function reports whether the level holds the species (the reference CYCLEs
// otherwise, M:4874 / 4889 / 4897) and, if so, returns the radius in `re`. ----
// Nt_c: c.Nt_c, or the column's own where a per-column droplet number is bound (kidmp_set_column_nc)
__device__ inline bool cloud_water_radius(const RadConsts &c, double Nt_c, double rho, double qc, double nc1, double &re)
{
    const double am_r_ = PI * rho_w / 6.0;
    const double rc = fmax(R1, qc * rho);
    const double nc = c.aero ? fmax(R2, nc1 * rho) : Nt_c;              // .NOT. is_aerosol_aware, M:4863
    if (rc <= R1 || nc <= R2) return false;                             // M:4873-4884
    const int inu_c = cloud_nu_c(nc);
    const double g_ratio = double((inu_c + 1) * (inu_c + 2) * (inu_c + 3));   // 24, 60, 120 ... 4896 = (n+1)(n+2)(n+3)
    const double lamc = fm::cbrt_pos(nc * am_r_ * g_ratio / rc);
    re = fmax(2.51E-6, fmin(0.5 * double(3. + inu_c) / lamc, 50.E-6));
    return true;
}
__device__ inline bool cloud_ice_radius(const RadConsts &c, double rho, double qi, double ni1, double &re)
{
    const double am_i_ = PI * rho_i / 6.0;
    const double ri = fmax(R1, qi * rho), ni = fmax(R2, ni1 * rho);
    if (ri <= R1 || ni <= R2) return false;                             // M:4887-4893
    const double lami = fm::cbrt_pos(am_i_ * c.cig2 * c.oig1 * ni / ri);
    re = fmax(5.01E-6, fmin(0.5 * double(3. + mu_i) / lami, 125.E-6));
    return true;
}
// rs = MAX(R1, qs*rho) > R1, s = snow_level(temp, rs, oams); M:4896-4930
__device__ inline double snow_radius(const double *sa, const double *sb, double cse1, const SnowLevel &s)
{
    const double smoc = snow_moment(sa, sb, cse1, s);
    return fmax(10.E-6, fmin(0.5 * (smoc / s.smob), 999.E-6));
}

// ---- calc_refl10cm at one level ----
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

// rain of a level with qr > R1: ze_rain, the median volume diameter and the slope; no 37.5 um / 2.5 mm limits here
// (cf. M:1661-1666)
__device__ inline double rain_ze(const ReflConsts &c, double rho, double qr, double nr1, double &mvd_r, double &lamr, double &N0_r)
{
    const double rr = qr * rho;
    const double nr = fmax(R2, nr1 * rho);
    lamr = cbrt_any(am_r * c.crg3 * c.org2 * nr / rr);                    // **obmr
    const double ilamr = 1. / lamr;
    N0_r = nr * c.org2 * lamr;                                            // lamr**cre(2), cre(2) = 1
    mvd_r = MVD_FAC * ilamr;
    return N0_r * c.crg4 * pw7(ilamr);                                    // ilamr**cre(4), M:5130
}
__device__ inline double rain_ze(const ReflConsts &c, double rho, double qr, double nr1, double &mvd_r, double &lamr)
{
    double N0_r;
    return rain_ze(c, rho, qr, nr1, mvd_r, lamr, N0_r);
}
__device__ inline double rain_ze(const ReflConsts &c, double rho, double qr, double nr1, double &mvd_r)
{
    double lamr;
    return rain_ze(c, rho, qr, nr1, mvd_r, lamr);
}
// snow of a level with qs > R2, M:5033-5038 and M:5131-5132
__device__ inline double snow_ze(const ReflConsts &c, const SnowLevel &s) { return ZE_SNOW_FAC * snow_moment(c.sa, c.sb, c.cse3, s); }

// graupel intercept of one level before the running minimum, M:5088-5096 (clamped to [gonv_min, gonv_max])
__device__ inline double graupel_n0_exp(bool slw, double mvd_r, double rg)
{
    const double xslw1 = slw ? 4.01 + fm::log10(mvd_r) : 0.01;
    const double ygra1 = 4.31 + fm::log10(fmax(5.E-5, rg));
    const double zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1));
    const double n0 = fm::exp10(zans1);
    return fmax(gonv_min, fmin(n0, gonv_max));
}
// graupel of a level with qg > R2 once the running minimum N0_exp is known, M:5099-5102 and M:5133-5135; ilamg goes out too
__device__ inline double graupel_ze(const ReflConsts &c, double N0_exp, double rg, double &ilamg, double &lamg, double &N0_g)
{
    const double lam_exp = fm::sqrt_pos(fm::sqrt_pos(N0_exp * am_g * c.cgg1 / rg));    // **oge1
    lamg = lam_exp * c.lamg_fac;
    ilamg = 1. / lamg;
    N0_g = N0_exp / (c.cgg2 * lam_exp) * lamg;                                          // lamg**cge(2), cge(2) = 1
    return ZE_GRAUPEL_FAC * N0_g * c.cgg4 * pw7(ilamg);                                 // ilamg**cge(4)
}
__device__ inline double graupel_ze(const ReflConsts &c, double N0_exp, double rg, double &ilamg)
{
    double lamg, N0_g;
    return graupel_ze(c, N0_exp, rg, ilamg, lamg, N0_g);
}
__device__ inline double graupel_ze(const ReflConsts &c, double N0_exp, double rg)
{
    double ilamg;
    return graupel_ze(c, N0_exp, rg, ilamg);
}
__device__ inline double dbz_of(double ze) { return 10. * fm::log10(ze * 1.E18); }     // M:5196

// ---- block O (M:3206-3354) at one level: the fall speeds of a state as mp_thompson loads it (M:1387-1493).  The
// exponents the scheme fixes are taken as roots and integer powers (fall_consts_supported): obmr = obmi = 1/3,
// bm_i = bm_r = 3, cre(3) = 4, cre(6) = 5, cre(12) = 2.5, cre(7) = 3.5, bv_i = 1, cse(1) = 3, oge1 = 1/4. ----
__device__ inline double cube(double x) { return x * x * x; }
constexpr double XDI_FAC = bm_i + mu_i + 1.;          // M:1431

// rain as loaded, M:1447-1474: rr, the limited nr, the limited median volume diameter and the slope block O forms
// from them (M:3222).  A level without rain: rr = R1, nr = R2, has = false; mvd and lamr are not read.
struct RainLoad { double rr, nr, mvd, lamr; bool has; };
__device__ inline double nr_of_mvd(const FallConsts &c, double rr, double mvd)
{
    const double lamr = MVD_FAC / mvd;
    return c.crg2 * c.org3 * rr * cube(lamr) / am_r;                       // lamr**bm_r
}
__device__ inline double rain_slope(const FallConsts &c, double rr, double nr) { return cbrt_any(am_r * c.crg3 * c.org2 * nr / rr); }
__device__ inline RainLoad rain_load(const FallConsts &c, double rho, double qr, double nr1)
{
    RainLoad r{R1, R2, 0., 0., qr > R1};
    if (!r.has) return r;
    r.rr = qr * rho;
    r.nr = fmax(R2, nr1 * rho);
    if (r.nr <= R2) r.nr = nr_of_mvd(c, r.rr, 1.0E-3);
    r.lamr = rain_slope(c, r.rr, r.nr);
    r.mvd = MVD_FAC / r.lamr;
    if (r.mvd > 2.5E-3) r.mvd = 2.5E-3;
    else if (r.mvd < D0r * 0.75) r.mvd = D0r * 0.75;
    else return r;
    r.nr = nr_of_mvd(c, r.rr, r.mvd);
    r.lamr = rain_slope(c, r.rr, r.nr);                                    // M:3222 on the limited number
    return r;
}
// M:3223-3233
__device__ inline void rain_fall_speeds(const FallConsts &c, double rhof, double lamr, double &vtr, double &vtnr)
{
    const double s = lamr + fv_r, l2 = lamr * lamr, s2 = s * s;
    vtr = rhof * av_r * c.crg6 * c.org3 * (l2 * l2) * (1. / (s2 * s2 * s));                                    // **cre(3), **(-cre(6))
    vtnr = rhof * av_r * c.crg7 / c.crg12 * (l2 * fm::sqrt_pos(lamr)) * (1. / (s2 * s * fm::sqrt_pos(s)));    // **cre(12), **(-cre(7))
}

// cloud ice as loaded, M:1420-1445, and its slope in block O (M:3257)
struct IceLoad { double ri, ni, lami; bool has; };
__device__ inline double ice_slope(const FallConsts &c, double ri, double ni) { return cbrt_any(am_i * c.cig2 * c.oig1 * ni / ri); }
__device__ inline double ni_of_slope(const FallConsts &c, double ri, double lami) { return c.cig1 * c.oig2 * ri / am_i * cube(lami); }
__device__ inline IceLoad ice_load(const FallConsts &c, double rho, double qi, double ni1)
{
    IceLoad r{R1, R2, 0., qi > R1};
    if (!r.has) return r;
    r.ri = qi * rho;
    r.ni = fmax(R2, ni1 * rho);
    if (r.ni <= R2) r.ni = fmin(499.E3, ni_of_slope(c, r.ri, c.cie2 / 25.E-6));
    r.lami = ice_slope(c, r.ri, r.ni);
    const double xDi = XDI_FAC * (1. / r.lami);
    if (xDi < 5.E-6) r.ni = fmin(499.E3, ni_of_slope(c, r.ri, c.cie2 / 5.E-6));
    else if (xDi > 300.E-6) r.ni = ni_of_slope(c, r.ri, c.cie2 / 300.E-6);
    else return r;
    r.lami = ice_slope(c, r.ri, r.ni);                                     // M:3257 on the limited number
    return r;
}
// M:3258-3265, ilami**bv_i with bv_i = 1
__device__ inline void ice_fall_speeds(const FallConsts &c, double rhof, double lami, double &vti, double &vtni)
{
    const double ilami = 1. / lami;
    vti = rhof * av_i * c.cig3 * c.oig2 * ilami;
    vtni = rhof * av_i * c.cig6 / c.cig7 * ilami;
}

// snow's mass-weighted speed before the boost, M:3289-3299; s = snow_level(temp, rs, oams) of a level with rs > R1
__device__ inline double snow_fall_speed(const FallConsts &c, double rhof, const SnowLevel &s)
{
    const double smoc = snow_moment(c.sa, c.sb, c.cse1, s);               // M:1590-1600
    const double xDs = smoc / s.smob;
    const double Mrat = 1. / xDs;
    double ils1 = 1. / (Mrat * Lam0 + fv_s);
    double ils2 = 1. / (Mrat * Lam1 + fv_s);
    const double mm = fm::pow(Mrat, mu_s);
    const double t1_vts = Kap0 * c.csg4 * fm::pow(ils1, c.cse4);
    const double t2_vts = Kap1 * mm * c.csg10 * fm::pow(ils2, c.cse10);
    ils1 = 1. / (Mrat * Lam0);
    ils2 = 1. / (Mrat * Lam1);
    const double t3_vts = Kap0 * c.csg1 * cube(ils1);                     // **cse(1)
    const double t4_vts = Kap1 * mm * c.csg7 * fm::pow(ils2, c.cse7);
    return rhof * av_s * (t1_vts + t2_vts) / (t3_vts + t4_vts);
}
// M:3300-3305: vtr is the rain speed the level holds after the inheritance
__device__ inline double snow_boosted(double vts, double boost, double temp, double vtr)
{
    if (temp > (T_0 + 0.1)) return fmax(vts * boost, vts * ((vtr - vts * boost) / (temp - T_0)));
    return vts * boost;
}
// graupel of a level with rg > R1 once the running minimum N0_exp is known: M:1650-1652, M:3326-3331
__device__ inline double graupel_fall_speed(const FallConsts &c, double rhof, double N0_exp, double rg, double temp, double vtr)
{
    const double lam_exp = fm::sqrt_pos(fm::sqrt_pos(N0_exp * am_g * c.cgg1 / rg));    // **oge1
    const double lamg = lam_exp * c.lamg_fac;
    const double ilamg = 1. / lamg;
    const double vtg = rhof * av_g * c.cgg6 * c.ogg3 * fm::pow(ilamg, bv_g);
    return temp > T_0 ? fmax(vtg, vtr) : vtg;
}
// INT(DT/delta_tp + 1.) with delta_tp = dzq(k)/v, M:3241-3242, capped (U5); v > 1.E-3
constexpr int FALL_MAX_SUBSTEPS = 10000;
__device__ inline int fall_substeps(double dt, double dz, double v)
{
    const double x = dt / (dz / v) + 1.;
    return x < double(FALL_MAX_SUBSTEPS) ? int(x) : FALL_MAX_SUBSTEPS;    // a NaN counts as the cap
}

// ---- the Doppler moments (include/kidmp_doppler.h) at one level: the reflectivity-weighted mean vz = <v sigma>/<sigma>
// and second moment v2 = <v**2 sigma>/<sigma> of the fall speed v(D) = rhof*av*D**bv*EXP(-fv*D) over the size distribution
// calc_refl10cm gives the species, sigma ~ D**6 (rain, graupel) or D**(2 bm_s) (snow).  Closed forms; the exponents taken
// as integers are pinned by doppler_consts_supported: mu_r = mu_g = 0 and bv_r = 1 (n = 7), bm_s = 2 (n = 5).  Every base
// gives its logarithm once; vz and v2 share it. ----
__device__ inline double pow_parts(const fm::Log2Parts &l, double y) { return fm::pow10_times_pow(0., l, y); }   // x**y, l = log2_parts(x)

// rain: 7 lamr**7/(lamr+fv_r)**8 and 56 lamr**7/(lamr+2 fv_r)**9, formed from lamr/(lamr+f) <= 1 so that no power overflows
__device__ inline void rain_doppler(const DopplerConsts &d, double rhof, double lamr, double &vz, double &v2)
{
    const double s1 = lamr + fv_r, s2 = lamr + 2. * fv_r;
    const double va = rhof * av_r;
    vz = va * d.gr1 * (pw7(lamr / s1) / s1);
    v2 = va * va * d.gr2 * (pw7(lamr / s2) / (s2 * s2));
}
// graupel: Gamma(7+bv_g)/Gamma(7) ilamg**bv_g and Gamma(7+2 bv_g)/Gamma(7) ilamg**(2 bv_g); no MAX(vtg, vtrk) above T_0
__device__ inline void graupel_doppler(const DopplerConsts &d, double rhof, double ilamg, double &vz, double &v2)
{
    const fm::Log2Parts l = fm::log2_parts(ilamg);
    const double va = rhof * av_g;
    vz = va * d.gg1 * pow_parts(l, bv_g);
    v2 = va * va * d.gg2 * pow_parts(l, 2. * bv_g);
}
// snow: block O's t1..t4_vts form (M:3289-3299) at the reflectivity moment n = 2 bm_s + 1 = 5.  With Mrat = smob/smoc,
//   A(b,f) = Kap0 Gamma(5+b) (Mrat Lam0 + f)**-(5+b) + Kap1 Mrat**mu_s Gamma(5+mu_s+b) (Mrat Lam1 + f)**-(5+mu_s+b)
// and A(0,0) = Mrat**-5 * a00 with a00 a constant of the host.  No vts_boost, no above-freezing blend.
__device__ inline double snow_mrat(const ReflConsts &c, const DopplerConsts &d, const SnowLevel &s)
{
    const double smoc = snow_moment(c.sa, c.sb, d.cse1, s);
    return s.smob / smoc;
}
__device__ inline double snow_mrat_mu(double Mrat) { return pow_parts(fm::log2_parts(Mrat), mu_s); }    // Mrat**mu_s
__device__ inline void snow_doppler(const ReflConsts &c, const DopplerConsts &d, double rhof, const SnowLevel &s, double &vz, double &v2)
{
    const double Mrat = snow_mrat(c, d, s);
    const double mm = snow_mrat_mu(Mrat);
    const double m2 = Mrat * Mrat, m5 = m2 * m2 * Mrat;
    const double x0 = Mrat * Lam0, x1 = Mrat * Lam1;
    const double a1 = d.ks0_1 * pow_parts(fm::log2_parts(x0 + fv_s), -(5. + bv_s))
                    + d.ks1_1 * mm * pow_parts(fm::log2_parts(x1 + fv_s), -(5. + mu_s + bv_s));
    const double a2 = d.ks0_2 * pow_parts(fm::log2_parts(x0 + 2. * fv_s), -(5. + 2. * bv_s))
                    + d.ks1_2 * mm * pow_parts(fm::log2_parts(x1 + 2. * fv_s), -(5. + mu_s + 2. * bv_s));
    const double va = rhof * av_s, ia00 = m5 * d.ia00;                   // 1/A(0,0)
    vz = va * (a1 * ia00);
    v2 = va * va * (a2 * ia00);
}

// ---- the size spectra (include/kidmp_spectra.h) at one level: the slope and intercept of each species' distribution as
// mp_thompson loads the state, and one bin of it as the reference's table builders form it (M:3768, M:3967-3975,
// M:4157-4164, M:4206-4221).  Beyond fall_consts_supported the integer exponents are pinned by spectra_consts_supported:
// mu_r = mu_g = mu_i = 0 (cre(2) = cge(2) = cie(1) = 1), cce(1,n) = n + 1, cce(2,n) = bm_r + n + 1 with bm_r = 3. ----
// An exponential term whose argument exceeds SPECTRA_EXP_MAX is exact +0.0: fm::exp is written for |x| < 700, and below
// that EXP(-x) is a normal number.  A NaN argument gives +0.0 too.
constexpr double SPECTRA_EXP_MAX = 700.;
__device__ inline double exp_neg(double x) { return x <= SPECTRA_EXP_MAX ? fm::exp(-x) : 0.; }

// N0_r = nr*org2*lamr**cre(2) (M:1664, M:3757), N0_i = ni*oig1*lami**cie(1) (M:4206): cre(2) = cie(1) = 1
__device__ inline double rain_intercept(const FallConsts &c, const RainLoad &r) { return r.nr * c.org2 * r.lamr; }
__device__ inline double ice_intercept(const FallConsts &c, const IceLoad &r) { return r.ni * c.oig1 * r.lami; }

// graupel of a level with rg > R1 once the running minimum N0_exp is known: lamg and N0_g of block E (M:1650-1653), cge(2) = 1
__device__ inline void graupel_slope(const FallConsts &c, double cgg2, double N0_exp, double rg, double &lamg, double &N0_g)
{
    const double lam_exp = fm::sqrt_pos(fm::sqrt_pos(N0_exp * am_g * c.cgg1 / rg));    // **oge1
    lamg = lam_exp * c.lamg_fac;
    N0_g = N0_exp / (cgg2 * lam_exp) * lamg;
}

// cloud water as loaded, M:1395-1410, then nu_c and lamc as block G forms them from the loaded number (M:1690-1692).
// Nt_c: the context's, or the column's own (kidmp_set_column_nc); aero: the droplet number is the caller's nc1, limited
// through xDc (M:1402-1409).  A level without cloud water, or a droplet number that is not above R2 (calc_effectRad's
// test, M:4873), has has = false and nothing else is read.  The gamma functions of integers are taken exactly, as
// calc_effectRad takes its g_ratio (M:4852): ccg(2,n)*ocg1(n) = (n+1)(n+2)(n+3) and ccg(1,n) = n!, where thompson_init's
// WGAMMA is off by up to 9e-12 at n = 15 -- sixteen times that in lamc**cce(1,n).
struct CloudLoad { double nc, lamc, n0; int nu; bool has; };
__device__ inline double cloud_g_ratio(int nu) { return double((nu + 1) * (nu + 2) * (nu + 3)); }
__device__ inline double cloud_slope(int nu, double rc, double nc) { return cbrt_any(nc * am_r * cloud_g_ratio(nu) / rc); }
__device__ inline CloudLoad cloud_load(bool aero, double Nt_c, double rho, double qc, double nc1)
{
    CloudLoad r{0., 0., 0., 0, qc > R1};
    if (!r.has) return r;
    const double rc = qc * rho;
    r.nc = Nt_c;                                                           // .NOT. is_aerosol_aware, M:1410
    if (aero) {
        r.nc = fmax(2., nc1 * rho);
        const int nu = cloud_nu_c(r.nc);
        double lamc = cloud_slope(nu, rc, r.nc);
        const double xDc = (bm_r + nu + 1.) / lamc;
        if (xDc < D0c) lamc = (bm_r + nu + 1.) / D0c;                     // cce(2,nu_c)
        else if (xDc > D0r * 2.) lamc = (bm_r + nu + 1.) / (D0r * 2.);
        r.nc = fmin(Nt_c_max, rc / cloud_g_ratio(nu) / am_r * cube(lamc));  // ccg(1,nu_c)*ocg2(nu_c) = 1/g_ratio
    }
    r.has = r.nc > R2;
    if (!r.has) return r;
    r.nu = cloud_nu_c(r.nc);
    r.lamc = cloud_slope(r.nu, rc, r.nc);
    double pw = r.lamc, b = r.lamc;                                        // lamc**cce(1,nu_c) = lamc * lamc**nu_c, nu_c in 2..15
    for (int e = r.nu; e > 0; e >>= 1) {                                   // (binary powering: at most 4 squarings)
        if (e & 1) pw *= b;
        b *= b;
    }
    double fact = 2.;                                                      // ccg(1,nu_c) = nu_c!
    for (int i = 3; i <= r.nu; ++i) fact *= double(i);
    r.n0 = r.nc / fact * pw;                                               // nc*ocg1(nu_c)*lamc**cce(1,nu_c), M:4158
    return r;
}

// snow of a level with rs > R1: what M:3967-3971 hands the bin loop.  s = snow_level(temp, rs, oams), smoc its cse(1) moment
struct SnowSpectrum { double Mrat, k1m0, slam1, slam2; };
__device__ inline SnowSpectrum snow_spectrum(const SnowLevel &s, double smoc)
{
    const double r = s.smob / smoc;
    SnowSpectrum o;
    o.Mrat = s.smob * r * r * r;
    o.k1m0 = Kap1 * pow_parts(fm::log2_parts(r), mu_s);
    o.slam1 = r * Lam0;
    o.slam2 = r * Lam1;
    return o;
}
// one bin: D and dD are the bin's diameter and width, Dmu = D**mu_s
__device__ inline double snow_bin(const SnowSpectrum &s, double D, double Dmu, double dD)
{ return s.Mrat * (Kap0 * exp_neg(s.slam1 * D) + s.k1m0 * Dmu * exp_neg(s.slam2 * D)) * dD; }
// rain, graupel, cloud ice: N0 * D**0 * EXP(-lam*D) * dD
__device__ inline double exp_bin(double n0, double lam, double D, double dD) { return n0 * exp_neg(lam * D) * dD; }
// cloud water: N0_c * D**nu_c * EXP(-lamc*D) * dD with D**nu_c picked from D, D**2, D**4, D**8 (nu_c in 2..15)
__device__ inline double cloud_bin(double n0, double lam, int nu, double D, double D2, double D4, double D8, double dD)
{
    const double Dnu = ((nu & 1 ? D : 1.) * (nu & 2 ? D2 : 1.)) * ((nu & 4 ? D4 : 1.) * (nu & 8 ? D8 : 1.));
    return n0 * Dnu * exp_neg(lam * D) * dD;
}

// ---- the Doppler spectrum (include/kidmp_dspectrum.h): the reflectivity z_b of one diameter bin at one level, in the
// units of ze, and what depends on the bin alone.  Rain and graupel: z_b = (A * exp_neg(lam*D_b)) * G_b with A = N0_r or
// ZE_GRAUPEL_FAC*N0_g and G_b = D_b**6 * dD_b.  Snow: z_b = (zs * (Kap0*exp_neg(x0*D_b) + (k1*D_b**mu_s)*exp_neg(x1*D_b))) * G_b
// with zs = ze_s*(Mrat**5*ia00), x0 = Mrat*Lam0, x1 = Mrat*Lam1, k1 = Kap1*Mrat**mu_s and G_b = D_b**4 * dD_b.
// The fall speed of the bin in still air of density rho_not is vfac_b = av*D_b**bv*exp_neg(fv*D_b) (bv_r = 1; graupel has
// no exponential): the level multiplies by rhof. ----
struct SnowEcho { double zs, x0, x1, k1; };
__device__ inline SnowEcho snow_echo(const DopplerConsts &d, double ze_s, double Mrat)
{
    const double m2 = Mrat * Mrat, m5 = m2 * m2 * Mrat;
    SnowEcho o;
    o.zs = ze_s * (m5 * d.ia00);
    o.x0 = Mrat * Lam0;
    o.x1 = Mrat * Lam1;
    o.k1 = Kap1 * snow_mrat_mu(Mrat);
    return o;
}
__device__ inline double exp_echo(double A, double lam, double D, double G) { return (A * exp_neg(lam * D)) * G; }
__device__ inline double snow_echo_bin(const SnowEcho &s, double D, double Dmu, double G)
{ return (s.zs * (Kap0 * exp_neg(s.x0 * D) + (s.k1 * Dmu) * exp_neg(s.x1 * D))) * G; }
__device__ inline double rain_bin_speed(double D) { return av_r * D * exp_neg(fv_r * D); }                    // bv_r = 1
__device__ inline double snow_bin_speed(double D) { return av_s * fm::pow(D, bv_s) * exp_neg(fv_s * D); }
__device__ inline double graupel_bin_speed(double D) { return av_g * fm::pow(D, bv_g); }
__device__ inline double pw6_times(double D, double dD) { const double D2 = D * D; return D2 * D2 * D2 * dD; }
__device__ inline double pw4_times(double D, double dD) { const double D2 = D * D; return D2 * D2 * dD; }

// ---- the lidar operator (include/kidmp_lidar.h) at one level: geometric-optics extinction (Q_ext = 2, cross-section
// pi/4 D**2) of the size distributions above, in closed form, and the mean of EXP(-x') over a layer of two-way depth x. ----
constexpr double LIDAR_PI = 3.14159265358979323846, LIDAR_K_B = 1.380649e-23;
// rain, graupel, cloud ice (mu = 0): (pi/2) N0 Gamma(3)/lam**3 = pi N0/lam**3
__device__ inline double exp_extinction(double n0, double lam) { return LIDAR_PI * n0 / (lam * lam * lam); }
// cloud water: (pi/2) nc (nu_c+1)(nu_c+2)/lamc**2, nc the loaded number
__device__ inline double cloud_extinction(double nc, int nu, double lamc) { return (0.5 * LIDAR_PI) * nc * double((nu + 1) * (nu + 2)) / (lamc * lamc); }
// snow: (pi/2) times the second moment, which is smob while bm_s = 2
__device__ inline double snow_extinction(double smob) { return (0.5 * LIDAR_PI) * smob; }
// g(x) = (1 - EXP(-x))/x for x >= 0, g(0) = 1, without cancellation: below 1 as EXP(-x/2) * sinh(x/2)/(x/2), the second
// factor a series of positive terms in (x/2)**2 (nine terms: the next is 2e-22 at x = 1); from 1 on as written, where
// EXP(-x) <= 0.37 and the 700 rule of exp_neg leaves 1/x.  Within 3 ulp everywhere, subnormal x included (both factors 1).
__device__ inline double layer_mean(double x)
{
    if (x >= 1.) return (1. - exp_neg(x)) / x;
    const double y = 0.5 * x, z = y * y;
    double s = 1. / 355687428096000.;                                      // 1/17!
    s = s * z + 1. / 1307674368000.;
    s = s * z + 1. / 6227020800.;
    s = s * z + 1. / 39916800.;
    s = s * z + 1. / 362880.;
    s = s * z + 1. / 5040.;
    s = s * z + 1. / 120.;
    s = s * z + 1. / 6.;
    s = s * z + 1.;
    return fm::exp(-y) * s;
}

}  // namespace lvl
}  // namespace kidmp
