// thompson_reflectivity.hip -- calc_refl10cm (M:4946-5244) on gfx950: the 10-cm radar reflectivity the scheme's own size
// distributions give in the Rayleigh approximation, dBZ = 10 log10((ze_rain + ze_snow + ze_graupel) * 1e18) (M:5196).
//
// Only the live part of the reference is computed.  Dead as shipped: rc (qc1d is never read), rhof, smoc, the melting-level
// search k_0/melti (M:5107-5121) and the whole wet-snow/graupel block (M:5140-5192): with nrbins = 0 (M:204) its bin loops
// are empty and its ze_* assignments are commented out, so calc_refl10cm has no bright band; k_bright_band below is an
// entry of its own that rebuilds that block (include/kidmp_brightband.h).
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
//
// k_column_outputs is the same column body with calc_effectRad (M:4834-4935) of every level formed beside it, in the
// form of the scheme's driver (presets first, M:1111-1116): re_qc, re_qi, re_qs and dbz from one read of the state.  The
// per-level arithmetic of both diagnostics is thompson_levels.h, shared with the pointwise k_effective_radii.
#include "thompson_reflectivity.h"

#include <cmath>
#include <type_traits>

#include "thompson_levels.h"
#include "kidmp_wave.h"
#include "kidmp_dspectrum_slot.h"
#include "kidmp_radiometer_layer.h"

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

constexpr int REFL_WAVES = 4;                        // columns (wavefronts) per workgroup
constexpr int REFL_THREADS = 64 * REFL_WAVES;
using wave::readlane;                                // kidmp_wave.h
using wave::wave_prefix_sum;

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

// The exclusive sums of a column: up[j] = the sum of v over the levels below the lane's level of group j, dn[j] = over the
// levels above it.  The level groups are chained through a wave-uniform carry, upward for up and from the top for dn (a
// reversed scan, not total minus prefix: nothing cancels, dn is exact +0.0 at the top level and never negative).  Levels
// past nz must hold +0.0.  The order of every sum is a pure function of the level and of NJ.
template <int NJ>
__device__ inline void column_depths(const double (&v)[NJ], int lane, bool want_up, bool want_dn, double (&up)[NJ], double (&dn)[NJ])
{
    double carry = 0.;
    if (want_up) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            double total;
            const double below = __shfl_up(wave_prefix_sum<false>(v[j], lane, total), 1, 64);
            up[j] = carry + (lane > 0 ? below : 0.);
            carry = carry + total;
        }
    }
    carry = 0.;
    if (want_dn) {
#pragma unroll
        for (int j = NJ - 1; j >= 0; --j) {
            double total;
            const double above = __shfl_down(wave_prefix_sum<true>(v[j], lane, total), 1, 64);
            dn[j] = carry + (lane < 63 ? above : 0.);
            carry = carry + total;
        }
    }
}

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

// calc_refl10cm of the lane's levels k = 64 j + lane of the column at `base`, left in dbz[j] (untouched where k >= nz).
// at_level(j, i, temp, pres, qv_in, qv, rho, qs, L_qs, sl) is called once for every level of the lane, between its load
// and the graupel scan: what a kernel forms beside the reflectivity from the same read.  Whole wavefronts only.
template <class T, int NJ, class F>
__device__ __forceinline__ void column_dbz(const ReflConsts &c, int nz, int lane, int64_t base, const T *__restrict__ t1d,
                                           const T *__restrict__ p1d, const T *__restrict__ qv1d, const T *__restrict__ qr1d,
                                           const T *__restrict__ nr1d, const T *__restrict__ qs1d, const T *__restrict__ qg1d,
                                           double (&dbz)[NJ], F &&at_level)
{
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
        const double qv_in = double(qv1d[i]);
        const double qv = fmax(1.E-10, qv_in);
        const double pres = double(p1d[i]);
        const double rho = lvl::air_density(pres, temp, qv);
        const double qr = double(qr1d[i]);
        const double qs = qs1d ? double(qs1d[i]) : 0.;
        const double qg = qg1d ? double(qg1d[i]) : 0.;
        const bool L_qr = qr > R1, L_qs = qs > R2;
        lqg[j] = qg > R2;
        double ze_rain = 1.E-22, ze_snow = 1.E-22, mvd_r = 50.E-6;
        if (L_qr) ze_rain = lvl::rain_ze(c, rho, qr, double(nr1d[i]), mvd_r);
        lvl::SnowLevel sl{};
        if (L_qs) {                                                  // bm_s = 2: smo2 = smob = rs*oams, M:5033-5038
            sl = lvl::snow_level(temp, qs * rho, c.oams);
            ze_snow = lvl::snow_ze(c, sl);                           // M:5131-5132
        }
        at_level(j, i, temp, pres, qv_in, qv, rho, qs, L_qs, sl);
        if (lqg[j]) rg[j] = qg * rho;
        ze_rs[j] = ze_rain + ze_snow;
        // ---- graupel intercept before the running minimum, M:5088-5096 ----
        n0[j] = lvl::graupel_n0_exp(temp < 270.65 && L_qr && mvd_r > 100.E-6, mvd_r, rg[j]);
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
        if (64 * j + lane >= nz) continue;
        double ze_graupel = 1.E-22;
        if (lqg[j]) ze_graupel = lvl::graupel_ze(c, n0[j], rg[j]);    // M:5099-5102, M:5133-5135
        dbz[j] = lvl::dbz_of(ze_rs[j] + ze_graupel);                  // M:5196
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
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);            // log10 / 10**x / x**y read their tables from LDS
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scan needs every lane
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

// ---- the per-column summary (include/kidmp_summary.h) ----
// butterfly over the wave: every lane ends with the same bits (a + b == b + a), in an order that depends on nothing
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}
// the lowest / highest level whose predicate holds, -1 if none: one ballot per level group, the level is a bit position
template <int NJ>
__device__ inline int lowest_level(const bool (&pred)[NJ])
{
    int k = -1;
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {
        const unsigned long long b = __ballot(pred[j]);
        if (b) k = 64 * j + __builtin_ctzll(b);
    }
    return k;
}
template <int NJ>
__device__ inline int highest_level(const bool (&pred)[NJ], int &count)
{
    int k = -1;
    count = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const unsigned long long b = __ballot(pred[j]);
        if (b) k = 64 * j + 63 - __builtin_clzll(b);
        count += __builtin_popcountll(b);
    }
    return k;
}
// sum of dz over the column's levels below `ktop` (ktop <= 0: +0.0), in the fixed order of wave_sum
template <int NJ>
__device__ inline double height_below(const double (&dz)[NJ], int lane, int ktop)
{
    double s = 0.;
#pragma unroll
    for (int j = 0; j < NJ; ++j) s += 64 * j + lane < ktop ? dz[j] : 0.;
    return wave_sum(s);
}
// v of level k (wave-uniform, 0 <= k < nz)
template <int NJ>
__device__ inline double level_of(const double (&v)[NJ], int k)
{
    double x = readlane(v[0], k & 63);                               // a lane read per group: the array stays in registers
#pragma unroll
    for (int j = 1; j < NJ; ++j) {
        const double y = readlane(v[j], k & 63);
        x = (k >> 6) == j ? y : x;
    }
    return x;
}

// ---- the fall speeds (include/kidmp_fall.h) ----
__device__ inline int wave_max_int(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}
template <int D>
__device__ inline int row_shl_int(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x100 + D, 0xf, 0xf, false); }

// One step of the inheritance scan: a lane whose level lacks the species takes what lane l + D of its row holds.
template <int D, bool TWO>
__device__ inline void carry_step(double &a, double &b, int &h, int r)
{
    const double oa = row_shl<D>(a), ob = TWO ? row_shl<D>(b) : 0.;
    const int oh = row_shl_int<D>(h);
    const bool take = r + D < 16 && !h;
    a = take ? oa : a;
    if (TWO) b = take ? ob : b;
    h = take ? oh : h;
}
// vtrk(k) = vtrk(k+1) where the level lacks the species (M:3235, 3267, 3307, 3333) over the 64 levels of a wave: a suffix
// scan with the associative operator "keep mine if my level has the species, else take the one above".  Only moves: a
// lane ends with the bits of the nearest lane at or above it whose `has` is set, and the return value tells whether
// there is one.  (ta, tb, th): lane 0's result, wave-uniform -- what the whole wave hands down to the levels below it.
// One predicate carries both values (TWO: the mass- and the number-weighted speed).  Whole wavefronts only.
template <bool TWO>
__device__ inline bool wave_carry_down(double &a, double &b, bool has, int lane, double &ta, double &tb, bool &th)
{
    int h = has;
    const int r = lane & 15;
    carry_step<1, TWO>(a, b, h, r);
    carry_step<2, TWO>(a, b, h, r);
    carry_step<4, TWO>(a, b, h, r);
    carry_step<8, TWO>(a, b, h, r);
    // lane 16 q holds what row q hands down
    const double a1 = readlane(a, 16), a2 = readlane(a, 32), a3 = readlane(a, 48);
    const double b1 = TWO ? readlane(b, 16) : 0., b2 = TWO ? readlane(b, 32) : 0., b3 = TWO ? readlane(b, 48) : 0.;
    const int h1 = __builtin_amdgcn_readlane(h, 16), h2 = __builtin_amdgcn_readlane(h, 32), h3 = __builtin_amdgcn_readlane(h, 48);
    const double u2a = a3, u1a = h2 ? a2 : a3, u0a = h1 ? a1 : u1a;     // what the rows above row q hand down
    const double u2b = b3, u1b = h2 ? b2 : b3, u0b = h1 ? b1 : u1b;
    const int u2h = h3, u1h = h2 | h3, u0h = h1 | u1h;
    const int q = lane >> 4;
    const int uh = q == 0 ? u0h : q == 1 ? u1h : q == 2 ? u2h : 0;
    if (!h && uh) {
        a = q == 0 ? u0a : q == 1 ? u1a : u2a;
        if (TWO) b = q == 0 ? u0b : q == 1 ? u1b : u2b;
        h = 1;
    }
    ta = readlane(a, 0);
    tb = TWO ? readlane(b, 0) : 0.;
    th = __builtin_amdgcn_readlane(h, 0) != 0;
    return h != 0;
}
// the column: the level groups chained from the top, the value above the top level is 0 (M:3209-3216)
template <int NJ, bool TWO>
__device__ inline void carry_down_column(double (&a)[NJ], double (&b)[NJ], const bool (&has)[NJ], int lane)
{
    double ca = 0., cb = 0.;
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {
        double ta, tb;
        bool th;
        const bool h = wave_carry_down<TWO>(a[j], b[j], has[j], lane, ta, tb, th);
        if (!h) { a[j] = ca; if (TWO) b[j] = cb; }
        if (th) { ca = ta; cb = tb; }
    }
}
// nstep of one species: MAX over the levels with v > 1.E-3 of INT(DT/delta_tp + 1.) (M:3239-3243); 0 is reported as 1,
// as NINT(1./onstep) gives it (M:3365)
template <int NJ>
__device__ inline int column_substeps(const double (&v)[NJ], const double (&dz)[NJ], double dt, int nz, int lane)
{
    int ns = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (64 * j + lane < nz && v[j] > 1.E-3) ns = max(ns, lvl::fall_substeps(dt, dz[j], v[j]));
    ns = wave_max_int(ns);
    return ns > 0 ? ns : 1;
}
template <class T, int NJ>
__device__ inline void store_profile(T *__restrict__ out, int64_t base, int nz, int lane, const double (&v)[NJ])
{
    if (!out) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        if (k < nz) out[base + k] = T(v[j]);
    }
}

// Block E's intercept of every level of the column (M:1633-1647): k_0 is the highest level with temp >= 270.65
// (M:1634-1637), mvd the limited median volume diameter of the level's rain (0: none), rg the graupel content (R1: none);
// n0 receives the running minimum from the top down (N0_min = gonv_max above the top, M:1633).  Whole wavefronts only.
template <int NJ>
__device__ inline void graupel_intercepts(const double (&temp)[NJ], const double (&mvd)[NJ], const double (&rg)[NJ], int nz, int lane,
                                          double (&n0)[NJ])
{
    int k_0 = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const unsigned long long b = __ballot(64 * j + lane < nz && temp[j] >= 270.65);
        if (b) k_0 = 64 * j + 63 - __builtin_clzll(b);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k < nz) n0[j] = lvl::graupel_n0_exp(k > k_0 && mvd[j] > 100.E-6, mvd[j], rg[j]);
    }
    double carry = gonv_max;
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {
        double tail;
        const double s = wave_suffix_min(n0[j], lane, tail);
        n0[j] = fmin(s, carry);
        carry = fmin(carry, tail);
    }
}

// ---- the size spectra (include/kidmp_spectra.h) ----
// The rows of one species that this block owns: the species' nb bins are dealt to the gridDim.y blocks of a column group in
// contiguous shares, and every bin is formed from the level's parameters and the bin's own D, dD alone, so its bits do not
// depend on the share it falls into.  out is [ncol][nb][nz]: one contiguous row of nz values per bin.  bin(j, D, dD, Dmu)
// gives the value of the lane's level of group j; live[j] is wave-uniform: no level of group j holds the species, and the
// row is +0.0 without an exponential.  POW: Dmu = D**mu_s, formed once per bin -- 64 bins at a time, one per lane, and
// handed round with v_readlane.  D and dD are wave-uniform loads.
template <class T, int NJ, bool POW, class F>
__device__ __forceinline__ void store_bins(T *__restrict__ out, const double *__restrict__ D, const double *__restrict__ dD, int nb,
                                           int64_t col, int nz, int lane, const double (&n0)[NJ], F &&bin)
{
    if (!out) return;
    const int per = (nb + int(gridDim.y) - 1) / int(gridDim.y);
    const int b0 = int(blockIdx.y) * per, b1 = b0 + per < nb ? b0 + per : nb;
    bool live[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) live[j] = __ballot(n0[j] > 0.) != 0;
    for (int bb = b0; bb < b1; bb += 64) {
        double mine = 0.;
        if (POW && bb + lane < b1) mine = fm::pow(D[bb + lane], mu_s);
        const int be = bb + 64 < b1 ? bb + 64 : b1;
        for (int b = bb; b < be; ++b) {
            const double Db = D[b], dDb = dD[b];
            const double Dmu = POW ? readlane(mine, b - bb) : 0.;
            T *__restrict__ row = out + (col * int64_t(nb) + b) * int64_t(nz);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int k = 64 * j + lane;
                double v = 0.;
                if (live[j]) v = bin(j, Db, dDb, Dmu);
                if (k < nz) row[k] = T(v);
            }
        }
    }
}

// ---- the state as mp_thompson loads it, species by species: what k_size_spectra and k_lidar_profiles share, so that the
// load is stated once (include/kidmp_spectra.h).  A: SpectraArgs or LidarArgs (t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg,
// set_nc_col, aero; a null frozen input: the species is absent everywhere).  A level whose species is absent, and a lane
// whose level does not exist, keep exact +0.0 in all of the species' own values.  Whole wavefronts only. ----
// M:1387-1391: temperature, pressure and the density from qv' = max(1e-10, qv); idle lanes: temp = pres = 0, rho = 1
template <int NJ, class A>
__device__ __forceinline__ void load_air(const A &a, int64_t base, int nz, int lane, double (&temp)[NJ], double (&pres)[NJ], double (&rho)[NJ])
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        temp[j] = 0.; pres[j] = 0.; rho[j] = 1.;
        if (k >= nz) continue;
        const int64_t i = base + k;
        temp[j] = double(a.t[i]);
        pres[j] = double(a.p[i]);
        rho[j] = lvl::air_density(pres[j], temp[j], fmax(1.E-10, double(a.qv[i])));
    }
}
// rain, M:1447-1474: its slope, its intercept and the limited median volume diameter that block E reads (0: no rain, M:1639)
template <int NJ, class A>
__device__ __forceinline__ void load_rain(const Consts *__restrict__ hc, FallConsts &c, const A &a, int64_t base, int nz, int lane,
                                          const double (&rho)[NJ], double (&mvd)[NJ], double (&lam)[NJ], double (&n0)[NJ])
{
    c.crg2 = hc->crg[1]; c.crg3 = hc->crg[2]; c.org2 = hc->org2; c.org3 = hc->org3;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        mvd[j] = 0.; n0[j] = lam[j] = 0.;
        if (k >= nz) continue;
        const lvl::RainLoad r = lvl::rain_load(c, rho[j], double(a.qr[base + k]), double(a.nr[base + k]));
        if (!r.has) continue;
        mvd[j] = r.mvd;
        lam[j] = r.lamr;
        n0[j] = lvl::rain_intercept(c, r);
    }
}
// cloud ice, M:1420-1445
template <int NJ, class A>
__device__ __forceinline__ void load_ice(const Consts *__restrict__ hc, FallConsts &c, const A &a, int64_t base, int nz, int lane,
                                         const double (&rho)[NJ], double (&lam)[NJ], double (&n0)[NJ])
{
    c.cie2 = hc->cie[1]; c.cig1 = hc->cig[0]; c.cig2 = hc->cig[1]; c.oig1 = hc->oig1; c.oig2 = hc->oig2;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        n0[j] = lam[j] = 0.;
        if (k >= nz || !a.qi) continue;
        const lvl::IceLoad r = lvl::ice_load(c, rho[j], double(a.qi[base + k]), double(a.ni[base + k]));
        if (!r.has) continue;
        lam[j] = r.lami;
        n0[j] = lvl::ice_intercept(c, r);
    }
}
// snow, M:1475-1483 and block D: smob; at(j, sl) is called at every level that holds snow, for what else the caller forms
// from the level's Field fit
template <int NJ, class A, class F>
__device__ __forceinline__ void load_snow(const Consts *__restrict__ hc, FallConsts &c, const A &a, int64_t base, int nz, int lane,
                                          const double (&temp)[NJ], const double (&rho)[NJ], double (&smob)[NJ], F &&at)
{
    c.oams = hc->oams;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        smob[j] = 0.;
        if (k >= nz || !a.qs) continue;
        const double qs = double(a.qs[base + k]);
        if (!(qs > R1)) continue;
        const lvl::SnowLevel sl = lvl::snow_level(temp[j], qs * rho[j], c.oams);
        smob[j] = sl.smob;
        at(j, sl);
    }
}
// graupel, M:1484-1492 and block E (M:1633-1654): the intercept is the running minimum from the top down over all levels
template <int NJ, class A>
__device__ __forceinline__ void load_graupel(const Consts *__restrict__ hc, FallConsts &c, const A &a, int64_t base, int nz, int lane,
                                             const double (&temp)[NJ], const double (&rho)[NJ], const double (&mvd)[NJ], double (&lam)[NJ],
                                             double (&n0)[NJ])
{
    double rg[NJ];
    bool has[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        rg[j] = R1; has[j] = false;
        if (k >= nz || !a.qg) continue;
        const double qg = double(a.qg[base + k]);
        has[j] = qg > R1;
        if (has[j]) rg[j] = qg * rho[j];
    }
    graupel_intercepts<NJ>(temp, mvd, rg, nz, lane, n0);
    const double cgg2 = hc->cgg[1];
    c.cgg1 = hc->cgg[0]; c.lamg_fac = hc->lamg_fac;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const double n0_exp = n0[j];
        n0[j] = lam[j] = 0.;
        if (has[j]) lvl::graupel_slope(c, cgg2, n0_exp, rg[j], lam[j], n0[j]);
    }
}
// cloud water, M:1395-1410 and M:1690-1692: the loaded number nc, nu_c, lamc and the intercept
template <int NJ, class A>
__device__ __forceinline__ void load_cloud(const Consts *__restrict__ hc, const A &a, int64_t col, int64_t base, int nz, int lane,
                                           const double (&rho)[NJ], double (&lam)[NJ], double (&n0)[NJ], double (&nc)[NJ], int (&nu)[NJ])
{
    const double Nt_c = a.set_nc_col ? a.set_nc_col[col] * 1.e6 : hc->Nt_c;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        n0[j] = lam[j] = nc[j] = 0.; nu[j] = 0;
        if (k >= nz) continue;
        const lvl::CloudLoad r = lvl::cloud_load(a.aero != 0, Nt_c, rho[j], double(a.qc[base + k]), a.nc ? double(a.nc[base + k]) : 0.);
        if (!r.has) continue;
        lam[j] = r.lamc; n0[j] = r.n0; nc[j] = r.nc; nu[j] = r.nu;
    }
}

}  // namespace

// what block O reads, picked from the context's Consts: on the device from its copy in HBM (scalar loads on demand: as
// kernel arguments the 50 values pressed on the SGPRs), on the host for whoever wants to look
__host__ __device__ FallConsts fall_consts(const Consts &hc)
{
    FallConsts c{};
    c.crg2 = hc.crg[1]; c.crg3 = hc.crg[2]; c.crg6 = hc.crg[5]; c.crg7 = hc.crg[6]; c.crg12 = hc.crg[11];
    c.org2 = hc.org2; c.org3 = hc.org3;
    c.cie2 = hc.cie[1]; c.cig1 = hc.cig[0]; c.cig2 = hc.cig[1]; c.cig3 = hc.cig[2]; c.cig6 = hc.cig[5]; c.cig7 = hc.cig[6];
    c.oig1 = hc.oig1; c.oig2 = hc.oig2;
    c.cse1 = hc.cse[0]; c.cse4 = hc.cse[3]; c.cse7 = hc.cse[6]; c.cse10 = hc.cse[9];
    c.csg1 = hc.csg[0]; c.csg4 = hc.csg[3]; c.csg7 = hc.csg[6]; c.csg10 = hc.csg[9]; c.oams = hc.oams;
    for (int i = 0; i < 10; ++i) { c.sa[i] = hc.sa[i]; c.sb[i] = hc.sb[i]; }
    c.cgg1 = hc.cgg[0]; c.cgg6 = hc.cgg[5]; c.ogg3 = hc.ogg3; c.lamg_fac = hc.lamg_fac;
    return c;
}

// One wavefront per column: block O (M:3206-3354) of the state as mp_thompson loads it -- the fall speeds of rain, ice,
// snow and graupel at every level, the sedimentation fluxes v * rho q and, on request, the CFL substep counts
// (include/kidmp_fall.h).  Species by species: the level's own speed, the inheritance scan, the stores; rain first,
// because snow and graupel read the inherited rain speed.  Nothing but the fastmath tables is in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_fall_speeds(const Consts *__restrict__ hc, FallArgs<T> a, int64_t ncol, int nz)
{
    const FallConsts c = fall_consts(*hc);
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    const bool count = a.nstep != nullptr;

    double temp[NJ], rho[NJ], rhof[NJ], mvd[NJ], dz[NJ], vtr[NJ], ftot[NJ];
    double va[NJ], vb[NJ], rq[NJ], fx[NJ];                           // the species at hand: its two speeds, its content rho*q, its flux
    bool has[NJ];
    int ns_r = 1, ns_i = 1, ns_s = 1, ns_g = 1;

    // ---- load (M:1387-1391, M:1447-1474) and rain (M:3221-3237) ----
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        temp[j] = 0.; rho[j] = 1.; rhof[j] = 0.; mvd[j] = 0.; dz[j] = 1.; va[j] = vb[j] = 0.; rq[j] = R1; has[j] = false;
        if (k >= nz) continue;
        const int64_t i = base + k;
        temp[j] = double(a.t[i]);
        rho[j] = lvl::air_density(double(a.p[i]), temp[j], fmax(1.E-10, double(a.qv[i])));
        rhof[j] = fm::sqrt_pos(rho_not / rho[j]);                    // M:3219
        if (count) dz[j] = double(a.dz[col * a.dz_col_stride + k]);
        const lvl::RainLoad r = lvl::rain_load(c, rho[j], double(a.qr[i]), double(a.nr[i]));
        has[j] = r.rr > R1;                                          // block O asks the content, M:3221
        rq[j] = r.rr;
        if (r.has) mvd[j] = r.mvd;                                   // 0: no rain (block E asks L_qr, M:1639)
        if (has[j]) lvl::rain_fall_speeds(c, rhof[j], r.lamr, va[j], vb[j]);
    }
    carry_down_column<NJ, true>(va, vb, has, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) { vtr[j] = va[j]; fx[j] = va[j] * rq[j]; ftot[j] = fx[j]; }      // sed_r, M:3368
    store_profile<T, NJ>(a.out[0], base, nz, lane, va);
    store_profile<T, NJ>(a.out[1], base, nz, lane, vb);
    store_profile<T, NJ>(a.out[6], base, nz, lane, fx);
    if (count) {
        double vm[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) vm[j] = fmax(va[j], vb[j]);     // M:3239
        ns_r = column_substeps<NJ>(vm, dz, a.dt, nz, lane);
    }

    if (a.warm) {                                                    // M:3346-3352: exact zeros
#pragma unroll
        for (int j = 0; j < NJ; ++j) va[j] = 0.;
#pragma unroll
        for (int o = 2; o < 10; ++o)
            if (o != 6) store_profile<T, NJ>(a.out[o], base, nz, lane, va);
    } else {
        // ---- cloud ice, M:1420-1445 and M:3253-3269 ----
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            va[j] = vb[j] = 0.; rq[j] = R1; has[j] = false;
            if (k >= nz) continue;
            const lvl::IceLoad r = lvl::ice_load(c, rho[j], double(a.qi[base + k]), double(a.ni[base + k]));
            has[j] = r.ri > R1;                                      // M:3256
            rq[j] = r.ri;
            if (has[j]) lvl::ice_fall_speeds(c, rhof[j], r.lami, va[j], vb[j]);
        }
        carry_down_column<NJ, true>(va, vb, has, lane);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { fx[j] = va[j] * rq[j]; ftot[j] = ftot[j] + fx[j]; }
        store_profile<T, NJ>(a.out[2], base, nz, lane, va);
        store_profile<T, NJ>(a.out[3], base, nz, lane, vb);
        store_profile<T, NJ>(a.out[7], base, nz, lane, fx);
        if (count) ns_i = column_substeps<NJ>(va, dz, a.dt, nz, lane);

        // ---- snow, M:1475-1483, block D and M:3285-3308 ----
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            va[j] = 0.; rq[j] = R1; has[j] = false;
            if (k >= nz) continue;
            const double qs = double(a.qs[base + k]);
            if (qs > R1) rq[j] = qs * rho[j];                        // M:1475-1483
            has[j] = rq[j] > R1;                                     // M:3288
            if (!has[j]) continue;
            const double boost = a.boost ? double(a.boost[base + k]) : temp[j] < T_0 ? 1.0 : 1.5;   // M:2027, M:1751
            const double vts = lvl::snow_fall_speed(c, rhof[j], lvl::snow_level(temp[j], rq[j], c.oams));
            va[j] = lvl::snow_boosted(vts, boost, temp[j], vtr[j]);
        }
        carry_down_column<NJ, false>(va, vb, has, lane);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { fx[j] = va[j] * rq[j]; ftot[j] = ftot[j] + fx[j]; }
        store_profile<T, NJ>(a.out[4], base, nz, lane, va);
        store_profile<T, NJ>(a.out[8], base, nz, lane, fx);
        if (count) ns_s = column_substeps<NJ>(va, dz, a.dt, nz, lane);

        // ---- graupel, M:1484-1492, block E (M:1633-1654) and M:3322-3334 ----
        double n0[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            va[j] = 0.; rq[j] = R1; has[j] = false;
            if (k >= nz) continue;
            const double qg = double(a.qg[base + k]);
            if (qg > R1) rq[j] = qg * rho[j];                        // M:1484-1492
            has[j] = rq[j] > R1;                                     // M:3325
        }
        graupel_intercepts<NJ>(temp, mvd, rq, nz, lane, n0);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (has[j]) va[j] = lvl::graupel_fall_speed(c, rhof[j], n0[j], rq[j], temp[j], vtr[j]);
        carry_down_column<NJ, false>(va, vb, has, lane);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { fx[j] = va[j] * rq[j]; ftot[j] = ftot[j] + fx[j]; }
        store_profile<T, NJ>(a.out[5], base, nz, lane, va);
        store_profile<T, NJ>(a.out[9], base, nz, lane, fx);
        if (count) ns_g = column_substeps<NJ>(va, dz, a.dt, nz, lane);
    }
    store_profile<T, NJ>(a.out[10], base, nz, lane, ftot);
    if (count && lane < 4) a.nstep[col * 4 + lane] = lane == 0 ? ns_r : lane == 1 ? ns_i : lane == 2 ? ns_s : ns_g;
}

// One wavefront per column and share of the bins: the size distributions of the state as mp_thompson loads it, on diameter
// bins (include/kidmp_spectra.h).  Species by species -- rain first, whose median volume diameter the graupel intercept
// reads -- the level's slope and intercept are formed once in registers, stored by the column's first share if asked for,
// and the species' bins follow at once, so that only one species' parameters are live at a time.  The load is
// k_fall_speeds' own, through the same lvl:: functions, stated once in load_air .. load_cloud above, which
// k_lidar_profiles calls as well.  Nothing but the fastmath tables is in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_size_spectra(const Consts *__restrict__ hc, SpectraArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scan needs every lane
    const int64_t base = col * int64_t(nz);
    const bool first = blockIdx.y == 0;                              // the share that stores the parameters
    T *const *par = a.par;
    const auto params = [&](int v, const double (&x)[NJ]) __attribute__((always_inline)) { if (first) store_profile<T, NJ>(par[v], base, nz, lane, x); };
    const auto wants = [&](int sp, int p0, int p1, int p2) __attribute__((always_inline)) { return a.spec[sp] || par[p0] || par[p1] || (p2 >= 0 && par[p2]); };

    double temp[NJ], pres[NJ], rho[NJ], mvd[NJ], n0[NJ], lam[NJ];

    // (each species picks its own few constants from the context's copy in HBM just before it needs them: all fifty of
    //  fall_consts at once, beside the forty pointers of the arguments, do not fit the scalar registers)
    FallConsts c{};
    load_air<NJ>(a, base, nz, lane, temp, pres, rho);
    load_rain<NJ>(hc, c, a, base, nz, lane, rho, mvd, lam, n0);
    params(SPECTRA_LAM_R, lam);
    params(SPECTRA_LAM_R + 1, n0);
    store_bins<T, NJ, false>(a.spec[2], a.D[2], a.dD[2], a.nb[2], col, nz, lane, n0,
                             [&](int j, double D, double dD, double) __attribute__((always_inline)) { return n0[j] > 0. ? lvl::exp_bin(n0[j], lam[j], D, dD) : 0.; });

    if (wants(1, SPECTRA_LAM_I, SPECTRA_LAM_I + 1, -1)) {
        load_ice<NJ>(hc, c, a, base, nz, lane, rho, lam, n0);
        params(SPECTRA_LAM_I, lam);
        params(SPECTRA_LAM_I + 1, n0);
        store_bins<T, NJ, false>(a.spec[1], a.D[1], a.dD[1], a.nb[1], col, nz, lane, n0,
                                 [&](int j, double D, double dD, double) __attribute__((always_inline)) { return n0[j] > 0. ? lvl::exp_bin(n0[j], lam[j], D, dD) : 0.; });
    }

    if (wants(3, SPECTRA_SMOB, SPECTRA_SMOB + 1, -1)) {
        lvl::SnowSpectrum sp[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) { lam[j] = 0.; sp[j] = lvl::SnowSpectrum{0., 0., 0., 0.}; }
        c.cse1 = hc->cse[0];
#pragma unroll
        for (int i = 0; i < 10; ++i) { c.sa[i] = hc->sa[i]; c.sb[i] = hc->sb[i]; }
        load_snow<NJ>(hc, c, a, base, nz, lane, temp, rho, n0, [&](int j, const lvl::SnowLevel &sl) __attribute__((always_inline)) {
            lam[j] = lvl::snow_moment(c.sa, c.sb, c.cse1, sl);      // smoc, M:1590-1600
            sp[j] = lvl::snow_spectrum(sl, lam[j]);
        });
        params(SPECTRA_SMOB, n0);
        params(SPECTRA_SMOB + 1, lam);
        store_bins<T, NJ, true>(a.spec[3], a.D[3], a.dD[3], a.nb[3], col, nz, lane, n0,
                                [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return n0[j] > 0. ? lvl::snow_bin(sp[j], D, Dmu, dD) : 0.; });
    }

    if (wants(4, SPECTRA_LAM_G, SPECTRA_LAM_G + 1, -1)) {
        load_graupel<NJ>(hc, c, a, base, nz, lane, temp, rho, mvd, lam, n0);
        params(SPECTRA_LAM_G, lam);
        params(SPECTRA_LAM_G + 1, n0);
        store_bins<T, NJ, false>(a.spec[4], a.D[4], a.dD[4], a.nb[4], col, nz, lane, n0,
                                 [&](int j, double D, double dD, double) __attribute__((always_inline)) { return n0[j] > 0. ? lvl::exp_bin(n0[j], lam[j], D, dD) : 0.; });
    }

    if (wants(0, SPECTRA_LAM_C, SPECTRA_LAM_C + 1, SPECTRA_LAM_C + 2)) {
        int nu[NJ];
        double ncl[NJ], fnu[NJ];
        load_cloud<NJ>(hc, a, col, base, nz, lane, rho, lam, n0, ncl, nu);
#pragma unroll
        for (int j = 0; j < NJ; ++j) fnu[j] = double(nu[j]);
        params(SPECTRA_LAM_C, lam);
        params(SPECTRA_LAM_C + 1, n0);
        params(SPECTRA_LAM_C + 2, fnu);
        store_bins<T, NJ, false>(a.spec[0], a.D[0], a.dD[0], a.nb[0], col, nz, lane, n0,
                                 [&](int j, double D, double dD, double) __attribute__((always_inline)) {
                                     const double D2 = D * D, D4 = D2 * D2;
                                     return n0[j] > 0. ? lvl::cloud_bin(n0[j], lam[j], nu[j], D, D2, D4, D4 * D4, dD) : 0.;
                                 });
    }
}

// One wavefront per column: the lidar operator of include/kidmp_lidar.h.  The load is k_size_spectra's, through the same
// functions, in the order of the total (c, i, r, s, g; rain before graupel, whose intercept reads rain's diameter), one
// species' slope and intercept live at a time.  The profiles that need no neighbour (the extinctions, bsc, bsc_mol) are
// stored first; a call that asks for nothing else ends there, without a scan and without an exponential.  Otherwise the
// optical depths are two pairs of wave scans (column_depths) of dtau and dtau_mol, the attenuated backscatter follows per
// level, and the eight numbers of the column come from wave_sum, ballots and height_below as in k_column_summary.
// Nothing but the fastmath tables is in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_lidar_profiles(const Consts *__restrict__ hc, LidarArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    T *const *out = a.out;
    const bool want_sr_up = out[LIDAR_SR_UP] != nullptr, want_sr_dn = out[LIDAR_SR_DN] != nullptr, summary = a.summary != nullptr;
    const bool want_up = out[LIDAR_TAU_UP] || out[LIDAR_ATT_UP] || want_sr_up || summary;
    const bool want_dn = out[LIDAR_TAU_DN] || out[LIDAR_ATT_DN] || want_sr_dn || summary;
    const bool totals = out[5] || out[6] || want_up || want_dn;      // ext and bsc take every species
    const auto wants = [&](int x) __attribute__((always_inline)) { return totals || out[x]; };

    double temp[NJ], pres[NJ], rho[NJ], mvd[NJ], lam[NJ], n0[NJ], e[NJ], ext[NJ], bsc[NJ];
    FallConsts c{};
    load_air<NJ>(a, base, nz, lane, temp, pres, rho);
#pragma unroll
    for (int j = 0; j < NJ; ++j) ext[j] = bsc[j] = mvd[j] = 0.;
    // ext = (((ext_c + ext_i) + ext_r) + ext_s) + ext_g and bsc likewise of ext_x / S_x; an absent species adds +0.0
    const auto add = [&](int x) __attribute__((always_inline)) {
        store_profile<T, NJ>(out[x], base, nz, lane, e);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { ext[j] = x == 0 ? e[j] : ext[j] + e[j]; bsc[j] = x == 0 ? e[j] / a.s_ratio[0] : bsc[j] + e[j] / a.s_ratio[x]; }
    };
    if (wants(0)) {
        int nu[NJ];
        double ncl[NJ];
        load_cloud<NJ>(hc, a, col, base, nz, lane, rho, lam, n0, ncl, nu);
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] = lam[j] > 0. ? lvl::cloud_extinction(ncl[j], nu[j], lam[j]) : 0.;
        add(0);
    }
    if (wants(1)) {
        load_ice<NJ>(hc, c, a, base, nz, lane, rho, lam, n0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] = lam[j] > 0. ? lvl::exp_extinction(n0[j], lam[j]) : 0.;
        add(1);
    }
    if (wants(2) || wants(4)) {
        load_rain<NJ>(hc, c, a, base, nz, lane, rho, mvd, lam, n0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] = lam[j] > 0. ? lvl::exp_extinction(n0[j], lam[j]) : 0.;
        add(2);
    }
    if (wants(3)) {
        load_snow<NJ>(hc, c, a, base, nz, lane, temp, rho, n0, [](int, const lvl::SnowLevel &) __attribute__((always_inline)) {});
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] = n0[j] > 0. ? lvl::snow_extinction(n0[j]) : 0.;
        add(3);
    }
    if (wants(4)) {
        load_graupel<NJ>(hc, c, a, base, nz, lane, temp, rho, mvd, lam, n0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] = lam[j] > 0. ? lvl::exp_extinction(n0[j], lam[j]) : 0.;
        add(4);
    }
    double bm[NJ];                                                   // bsc_mol = c_mol * N, N = p/(k_B T) molecules per m3
#pragma unroll
    for (int j = 0; j < NJ; ++j) bm[j] = 64 * j + lane < nz ? a.c_mol * (pres[j] / (lvl::LIDAR_K_B * temp[j])) : 0.;
    store_profile<T, NJ>(out[5], base, nz, lane, ext);
    store_profile<T, NJ>(out[6], base, nz, lane, bsc);
    store_profile<T, NJ>(out[7], base, nz, lane, bm);
    if (!(want_up || want_dn)) return;                               // wave-uniform

    // ---- optical depth: dtau = (eta ext + ext_mol) dz, dtau_mol = ext_mol dz; levels past nz hold +0.0 ----
    const T *__restrict__ dzc = a.dz + col * a.dz_col_stride;
    double dz[NJ], dt[NJ], dm[NJ], tu[NJ], td[NJ], mu[NJ], md[NJ], part = 0., mol = 0.;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        dz[j] = k < nz ? double(dzc[k]) : 0.;
        const double em = (8. * lvl::LIDAR_PI / 3.) * bm[j];
        dt[j] = (a.eta * ext[j] + em) * dz[j];
        dm[j] = em * dz[j];
        part += ext[j] * dz[j];
        mol += dm[j];
        tu[j] = td[j] = mu[j] = md[j] = 0.;
    }
    column_depths<NJ>(dt, lane, want_up, want_dn, tu, td);
    if (want_sr_up || want_sr_dn) column_depths<NJ>(dm, lane, want_sr_up, want_sr_dn, mu, md);
    store_profile<T, NJ>(out[LIDAR_TAU_UP], base, nz, lane, tu);
    store_profile<T, NJ>(out[LIDAR_TAU_DN], base, nz, lane, td);

    if (!(out[LIDAR_ATT_UP] || out[LIDAR_ATT_DN] || want_sr_up || want_sr_dn || summary)) return;   // the depths alone: no exponential

    // ---- layer-mean attenuated backscatter and the scattering ratio ----
    double au[NJ], ad[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const double b = bsc[j] + bm[j], g = lvl::layer_mean(2. * dt[j]);
        au[j] = want_up ? b * lvl::exp_neg(2. * tu[j]) * g : 0.;
        ad[j] = want_dn ? b * lvl::exp_neg(2. * td[j]) * g : 0.;
    }
    store_profile<T, NJ>(out[LIDAR_ATT_UP], base, nz, lane, au);
    store_profile<T, NJ>(out[LIDAR_ATT_DN], base, nz, lane, ad);
    if (want_sr_up || want_sr_dn) {
        double su[NJ], sd[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const double gm = lvl::layer_mean(2. * dm[j]);
            su[j] = want_sr_up ? au[j] / (bm[j] * lvl::exp_neg(2. * mu[j]) * gm) : 0.;
            sd[j] = want_sr_dn ? ad[j] / (bm[j] * lvl::exp_neg(2. * md[j]) * gm) : 0.;
        }
        store_profile<T, NJ>(out[LIDAR_SR_UP], base, nz, lane, su);
        store_profile<T, NJ>(out[LIDAR_SR_DN], base, nz, lane, sd);
    }
    if (!summary) return;

    // ---- the column's eight numbers: sums as in k_column_summary, levels by ballot, heights as masked sums of dz ----
    part = wave_sum(part);
    mol = wave_sum(mol);
    bool det_up[NJ], det_dn[NJ], lost_up[NJ], lost_dn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const bool level = 64 * j + lane < nz;
        det_up[j] = level && au[j] >= a.beta_detect;
        det_dn[j] = level && ad[j] >= a.beta_detect;
        lost_up[j] = level && lvl::exp_neg(2. * (tu[j] + dt[j])) < a.trans_lost;
        lost_dn[j] = level && lvl::exp_neg(2. * (td[j] + dt[j])) < a.trans_lost;
    }
    int n_up, n_dn, n_lost;
    const int k_base = lowest_level<NJ>(det_up), k_lost_up = lowest_level<NJ>(lost_up);
    const int k_top = highest_level<NJ>(det_dn, n_dn), k_lost_dn = highest_level<NJ>(lost_dn, n_lost);
    highest_level<NJ>(det_up, n_up);
    const double nan = __builtin_nan("");
    const double slot[LIDAR_SUMMARY_N] = {part, mol,
                                          k_base < 0 ? nan : height_below<NJ>(dz, lane, k_base),
                                          k_lost_up < 0 ? nan : height_below<NJ>(dz, lane, k_lost_up + 1),
                                          k_top < 0 ? nan : height_below<NJ>(dz, lane, k_top + 1),
                                          k_lost_dn < 0 ? nan : height_below<NJ>(dz, lane, k_lost_dn),
                                          double(n_up), double(n_dn)};
    double v = slot[0];
#pragma unroll
    for (int s = 1; s < LIDAR_SUMMARY_N; ++s) v = lane == s ? slot[s] : v;
    if (lane < LIDAR_SUMMARY_N) a.summary[col * LIDAR_SUMMARY_N + lane] = v;     // one 64-byte line
}

// ---- what k_doppler_moments and k_doppler_spectrum share: calc_refl10cm's load of one level (M:4991-5028) with the
// slopes and intercepts that column_dbz leaves inside lvl::rain_ze and lvl::graupel_ze ----
// An absent species: ze = 1.E-22 (M:5127-5136), lamr = N0_r = 0, sl zero.  n0_exp is the level's graupel intercept before
// the running minimum.  A: DopplerArgs, DSpectrumArgs or BrightBandArgs (t, p, qv, qr, nr; qs, qg null = zero).  temp and
// rs = qs*rho (R1 without snow, M:5019) are what the melting layer reads beside them.
struct RadarLevel {
    bool L_qr, L_qs, L_qg;
    double temp, rho, rs, rhof, rg, n0_exp, ze_rain, ze_snow, lamr, N0_r;
    lvl::SnowLevel sl;
};
template <class A>
__device__ __forceinline__ RadarLevel radar_level(const ReflConsts &c, const A &a, int64_t i)
{
    RadarLevel r;
    const double temp = double(a.t[i]);
    const double qv = fmax(1.E-10, double(a.qv[i]));
    const double rho = lvl::air_density(double(a.p[i]), temp, qv);
    const double qr = double(a.qr[i]);
    const double qs = a.qs ? double(a.qs[i]) : 0.;
    const double qg = a.qg ? double(a.qg[i]) : 0.;
    r.L_qr = qr > R1;
    r.L_qs = qs > R2;
    r.L_qg = qg > R2;
    r.rho = rho;
    r.rhof = fm::sqrt_pos(rho_not / rho);
    r.ze_rain = r.ze_snow = 1.E-22;
    r.lamr = r.N0_r = 0.;
    r.sl = lvl::SnowLevel{};
    r.rg = r.rs = R1;
    r.temp = temp;
    double mvd_r = 50.E-6;
    if (r.L_qr) r.ze_rain = lvl::rain_ze(c, rho, qr, double(a.nr[i]), mvd_r, r.lamr, r.N0_r);
    if (r.L_qs) {
        r.rs = qs * rho;
        r.sl = lvl::snow_level(temp, r.rs, c.oams);
        r.ze_snow = lvl::snow_ze(c, r.sl);
    }
    if (r.L_qg) r.rg = qg * rho;
    r.n0_exp = lvl::graupel_n0_exp(temp < 270.65 && r.L_qr && mvd_r > 100.E-6, mvd_r, r.rg);
    return r;
}
// N0_min = MIN(N0_exp, N0_min) from kte down to kts (M:5097-5098): n0 holds N0_exp (+inf past kte) and receives the
// running minimum, the level groups chained from the top through a wave-uniform carry.  Whole wavefronts only.
template <int NJ>
__device__ __forceinline__ void graupel_running_min(double (&n0)[NJ], int lane)
{
    double carry = gonv_max;
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {
        double tail;
        const double s = wave_suffix_min(n0[j], lane, tail);
        n0[j] = fmin(s, carry);
        carry = fmin(carry, tail);
    }
}

// One wavefront per column: the three radar moments of every level (include/kidmp_doppler.h).  The load, the ze_* and the
// order of their sum are column_dbz's, through the same lvl:: functions; beside them the reflectivity-weighted first and
// second moments of each species' fall speed.  Rain and snow are finished before the graupel scan and leave only their
// sums behind; graupel follows the running minimum of its intercept.  Nothing but the fastmath tables is in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_doppler_moments(ReflConsts c, DopplerConsts dc, DopplerArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scan needs every lane
    const int64_t base = col * int64_t(nz);

    // of rain and snow together: ze with the 1.E-22 of an absent species (dbz), ze of the present ones, ze*vz, ze*v2
    double ze_rs[NJ], wt[NJ], m1[NJ], m2[NJ], rhof[NJ], rg[NJ], n0[NJ];
    bool lqg[NJ], any[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        ze_rs[j] = wt[j] = m1[j] = m2[j] = rhof[j] = 0.;
        rg[j] = R1;
        lqg[j] = any[j] = false;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k >= nz) continue;
        const int64_t i = base + k;
        const RadarLevel r = radar_level(c, a, i);                   // ---- load, M:4991-5028 ----
        const bool L_qr = r.L_qr, L_qs = r.L_qs;
        const double ze_rain = r.ze_rain, ze_snow = r.ze_snow;
        lqg[j] = r.L_qg;
        any[j] = L_qr || L_qs || lqg[j];
        rhof[j] = r.rhof;
        rg[j] = r.rg;
        double vz_r = 0., v2_r = 0., vz_s = 0., v2_s = 0.;
        if (L_qr) lvl::rain_doppler(dc, rhof[j], r.lamr, vz_r, v2_r);
        if (L_qs) lvl::snow_doppler(c, dc, rhof[j], r.sl, vz_s, v2_s);
        ze_rs[j] = ze_rain + ze_snow;
        wt[j] = (L_qr ? ze_rain : 0.) + (L_qs ? ze_snow : 0.);
        m1[j] = ze_rain * vz_r + ze_snow * vz_s;                     // an absent species has vz = v2 = +0.0
        m2[j] = ze_rain * v2_r + ze_snow * v2_s;
        n0[j] = r.n0_exp;
        if (a.out[3]) a.out[3][i] = T(vz_r);
        if (a.out[4]) a.out[4][i] = T(vz_s);
        if (a.out[6]) a.out[6][i] = T(lvl::dbz_of(ze_rain));
        if (a.out[7]) a.out[7][i] = T(lvl::dbz_of(ze_snow));
    }

    graupel_running_min<NJ>(n0, lane);

#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        if (k >= nz) continue;
        const int64_t i = base + k;
        double ze_graupel = 1.E-22, vz_g = 0., v2_g = 0.;
        if (lqg[j]) {
            double ilamg;
            ze_graupel = lvl::graupel_ze(c, n0[j], rg[j], ilamg);
            lvl::graupel_doppler(dc, rhof[j], ilamg, vz_g, v2_g);
        }
        if (a.out[0]) a.out[0][i] = T(lvl::dbz_of(ze_rs[j] + ze_graupel));          // M:5196
        if (a.out[5]) a.out[5][i] = T(vz_g);
        if (a.out[8]) a.out[8][i] = T(lvl::dbz_of(ze_graupel));
        double vd = 0., sw = 0.;                                     // a level with no species: +0.0, w is not applied
        if (any[j]) {
            const double W = wt[j] + (lqg[j] ? ze_graupel : 0.);
            const double V = (m1[j] + ze_graupel * vz_g) / W;
            const double var = (m2[j] + ze_graupel * v2_g) / W - V * V;
            vd = V - (a.w ? double(a.w[i]) : 0.);
            sw = var > 0. ? fm::sqrt_pos(var) : 0.;
        }
        if (a.out[1]) a.out[1][i] = T(vd);
        if (a.out[2]) a.out[2][i] = T(sw);
    }
}

// ---- the Doppler spectrum (include/kidmp_dspectrum.h) ----
// what a level keeps for its bins: the three species' factors of lvl::exp_echo / lvl::snow_echo_bin
struct EchoLevel {
    double rhof, w, n0r, lamr, n0g, lamg;
    lvl::SnowEcho s;
    bool pr, ps, pg;
};
__device__ inline double wave_min(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}

// One species' bins of one level group into the slots [t0, t1) of the wave's tile, `acc` laid out [slot - t0][lane]:
// every lane owns a column of the tile, so no two lanes meet and the order of the additions to a slot is the order of
// the bins.  Slots are counted from `below` = 0: slot s holds velocity bin s - 1, slot nv + 1 is `above`.
// What depends on the bin alone is formed once per bin, 64 bins at a time and one per lane, and handed round with
// v_readlane.  Each of those lanes also bounds the slots its bin can reach at any level of the group, from the group's
// extremes of rhof and w: the position (rhof*vfac - w - v0)*idv is monotone in rhof and in w under rounding, so the bound
// holds exactly, and a bin that cannot reach the tile is passed over before its exponential.  The bound only prunes;
// whether a lane deposits is decided by its own slot, so the result does not depend on the tile.
template <int SP, class T>
__device__ __forceinline__ void deposit_species(double *__restrict__ acc, int t0, int t1, const EchoLevel &L, bool present,
                                                const DSpectrumArgs<T> &a, int lane)
{
    if (!__ballot(present)) return;
    const double inf = double(__builtin_inf());
    const bool wild = __ballot(present && !(fabs(L.rhof) < inf && fabs(L.w) < inf)) != 0;   // NaN or infinite: no bound
    const double rmin = wave_min(present ? L.rhof : inf), rmax = wave_max(present ? L.rhof : -inf);
    const double wmin = wave_min(present ? L.w : inf), wmax = wave_max(present ? L.w : -inf);
    const double *__restrict__ D = a.D[SP], *__restrict__ dD = a.dD[SP];
    const int nb = a.nb[SP], nv = a.nv, top = nv + 1;
    for (int bb = 0; bb < nb; bb += 64) {
        double mD = 0., mG = 0., mV = 0., mMu = 0.;
        bool reach = false;
        if (bb + lane < nb) {
            mD = D[bb + lane];
            const double dDb = dD[bb + lane];
            if (SP == 0) { mG = lvl::pw6_times(mD, dDb); mV = lvl::rain_bin_speed(mD); }
            if (SP == 1) { mG = lvl::pw4_times(mD, dDb); mV = lvl::snow_bin_speed(mD); mMu = fm::pow(mD, mu_s); }
            if (SP == 2) { mG = lvl::pw6_times(mD, dDb); mV = lvl::graupel_bin_speed(mD); }
            int lo = 0, hi = top;
            if (!wild && mV >= 0.) {
                lo = dspectrum_slot((rmin * mV - wmax - a.v0) * a.idv, nv).j + 1;
                hi = dspectrum_slot((rmax * mV - wmin - a.v0) * a.idv, nv).j + 2;
            }
            reach = hi >= t0 && lo < t1;
        }
        unsigned long long hit = __ballot(reach);
        while (hit) {
            const int b = __builtin_ctzll(hit);
            hit &= hit - 1;
            const double Db = readlane(mD, b), Gb = readlane(mG, b), Vb = readlane(mV, b);
            const double Dmu = SP == 1 ? readlane(mMu, b) : 0.;
            const DSpectrumSlot s = dspectrum_slot((L.rhof * Vb - L.w - a.v0) * a.idv, nv);
            const int s0 = s.j + 1, s1 = s.j + 2;                    // 0 .. nv, 1 .. nv + 1
            const bool in0 = s0 >= t0 && s0 < t1, in1 = s1 >= t0 && s1 < t1;
            if (present && (in0 || in1)) {
                double z = 0.;
                if (SP == 0) z = lvl::exp_echo(L.n0r, L.lamr, Db, Gb);
                if (SP == 1) z = lvl::snow_echo_bin(L.s, Db, Dmu, Gb);
                if (SP == 2) z = lvl::exp_echo(L.n0g, L.lamg, Db, Gb);
                if (in0) acc[(s0 - t0) * 64 + lane] += (1. - s.f) * z;
                if (in1) acc[(s1 - t0) * 64 + lane] += s.f * z;
            }
        }
    }
}

// One wavefront per column: the Doppler spectrum of every level (include/kidmp_dspectrum.h).  The load and the scan are
// k_doppler_moments' (radar_level, graupel_running_min); every level keeps the factors of its three species in registers.
// Then, per level group and per requested spectrum (total with below and above, rain, snow, graupel: one pass each), the
// nv + 2 slots are walked in tiles of DSPECTRUM_TILE: the tile's accumulators are a lane-private column in LDS, zeroed,
// filled species by species in the order rain, snow, graupel with the bins ascending, and written out as one row store
// per velocity bin.  No atomics; a slot's additions come in one order whatever the tile, the pass and the grid.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_doppler_spectrum(ReflConsts c, DopplerConsts dc, DSpectrumArgs<T> a, int64_t ncol, int nz)
{
    __shared__ double s_acc[REFL_WAVES][DSPECTRUM_TILE * 64];
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scan needs every lane
    const int64_t base = col * int64_t(nz);
    double *__restrict__ acc = s_acc[int(threadIdx.x) >> 6];

    EchoLevel lv[NJ];
    double rg[NJ], n0[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        lv[j] = EchoLevel{};
        rg[j] = R1;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k >= nz) continue;
        const int64_t i = base + k;
        const RadarLevel r = radar_level(c, a, i);
        lv[j].rhof = r.rhof;
        lv[j].pr = r.L_qr; lv[j].ps = r.L_qs; lv[j].pg = r.L_qg;
        if (r.L_qr || r.L_qs || r.L_qg) lv[j].w = a.w ? double(a.w[i]) : 0.;     // a level with no species: w is not read
        lv[j].n0r = r.N0_r; lv[j].lamr = r.lamr;
        if (r.L_qs) lv[j].s = lvl::snow_echo(dc, r.ze_snow, lvl::snow_mrat(c, dc, r.sl));
        rg[j] = r.rg;
        n0[j] = r.n0_exp;
    }
    graupel_running_min<NJ>(n0, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (!lv[j].pg) continue;
        double ilamg, N0_g;
        lvl::graupel_ze(c, n0[j], rg[j], ilamg, lv[j].lamg, N0_g);
        lv[j].n0g = lvl::ZE_GRAUPEL_FAC * N0_g;
    }

    const int nv = a.nv, nslot = nv + 2;
    for (int j = 0; j < NJ; ++j) {
        EchoLevel L = lv[0];
#pragma unroll
        for (int jj = 1; jj < NJ; ++jj)
            if (j == jj) L = lv[jj];
        const int k = 64 * j + lane;
        for (int pass = 0; pass < 4; ++pass) {
            const bool edges = pass == 0 && (a.out[4] || a.out[5]);
            T *__restrict__ spec = a.out[pass];
            if (!spec && !edges) continue;
            for (int t0 = 0; t0 < nslot; t0 += DSPECTRUM_TILE) {
                const int t1 = t0 + DSPECTRUM_TILE < nslot ? t0 + DSPECTRUM_TILE : nslot;
                if (!spec && t0 > 0 && t1 < nslot) continue;         // below and above alone: the first and the last tile
                for (int s = 0; s < t1 - t0; ++s) acc[s * 64 + lane] = 0.;
                if (pass == 0 || pass == 1) deposit_species<0, T>(acc, t0, t1, L, L.pr, a, lane);
                if (pass == 0 || pass == 2) deposit_species<1, T>(acc, t0, t1, L, L.ps, a, lane);
                if (pass == 0 || pass == 3) deposit_species<2, T>(acc, t0, t1, L, L.pg, a, lane);
                if (k < nz)
                    for (int s = t0; s < t1; ++s) {
                        const double v = acc[(s - t0) * 64 + lane];
                        if (s == 0) { if (edges && a.out[4]) a.out[4][base + k] = T(v); }
                        else if (s == nslot - 1) { if (edges && a.out[5]) a.out[5][base + k] = T(v); }
                        else if (spec) spec[(col * int64_t(nv) + (s - 1)) * int64_t(nz) + k] = T(v);
                    }
            }
        }
    }
}

// ---- the bright band (include/kidmp_brightband.h) ----
// sum over the wave in the order the header fixes: a butterfly over xor 32, 16, ..., 1; every lane ends with the same bits
__device__ inline double wave_sum_down(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
constexpr int BB_STRIDES = BRIGHTBAND_MAX_BINS / 64;

// One species' active levels of the column: the lanes sweep the diameter bins, lane l taking bins l, l + 64, ...  What
// depends on the bin alone -- D, dD, D**mu_s, the mass, the unmelted particle's ice and envelope, its dry weight -- is
// formed once per lane and kept in registers.  Per level group the ballot of active levels is walked by bit scans, lowest
// level first; the level's parameters arrive wave-uniform through v_readlane: fm and p0, p1, p2 = snow's Mrat, k1m0 and
// smob/smoc (lvl::SnowSpectrum) or graupel's N0_g and lamg.  enh receives the level's ratio in the lane that owns it.
// The order in which the pairs are taken changes no bit: every pair has accumulators of its own.
template <int SP, int NJ, class T>
__device__ __forceinline__ void bright_band_species(const BrightBandArgs<T> &a, int lane, const double (&fmelt)[NJ],
                                                    const double (&p0)[NJ], const double (&p1)[NJ], const double (&p2)[NJ],
                                                    double (&enh)[NJ])
{
    const double *__restrict__ D = a.D[SP], *__restrict__ dD = a.dD[SP];
    const int nb = a.nb[SP];
    double bD[BB_STRIDES], bdD[BB_STRIDES], bMu[BB_STRIDES];
    BBBin bb[BB_STRIDES];
#pragma unroll
    for (int q = 0; q < BB_STRIDES; ++q) {
        const int b = 64 * q + lane;
        bD[q] = bdD[q] = bMu[q] = 0.;
        bb[q] = BBBin{};
        if (b >= nb) continue;
        const double d = D[b];
        bD[q] = d;
        bdD[q] = dD[b];
        if (SP == 0) bMu[q] = fm::pow(d, mu_s);
        bb[q] = bb_bin(a.mix, SP == 0 ? am_s * (d * d) : am_g * (d * d * d), d);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        unsigned long long act = __ballot(fmelt[j] > 0.);
        while (act) {
            const int l = __builtin_ctzll(act);
            act &= act - 1;
            const double f = readlane(fmelt[j], l), u0 = readlane(p0[j], l), u1 = readlane(p1[j], l), u2 = readlane(p2[j], l);
            lvl::SnowSpectrum ss{};
            if (SP == 0) { ss.Mrat = u0; ss.k1m0 = u1; ss.slam1 = u2 * Lam0; ss.slam2 = u2 * Lam1; }
            double wet = 0., dry = 0.;
#pragma unroll
            for (int q = 0; q < BB_STRIDES; ++q) {
                if (64 * q >= nb) break;                             // wave-uniform
                if (64 * q + lane >= nb) continue;
                const double n = SP == 0 ? lvl::snow_bin(ss, bD[q], bMu[q], bdD[q]) : lvl::exp_bin(u0, u1, bD[q], bdD[q]);
                wet += n * bb_wet(a.mix, bb[q], f);
                dry += n * bb[q].dry;
            }
            wet = wave_sum_down(wet);
            dry = wave_sum_down(dry);
            const double e = dry > 0. ? wet / dry : 1.;
            if (lane == l) enh[j] = e;
        }
    }
}

// One wavefront per column: calc_refl10cm with the melting layer (include/kidmp_brightband.h).  The load and the scan are
// k_doppler_moments' (radar_level, graupel_running_min), lanes over levels.  The melting level comes from ballots, the top
// level group first; rs and rg of that level are handed round with v_readlane.  A column without a melting level stores
// the dry profiles and does nothing else; otherwise the few active (level, species) pairs below the melting level are
// integrated with the lanes over the diameter bins (bright_band_species).  No atomics, no scratch, nothing but the
// fastmath tables in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_bright_band(ReflConsts c, DopplerConsts dc, BrightBandArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);

    double ze_r[NJ], ze_s[NJ], ze_g[NJ], rs[NJ], rg[NJ], n0[NJ];
    double s0[NJ], s1[NJ], s2[NJ], g0[NJ], g1[NJ];                   // snow: tc0, smob, then Mrat, k1m0, smob/smoc; graupel: N0_g, lamg
    bool lqs[NJ], lqg[NJ], warm_rain[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        ze_r[j] = ze_s[j] = ze_g[j] = 1.E-22;
        rs[j] = rg[j] = R1;
        s0[j] = s1[j] = s2[j] = g0[j] = g1[j] = 0.;
        lqs[j] = lqg[j] = warm_rain[j] = false;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k >= nz) continue;
        const RadarLevel r = radar_level(c, a, base + k);            // ---- load, M:4991-5028 ----
        ze_r[j] = r.ze_rain;
        ze_s[j] = r.ze_snow;
        rs[j] = r.rs;
        rg[j] = r.rg;
        lqs[j] = r.L_qs;
        lqg[j] = r.L_qg;
        warm_rain[j] = k <= nz - 2 && r.temp > 273.15 && r.L_qr;     // M:5112
        s0[j] = r.sl.tc0;
        s1[j] = r.sl.smob;
        n0[j] = r.n0_exp;
    }
    graupel_running_min<NJ>(n0, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (!lqg[j]) continue;
        double ilamg;
        ze_g[j] = lvl::graupel_ze(c, n0[j], rg[j], ilamg, g1[j], g0[j]);
    }

    // ---- the melting level, M:5109-5118: the highest k with warm rain under snow or graupel; k0 = k + 1 ----
    unsigned long long ms[NJ], mg[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { ms[j] = __ballot(lqs[j]); mg[j] = __ballot(lqg[j]); }
    int k0 = -1;
    if (!a.warm) {
#pragma unroll
        for (int j = NJ - 1; j >= 0; --j) {
            unsigned long long above = (ms[j] | mg[j]) >> 1;         // bit l: level 64 j + l + 1 holds snow or graupel
            const int ju = j + 1 < NJ ? j + 1 : j;
            if (j + 1 < NJ) above |= (ms[ju] | mg[ju]) << 63;
            const unsigned long long hit = __ballot(warm_rain[j]) & above;
            if (hit && k0 < 0) k0 = 64 * j + 64 - __builtin_clzll(hit);
        }
    }

    double fms[NJ], fmg[NJ], es[NJ], eg[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { fms[j] = fmg[j] = 0.; es[j] = eg[j] = 1.; }
    if (k0 >= 0) {
        bool snow0 = false, graupel0 = false;                        // L_qs(k_0), L_qg(k_0)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if ((k0 >> 6) == j) { snow0 = (ms[j] >> (k0 & 63)) & 1; graupel0 = (mg[j] >> (k0 & 63)) & 1; }
        const double rs0 = level_of<NJ>(rs, k0), rg0 = level_of<NJ>(rg, k0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            if (k < k0 && lqs[j] && snow0) fms[j] = fmax(0.05, fmin(1. - rs[j] / rs0, 0.99));       // M:5152
            if (k < k0 && lqg[j] && graupel0) fmg[j] = fmax(0.05, fmin(1. - rg[j] / rg0, 0.99));    // M:5176
        }
        if (snow0 && (a.out[0] || a.out[1] || a.out[3])) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!(fms[j] > 0.)) continue;
                lvl::SnowLevel sl;
                sl.tc0 = s0[j];
                sl.smob = s1[j];
                sl.l2 = fm::log2_parts(sl.smob);
                const double smoc = lvl::snow_moment(c.sa, c.sb, dc.cse1, sl);
                const lvl::SnowSpectrum ss = lvl::snow_spectrum(sl, smoc);
                s0[j] = ss.Mrat;
                s1[j] = ss.k1m0;
                s2[j] = sl.smob / smoc;                              // slam1 = s2*Lam0, slam2 = s2*Lam1
            }
            bright_band_species<0, NJ, T>(a, lane, fms, s0, s1, s2, es);
        }
        if (graupel0 && (a.out[0] || a.out[2] || a.out[4]))
            bright_band_species<1, NJ, T>(a, lane, fmg, g0, g1, g1, eg);
    }

#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        if (k >= nz) continue;
        const int64_t i = base + k;
        const double zs = ze_s[j] * es[j], zg = ze_g[j] * eg[j];
        if (a.out[0]) a.out[0][i] = T(lvl::dbz_of(ze_r[j] + zs + zg));               // M:5196
        if (a.out[1]) a.out[1][i] = T(lvl::dbz_of(zs));
        if (a.out[2]) a.out[2][i] = T(lvl::dbz_of(zg));
        if (a.out[3]) a.out[3][i] = T(es[j]);
        if (a.out[4]) a.out[4][i] = T(eg[j]);
        if (a.out[5]) a.out[5][i] = T(fms[j]);
        if (a.out[6]) a.out[6][i] = T(fmg[j]);
    }
    if (a.k0 && lane == 0) a.k0[col] = k0;
}

// ---- the cloud radar (include/kidmp_mie.h) ----
constexpr double MIE_PIA = 20. / 2.302585092994045684;              // two-way dB per unit of one-way optical depth: 2*(10/ln 10)

// The loop over the bins of one species' table at every level of the lane, NR rows per bin.  The lanes hold levels; D, dD
// and the rows are wave-uniform loads.  density(j, D, dD, Dmu) gives n of the lane's level of group j; add(j, n, r) folds
// the bin's rows r[NR] into the caller's accumulators.  A level group none of whose levels holds the species is passed
// over.  SP == 1: Dmu = D**mu_s is formed once per bin, 64 bins at a time and one per lane, and handed round with
// v_readlane (as store_bins does).  A: MieArgs or RadiometerArgs.
template <int SP, int NJ, int NR, class A, class F, class G>
__device__ __forceinline__ void bin_loop(const A &a, int lane, const bool (&has)[NJ], F &&density, G &&add)
{
    const double *__restrict__ D = a.D[SP], *__restrict__ dD = a.dD[SP], *__restrict__ rows = a.rows[SP];
    const int nb = a.nb[SP];
    bool live[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) live[j] = __ballot(has[j]) != 0;
    for (int bb = 0; bb < nb; bb += 64) {
        double mine = 0.;
        if (SP == 1 && bb + lane < nb) mine = fm::pow(D[bb + lane], mu_s);
        const int be = bb + 64 < nb ? bb + 64 : nb;
        for (int b = bb; b < be; ++b) {
            const double Db = D[b], dDb = dD[b];
            const double Dmu = SP == 1 ? readlane(mine, b - bb) : 0.;
            double r[NR];
#pragma unroll
            for (int i = 0; i < NR; ++i) r[i] = rows[i * nb + b];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!live[j]) continue;                              // wave-uniform
                const double n = has[j] ? density(j, Db, dDb, Dmu) : 0.;
                add(j, n, r);
            }
        }
    }
}

// bin_loop for a tile of CT channels (include/kidmp_multichannel.h): the tables of the channels lie on the same grids, so
// D, dD, Dmu and the density n are formed once per bin and level group and shared; rows[cc] is channel cc's [NR][nb], and
// add(j, n, r) folds r[cc][NR] of every channel of the tile into the caller's accumulators.  The rows of a tile's unused
// places (the caller points them at a channel in use) are loaded and not read.  With CT == 1 this is bin_loop.
template <int SP, int NJ, int NR, int CT, class F, class G>
__device__ __forceinline__ void bin_loop_multi(const double *__restrict__ D, const double *__restrict__ dD, int nb, const double *const (&rows)[CT],
                                               int lane, const bool (&has)[NJ], F &&density, G &&add)
{
    bool live[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) live[j] = __ballot(has[j]) != 0;
    for (int bb = 0; bb < nb; bb += 64) {
        double mine = 0.;
        if (SP == 1 && bb + lane < nb) mine = fm::pow(D[bb + lane], mu_s);
        const int be = bb + 64 < nb ? bb + 64 : nb;
        for (int b = bb; b < be; ++b) {
            const double Db = D[b], dDb = dD[b];
            const double Dmu = SP == 1 ? readlane(mine, b - bb) : 0.;
            double r[CT][NR];
#pragma unroll
            for (int cc = 0; cc < CT; ++cc)
#pragma unroll
                for (int i = 0; i < NR; ++i) r[cc][i] = rows[cc][i * nb + b];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!live[j]) continue;                              // wave-uniform
                const double n = has[j] ? density(j, Db, dDb, Dmu) : 0.;
                add(j, n, r);
            }
        }
    }
}

// What k_mie_radar, k_radiometer and their multi-channel kernels keep of a column's levels: the load (radar_level), the
// running minimum of the graupel intercept and the parameters of the three size distributions.  Lanes over levels; a level
// past nz holds no species.  What a kernel does not read is not formed.
template <int NJ> struct ChannelLevels {
    double temp[NJ], ze_r[NJ], ze_s[NJ], ze_g[NJ], rho[NJ], rhof[NJ], rs[NJ], rg[NJ], N0_r[NJ], lamr[NJ], N0_g[NJ], lamg[NJ];
    lvl::SnowSpectrum ss[NJ];
    bool lqr[NJ], lqs[NJ], lqg[NJ];
};
template <int NJ, class A>
__device__ __forceinline__ void load_channel_levels(const ReflConsts &c, const DopplerConsts &dc, const A &a, int64_t base, int nz, int lane,
                                                    ChannelLevels<NJ> &L)
{
    double n0[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        L.ze_r[j] = L.ze_s[j] = L.ze_g[j] = 1.E-22;
        L.temp[j] = 0.;
        L.rho[j] = 1.; L.rhof[j] = 0.;
        L.rs[j] = L.rg[j] = R1;
        L.N0_r[j] = L.lamr[j] = 0.;
        L.ss[j] = lvl::SnowSpectrum{0., 0., 0., 0.};
        L.lqr[j] = L.lqs[j] = L.lqg[j] = false;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k >= nz) continue;
        const RadarLevel r = radar_level(c, a, base + k);            // ---- load, M:4991-5028 ----
        L.temp[j] = r.temp;
        L.ze_r[j] = r.ze_rain;
        L.ze_s[j] = r.ze_snow;
        L.rho[j] = r.rho;
        L.rhof[j] = r.rhof;
        L.rs[j] = r.rs;
        L.rg[j] = r.rg;
        L.N0_r[j] = r.N0_r;
        L.lamr[j] = r.lamr;
        L.lqr[j] = r.L_qr; L.lqs[j] = r.L_qs; L.lqg[j] = r.L_qg;
        if (r.L_qs) L.ss[j] = lvl::snow_spectrum(r.sl, lvl::snow_moment(c.sa, c.sb, dc.cse1, r.sl));
        n0[j] = r.n0_exp;
    }
    graupel_running_min<NJ>(n0, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        L.N0_g[j] = L.lamg[j] = 0.;
        if (!L.lqg[j]) continue;
        double ilamg;
        L.ze_g[j] = lvl::graupel_ze(c, n0[j], L.rg[j], ilamg, L.lamg[j], L.N0_g[j]);
    }
}
// rr = qr*rho where rain is present, what scales rain's sums
template <int NJ, class A>
__device__ __forceinline__ void rain_mass(const A &a, int64_t base, int lane, const ChannelLevels<NJ> &L, double (&rr)[NJ])
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) rr[j] = L.lqr[j] ? double(a.qr[base + 64 * j + lane]) * L.rho[j] : 0.;
}

// ---- the cloud radar: what k_mie_radar and k_mie_radar_multi share ----
// One channel's outputs and scalars: a profile of the channel is out[v] + slab where out[v] is not null; k_gas is the
// column's row or null.
template <class T> struct MieChannel {
    T *const *out;
    int64_t slab;
    T *pia_total;
    const T *k_gas;
    double kc, rho_w;
    __device__ __forceinline__ T *profile(int v) const { return out[v] ? out[v] + slab : nullptr; }
};
struct MieWants { bool up, dn, path, ext, all; };
template <class T>
__device__ __forceinline__ MieWants mie_wants(T *const *out, const T *pia_total)
{
    MieWants w;
    w.up = out[MIE_DBZ_UP] || out[MIE_PIA_UP];
    w.dn = out[MIE_DBZ_DOWN] || out[MIE_PIA_DOWN];
    w.path = w.up || w.dn || pia_total;
    w.ext = w.path || out[MIE_EXT];
    w.all = w.ext || out[MIE_DBZ] || out[MIE_VD];                    // what takes every species
    return w;
}
// What a species' five sums (A = sum n s_mie, B = sum n s_ray, E = sum n s_ext, M = sum n mass, V = sum (n s_mie) v0, over
// the bins ascending into accumulators that start at +0.0) leave behind: ze_x' in ze, the species' share of ext and of the
// Doppler sums (where it is present with A above 0), and its own two profiles.
template <class T, int NJ>
__device__ __forceinline__ void mie_species_finish(const bool (&has)[NJ], const double (&rq)[NJ], const double (&A)[NJ], const double (&B)[NJ],
                                                   const double (&E)[NJ], const double (&M)[NJ], const double (&V)[NJ], double (&ze)[NJ],
                                                   double (&ext)[NJ], double (&zw)[NJ], double (&zv)[NJ], T *out_mie, T *out_dbz,
                                                   int64_t base, int nz, int lane)
{
    double mie[NJ], dbz_out[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        mie[j] = has[j] && B[j] > 0. ? A[j] / B[j] : 1.;
        ze[j] = ze[j] * mie[j];
        ext[j] = ext[j] + (has[j] && M[j] > 0. ? rq[j] * E[j] / M[j] : 0.);
        if (has[j] && A[j] > 0.) { zw[j] = zw[j] + ze[j]; zv[j] = zv[j] + ze[j] * (V[j] / A[j]); }
        dbz_out[j] = lvl::dbz_of(ze[j]);
    }
    store_profile<T, NJ>(out_mie, base, nz, lane, mie);
    store_profile<T, NJ>(out_dbz, base, nz, lane, dbz_out);
}
// What follows the species, for one channel: dbz and vd, then ext = ((ext_r + ext_s) + ext_g) + ext_c + k_gas, then the
// path integrals (column_depths); a request ends as early as its outputs allow.  A: MieArgs or MieMultiArgs (qc, w, dz).
template <class T, int NJ, class A>
__device__ __forceinline__ void mie_tail(const A &a, const MieChannel<T> &ch, const MieWants &want, int64_t col, int64_t base, int nz, int lane,
                                         const ChannelLevels<NJ> &L, const double (&ze_r)[NJ], const double (&ze_s)[NJ],
                                         const double (&ze_g)[NJ], double (&ext)[NJ], const double (&zw)[NJ], const double (&zv)[NJ])
{
    double dbz[NJ], vd[NJ], dbz_out[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        dbz[j] = lvl::dbz_of(ze_r[j] + ze_s[j] + ze_g[j]);           // M:5196
        vd[j] = 0.;                                                  // no echo: +0.0, w is not applied
        if (k < nz && zw[j] > 0.) vd[j] = L.rhof[j] * (zv[j] / zw[j]) - (a.w ? double(a.w[base + k]) : 0.);
    }
    store_profile<T, NJ>(ch.profile(MIE_DBZ), base, nz, lane, dbz);
    store_profile<T, NJ>(ch.profile(MIE_VD), base, nz, lane, vd);
    if (!want.ext) return;

    // ---- ext = ((ext_r + ext_s) + ext_g) + ext_c + k_gas; levels past nz keep +0.0 ----
    // cloud water enters through its mass alone, so of load_cloud only the presence test is taken (qc > R1, M:1395): its
    // droplet number, nu_c and lamc would be formed and thrown away
    if (a.qc) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (64 * j + lane >= nz) continue;
            const double qc = double(a.qc[base + 64 * j + lane]);
            if (qc > R1) ext[j] = ext[j] + ch.kc * ((L.rho[j] * qc) / ch.rho_w);
        }
    }
    if (ch.k_gas) {
        const T *__restrict__ kg = ch.k_gas;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (64 * j + lane < nz) ext[j] = ext[j] + double(kg[64 * j + lane]);
    }
    store_profile<T, NJ>(ch.profile(MIE_EXT), base, nz, lane, ext);
    if (!want.path) return;

    // ---- the path: dtau = ext*dz, tau_up = (the levels below) + dtau/2, tau_down from the top ----
    const T *__restrict__ dzc = a.dz + col * a.dz_col_stride;
    double dt[NJ], tu[NJ], td[NJ], total = 0.;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        dt[j] = k < nz ? ext[j] * double(dzc[k]) : 0.;
        total += dt[j];
        tu[j] = td[j] = 0.;
    }
    if (ch.pia_total) {
        total = wave_sum(total);
        if (lane == 0) ch.pia_total[col] = T(MIE_PIA * total);
    }
    if (!(want.up || want.dn)) return;
    column_depths<NJ>(dt, lane, want.up, want.dn, tu, td);
    if (want.up) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) { tu[j] = MIE_PIA * (tu[j] + 0.5 * dt[j]); dbz_out[j] = dbz[j] - tu[j]; }
        store_profile<T, NJ>(ch.profile(MIE_PIA_UP), base, nz, lane, tu);
        store_profile<T, NJ>(ch.profile(MIE_DBZ_UP), base, nz, lane, dbz_out);
    }
    if (want.dn) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) { td[j] = MIE_PIA * (td[j] + 0.5 * dt[j]); dbz_out[j] = dbz[j] - td[j]; }
        store_profile<T, NJ>(ch.profile(MIE_PIA_DOWN), base, nz, lane, td);
        store_profile<T, NJ>(ch.profile(MIE_DBZ_DOWN), base, nz, lane, dbz_out);
    }
}

// The five sums of one species for a tile of CT channels.  Per channel and bin the operations are those of one channel
// alone, in their order: ns = n*s_mie; A += ns; B += n*s_ray; E += n*s_ext; M += n*mass; V += ns*v0.  s_ray, mass and v0
// do not depend on the wavelength, so B and M are formed once, from the rows of the tile's first channel; `used` (wave-
// uniform) is how many of the tile's places hold a channel.
template <int SP, int NJ, int CT, class F>
__device__ __forceinline__ void mie_sums(const double *D, const double *dD, int nb, const double *const (&rows)[CT], int used, int lane,
                                         const bool (&has)[NJ], F &&density, double (&A)[CT][NJ], double (&B)[NJ], double (&E)[CT][NJ],
                                         double (&M)[NJ], double (&V)[CT][NJ])
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        B[j] = M[j] = 0.;
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) A[cc][j] = E[cc][j] = V[cc][j] = 0.;
    }
    bin_loop_multi<SP, NJ, MIE_NROWS, CT>(D, dD, nb, rows, lane, has, density,
                                          [&](int j, double n, const double (&r)[CT][MIE_NROWS]) __attribute__((always_inline)) {
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) {
            if (cc >= used) continue;                                // wave-uniform
            const double ns = n * r[cc][0];
            A[cc][j] += ns;
            if (cc == 0) B[j] += n * r[0][1];
            E[cc][j] += n * r[cc][2];
            if (cc == 0) M[j] += n * r[0][3];
            V[cc][j] += ns * r[0][4];
        }
    });
}

// One wavefront per column: the cloud radar of include/kidmp_mie.h.  The load and the scan are k_doppler_moments'
// (load_channel_levels), lanes over levels.  Then species by species -- rain, snow, graupel -- the five sums over the
// table's bins (mie_sums), which leave behind only mie_x, the species' extinction and its share of the Doppler sums
// (mie_species_finish).  Cloud water (present where qc > R1) and the caller's gas extinction close ext; the path integrals
// are column_depths, the scans of k_lidar_profiles, and a request without them ends before (mie_tail).  No atomics, no
// scratch, nothing but the fastmath tables in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_mie_radar(ReflConsts c, DopplerConsts dc, MieArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    T *const *out = a.out;
    const MieChannel<T> ch{out, 0, a.pia_total, a.k_gas ? a.k_gas + col * a.k_gas_col_stride : nullptr, a.kc, a.rho_w};
    const MieWants want = mie_wants<T>(out, a.pia_total);
    const auto wants = [&](int x) __attribute__((always_inline)) { return want.all || out[MIE_DBZ_X + x] || out[MIE_MIE_X + x]; };

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);

    // what the species leave behind: ze_x' in ze_x, ext = (ext_r + ext_s) + ext_g, and the Doppler sums over the species
    // that are present with A above 0
    double ext[NJ], zw[NJ], zv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) ext[j] = zw[j] = zv[j] = 0.;
    double A[1][NJ], B[NJ], E[1][NJ], M[NJ], V[1][NJ];
    if (wants(0)) {
        double rr[NJ];
        rain_mass<NJ>(a, base, lane, L, rr);
        const double *const rows[1] = {a.rows[0]};
        mie_sums<0, NJ, 1>(a.D[0], a.dD[0], a.nb[0], rows, 1, lane, L.lqr,
                           [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); },
                           A, B, E, M, V);
        mie_species_finish<T, NJ>(L.lqr, rr, A[0], B, E[0], M, V[0], L.ze_r, ext, zw, zv, out[MIE_MIE_X + 0], out[MIE_DBZ_X + 0], base, nz, lane);
    }
    if (wants(1)) {
        const double *const rows[1] = {a.rows[1]};
        mie_sums<1, NJ, 1>(a.D[1], a.dD[1], a.nb[1], rows, 1, lane, L.lqs,
                           [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); },
                           A, B, E, M, V);
        mie_species_finish<T, NJ>(L.lqs, L.rs, A[0], B, E[0], M, V[0], L.ze_s, ext, zw, zv, out[MIE_MIE_X + 1], out[MIE_DBZ_X + 1], base, nz, lane);
    }
    if (wants(2)) {
        const double *const rows[1] = {a.rows[2]};
        mie_sums<2, NJ, 1>(a.D[2], a.dD[2], a.nb[2], rows, 1, lane, L.lqg,
                           [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); },
                           A, B, E, M, V);
        mie_species_finish<T, NJ>(L.lqg, L.rg, A[0], B, E[0], M, V[0], L.ze_g, ext, zw, zv, out[MIE_MIE_X + 2], out[MIE_DBZ_X + 2], base, nz, lane);
    }
    if (!want.all) return;                                           // wave-uniform: one species' own profiles alone
    mie_tail<T, NJ>(a, ch, want, col, base, nz, lane, L, L.ze_r, L.ze_s, L.ze_g, ext, zw, zv);
}

// One wavefront per column: nch channels of the cloud radar (include/kidmp_multichannel.h).  The load is formed once; the
// channels are taken in tiles of CT, and per tile and species one walk over the bins forms every density once and folds
// it into the sums of the tile's channels (mie_sums).  What stays alive per channel across the species is ze_r', ze_s',
// ze_g', ext and the two Doppler sums; mie_species_finish and mie_tail then run per channel as in k_mie_radar, so slab c
// of every output holds k_mie_radar's bits for channel c's table.  No atomics, no scratch.
template <class T, int NJ, int CT>
__global__ void __launch_bounds__(REFL_THREADS)
k_mie_radar_multi(ReflConsts c, DopplerConsts dc, MieMultiArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    const MieWants want = mie_wants<T>(a.out, a.pia_total);
    const auto wants = [&](int x) __attribute__((always_inline)) { return want.all || a.out[MIE_DBZ_X + x] || a.out[MIE_MIE_X + x]; };

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);
    double rr[NJ];
    rain_mass<NJ>(a, base, lane, L, rr);

    for (int c0 = 0; c0 < a.nch; c0 += CT) {
        const int used = a.nch - c0 < CT ? a.nch - c0 : CT;
        double ze_r[CT][NJ], ze_s[CT][NJ], ze_g[CT][NJ], ext[CT][NJ], zw[CT][NJ], zv[CT][NJ];
#pragma unroll
        for (int cc = 0; cc < CT; ++cc)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                ze_r[cc][j] = L.ze_r[j]; ze_s[cc][j] = L.ze_s[j]; ze_g[cc][j] = L.ze_g[j];
                ext[cc][j] = zw[cc][j] = zv[cc][j] = 0.;
            }
        double A[CT][NJ], B[NJ], E[CT][NJ], M[NJ], V[CT][NJ];
        const auto rows_of = [&](int x, const double *(&rows)[CT]) __attribute__((always_inline)) {
#pragma unroll
            for (int cc = 0; cc < CT; ++cc) rows[cc] = a.rows[c0 + (cc < used ? cc : 0)][x];
        };
        const auto finish = [&](int x, const bool (&has)[NJ], const double (&rq)[NJ], double (&ze)[CT][NJ]) __attribute__((always_inline)) {
#pragma unroll
            for (int cc = 0; cc < CT; ++cc) {
                if (cc >= used) continue;                            // wave-uniform
                const int64_t slab = int64_t(c0 + cc) * a.prof_ch_stride;
                T *const om = a.out[MIE_MIE_X + x], *const od = a.out[MIE_DBZ_X + x];
                mie_species_finish<T, NJ>(has, rq, A[cc], B, E[cc], M, V[cc], ze[cc], ext[cc], zw[cc], zv[cc], om ? om + slab : nullptr,
                                          od ? od + slab : nullptr, base, nz, lane);
            }
        };
        const double *rows[CT];
        if (wants(0)) {
            rows_of(0, rows);
            mie_sums<0, NJ, CT>(a.D[0], a.dD[0], a.nb[0], rows, used, lane, L.lqr,
                                [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); },
                                A, B, E, M, V);
            finish(0, L.lqr, rr, ze_r);
        }
        if (wants(1)) {
            rows_of(1, rows);
            mie_sums<1, NJ, CT>(a.D[1], a.dD[1], a.nb[1], rows, used, lane, L.lqs,
                                [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); },
                                A, B, E, M, V);
            finish(1, L.lqs, L.rs, ze_s);
        }
        if (wants(2)) {
            rows_of(2, rows);
            mie_sums<2, NJ, CT>(a.D[2], a.dD[2], a.nb[2], rows, used, lane, L.lqg,
                                [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); },
                                A, B, E, M, V);
            finish(2, L.lqg, L.rg, ze_g);
        }
        if (!want.all) continue;                                     // wave-uniform: one species' own profiles alone
        // the tail once in the code, channel after channel: the channel's registers are picked by wave-uniform selects
#pragma unroll 1
        for (int cc = 0; cc < used; ++cc) {
            double zr[NJ], zs[NJ], zg[NJ], ex[NJ], w1[NJ], v1[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                zr[j] = ze_r[0][j]; zs[j] = ze_s[0][j]; zg[j] = ze_g[0][j]; ex[j] = ext[0][j]; w1[j] = zw[0][j]; v1[j] = zv[0][j];
#pragma unroll
                for (int u = 1; u < CT; ++u)
                    if (u == cc) { zr[j] = ze_r[u][j]; zs[j] = ze_s[u][j]; zg[j] = ze_g[u][j]; ex[j] = ext[u][j]; w1[j] = zw[u][j]; v1[j] = zv[u][j]; }
            }
            const int ci = c0 + cc;
            const MieChannel<T> ch{a.out, int64_t(ci) * a.prof_ch_stride, a.pia_total ? a.pia_total + int64_t(ci) * a.col_ch_stride : nullptr,
                                   a.k_gas ? a.k_gas + int64_t(ci) * a.k_gas_ch_stride + col * a.k_gas_col_stride : nullptr, a.kc[ci], a.rho_w[ci]};
            mie_tail<T, NJ>(a, ch, want, col, base, nz, lane, L, zr, zs, zg, ex, w1, v1);
        }
    }
}

// ---- the microwave radiometer (include/kidmp_radiometer.h) ----
__device__ __forceinline__ RadState state_readlane(const RadState &v, int l)
{ return RadState{readlane(v.Rt, l), readlane(v.Rb, l), readlane(v.T, l), readlane(v.Eu, l), readlane(v.Ed, l)}; }
template <bool DOWN>
__device__ __forceinline__ RadState state_shift(const RadState &v, int d)
{
    return DOWN ? RadState{__shfl_down(v.Rt, d, 64), __shfl_down(v.Rb, d, 64), __shfl_down(v.T, d, 64), __shfl_down(v.Eu, d, 64), __shfl_down(v.Ed, d, 64)}
                : RadState{__shfl_up(v.Rt, d, 64), __shfl_up(v.Rb, d, 64), __shfl_up(v.T, d, 64), __shfl_up(v.Eu, d, 64), __shfl_up(v.Ed, d, 64)};
}
__device__ __forceinline__ RadState state_select(bool c, const RadState &a, const RadState &b)
{ return RadState{c ? a.Rt : b.Rt, c ? a.Rb : b.Rb, c ? a.T : b.T, c ? a.Eu : b.Eu, c ? a.Ed : b.Ed}; }
// Inclusive scan over the wave with the adding of layers in place of a sum: Kogge-Stone over __shfl_up, of the shape of
// wave_prefix_sum.  The operator is associative but not commutative: the lower stack always comes first.  Lane l receives
// the stack of the levels 0..l of its group, in an order that l alone fixes; DOWN is the mirror image over __shfl_down and
// gives the levels l..63.  A lane without a partner keeps its value (what it computed from the shuffle's own-lane return
// is thrown away).  Whole wavefronts only.
template <bool DOWN>
__device__ __forceinline__ RadState wave_adding_scan(RadState v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const RadState o = state_shift<DOWN>(v, d);
        const RadState c = DOWN ? rad_combine(v, o) : rad_combine(o, v);
        v = state_select(DOWN ? lane + d < 64 : lane >= d, c, v);
    }
    return v;
}

// ---- what k_radiometer and k_radiometer_multi share ----
// One channel's outputs and scalars: a profile of the channel is out[v] + slab where out[v] is not null; k_gas is the
// column's row or null.
template <class T> struct RadChannel {
    T *const *out;
    int64_t slab;
    T *tb_toa, *tb_ground, *tau_abs;
    const T *k_gas;
    double kc, rho_w, mu, emissivity, t_cosmic;
    __device__ __forceinline__ T *profile(int v) const { return out[v] ? out[v] + slab : nullptr; }
};
// The three sums of one species for a tile of CT channels.  Per channel and bin the operations are those of one channel
// alone: A += n*s_abs; S += n*s_bsc; M += n*mass.  The mass row does not depend on the wavelength, so M is formed once,
// from the rows of the tile's first channel; `used` (wave-uniform) is how many of the tile's places hold a channel.
template <int SP, int NJ, int CT, class F>
__device__ __forceinline__ void radiometer_sums(const double *D, const double *dD, int nb, const double *const (&rows)[CT], int used, int lane,
                                                const bool (&has)[NJ], F &&density, double (&A)[CT][NJ], double (&S)[CT][NJ], double (&M)[NJ])
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        M[j] = 0.;
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) A[cc][j] = S[cc][j] = 0.;
    }
    bin_loop_multi<SP, NJ, RAD_NROWS, CT>(D, dD, nb, rows, lane, has, density,
                                          [&](int j, double n, const double (&r)[CT][RAD_NROWS]) __attribute__((always_inline)) {
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) {
            if (cc >= used) continue;                                // wave-uniform
            A[cc][j] += n * r[cc][0];
            S[cc][j] += n * r[cc][1];
            if (cc == 0) M[j] += n * r[0][2];
        }
    });
}
// a species' carriers abs_x = (rho*q_x)*A/M and bsc_x = (rho*q_x)*S/M, added to k_abs and k_bsc
template <int NJ>
__device__ __forceinline__ void radiometer_species_finish(const bool (&has)[NJ], const double (&rq)[NJ], const double (&A)[NJ],
                                                          const double (&S)[NJ], const double (&M)[NJ], double (&kabs)[NJ], double (&kbsc)[NJ])
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const bool ok = has[j] && M[j] > 0.;
        kabs[j] = kabs[j] + (ok ? rq[j] * A[j] / M[j] : 0.);
        kbsc[j] = kbsc[j] + (ok ? rq[j] * S[j] / M[j] : 0.);
    }
}
// What follows the species, for one channel: cloud water and the caller's gas absorption close k_abs; the layers follow per
// level (kidmp_radiometer_layer.h).  The stacks above every level come from a suffix scan of the layers, the level groups
// chained from the top through a wave-uniform carry state as column_depths chains its sums; the stacks below from the
// prefix scan, group by group, each group's brightness temperatures stored before the next is scanned, so that only the
// suffix states stay alive across groups.  A request without a brightness temperature ends before the scans, one without
// refl, trans either before the exponentials.  A: RadiometerArgs or RadiometerMultiArgs (qc, dz, t_sfc, t).
template <class T, int NJ, class A>
__device__ __forceinline__ void radiometer_tail(const A &a, const RadChannel<T> &ch, int64_t col, int64_t base, int nz, int lane,
                                                const ChannelLevels<NJ> &L, double (&kabs)[NJ], const double (&kbsc)[NJ])
{
    T *const tb_up = ch.profile(RAD_TB_UP), *const tb_down = ch.profile(RAD_TB_DOWN);
    const bool want_tb = tb_up || tb_down || ch.tb_toa || ch.tb_ground;
    const bool want_layer = want_tb || ch.profile(RAD_REFL) || ch.profile(RAD_TRANS);
    if (a.qc) {                                                      // present where qc > R1, as in k_mie_radar
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (64 * j + lane >= nz) continue;
            const double qc = double(a.qc[base + 64 * j + lane]);
            if (qc > R1) kabs[j] = kabs[j] + ch.kc * ((L.rho[j] * qc) / ch.rho_w);
        }
    }
    if (ch.k_gas) {
        const T *__restrict__ kg = ch.k_gas;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (64 * j + lane < nz) kabs[j] = kabs[j] + double(kg[64 * j + lane]);
    }
    store_profile<T, NJ>(ch.profile(RAD_K_ABS), base, nz, lane, kabs);
    store_profile<T, NJ>(ch.profile(RAD_K_BSC), base, nz, lane, kbsc);
    if (!(want_layer || ch.tau_abs)) return;                         // wave-uniform: the optics alone

    const T *__restrict__ dzc = a.dz + col * a.dz_col_stride;
    double ta[NJ], bs[NJ], total = 0.;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        const double dz = k < nz ? double(dzc[k]) : 0.;
        ta[j] = k < nz ? kabs[j] * dz : 0.;
        bs[j] = k < nz ? kbsc[j] * dz : 0.;
        total += ta[j];
    }
    if (ch.tau_abs) {
        total = wave_sum(total);
        if (lane == 0) ch.tau_abs[col] = T(total);
    }
    if (!want_layer) return;

    // ---- the layer of every level; a level past nz is the identity ----
    double lr[NJ], lt[NJ], le[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const double x = rad_layer_x(ta[j], bs[j]), y = x / ch.mu;
        const double e = lvl::exp_neg(y), f = y * lvl::layer_mean(y);
        const RadLayer l = rad_layer(ta[j], bs[j], x, ch.mu, e, f);
        lr[j] = l.R; lt[j] = l.T; le[j] = l.a * L.temp[j];
    }
    store_profile<T, NJ>(ch.profile(RAD_REFL), base, nz, lane, lr);
    store_profile<T, NJ>(ch.profile(RAD_TRANS), base, nz, lane, lt);
    if (!want_tb) return;

    // ---- the stack above every level: suffix scan, chained from the top ----
    RadState above[NJ];
    {
        RadState carry = rad_identity();
#pragma unroll
        for (int j = NJ - 1; j >= 0; --j) {
            const RadState inc = wave_adding_scan<true>(RadState{lr[j], lr[j], lt[j], le[j], le[j]}, lane);
            const RadState first = state_readlane(inc, 0);
            const RadState next = state_shift<true>(inc, 1);
            above[j] = state_select(lane < 63, rad_combine(next, carry), carry);
            carry = rad_combine(first, carry);
        }
    }
    // ---- the stack below, group by group, and the closure at the level's two faces ----
    const double ts = a.t_sfc ? double(a.t_sfc[col]) : double(a.t[base]);
    const double rsfc = 1. - ch.emissivity;
    RadState carry = rad_identity();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const RadState own{lr[j], lr[j], lt[j], le[j], le[j]};
        const RadState inc = wave_adding_scan<false>(own, lane);
        const RadState last = state_readlane(inc, 63);
        const RadState prev = state_shift<false>(inc, 1);
        const RadState below = state_select(lane > 0, rad_combine(carry, prev), carry);
        carry = rad_combine(carry, last);
        const int k = 64 * j + lane;
        if (k >= nz) continue;
        const double up = rad_face(rad_combine(below, own), above[j], ch.emissivity, rsfc, ts, ch.t_cosmic).up;
        const double down = rad_face(below, rad_combine(own, above[j]), ch.emissivity, rsfc, ts, ch.t_cosmic).down;
        if (tb_up) tb_up[base + k] = T(up);
        if (tb_down) tb_down[base + k] = T(down);
        if (ch.tb_toa && k == nz - 1) ch.tb_toa[col] = T(up);
        if (ch.tb_ground && k == 0) ch.tb_ground[col] = T(down);
    }
}

// One wavefront per column: the radiometer of include/kidmp_radiometer.h.  The load is k_mie_radar's (load_channel_levels),
// lanes over levels.  Then species by species the three sums over the table's bins (radiometer_sums), which leave behind
// only k_abs and k_bsc; the rest is radiometer_tail.  No atomics, no scratch, nothing but the fastmath tables in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_radiometer(ReflConsts c, DopplerConsts dc, RadiometerArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    const RadChannel<T> ch{a.out, 0, a.tb_toa, a.tb_ground, a.tau_abs, a.k_gas ? a.k_gas + col * a.k_gas_col_stride : nullptr,
                           a.kc, a.rho_w, a.mu, a.emissivity, a.t_cosmic};

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);

    // ---- k_abs = (((abs_r + abs_s) + abs_g) + abs_c) + k_gas, k_bsc = (bsc_r + bsc_s) + bsc_g; levels past nz keep +0.0 ----
    double kabs[NJ], kbsc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) kabs[j] = kbsc[j] = 0.;
    {
        double A[1][NJ], S[1][NJ], M[NJ], rr[NJ];
        rain_mass<NJ>(a, base, lane, L, rr);
        const double *const rows_r[1] = {a.rows[0]}, *const rows_s[1] = {a.rows[1]}, *const rows_g[1] = {a.rows[2]};
        radiometer_sums<0, NJ, 1>(a.D[0], a.dD[0], a.nb[0], rows_r, 1, lane, L.lqr,
                                  [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); }, A, S, M);
        radiometer_species_finish<NJ>(L.lqr, rr, A[0], S[0], M, kabs, kbsc);
        radiometer_sums<1, NJ, 1>(a.D[1], a.dD[1], a.nb[1], rows_s, 1, lane, L.lqs,
                                  [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); }, A, S, M);
        radiometer_species_finish<NJ>(L.lqs, L.rs, A[0], S[0], M, kabs, kbsc);
        radiometer_sums<2, NJ, 1>(a.D[2], a.dD[2], a.nb[2], rows_g, 1, lane, L.lqg,
                                  [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); }, A, S, M);
        radiometer_species_finish<NJ>(L.lqg, L.rg, A[0], S[0], M, kabs, kbsc);
    }
    radiometer_tail<T, NJ>(a, ch, col, base, nz, lane, L, kabs, kbsc);
}

// One wavefront per column: nch channels of the radiometer (include/kidmp_multichannel.h).  The load is formed once; the
// channels are taken in tiles of CT, and per tile and species one walk over the bins forms every density once and folds
// it into the sums of the tile's channels (radiometer_sums).  What stays alive per channel across the species is k_abs and
// k_bsc; radiometer_tail then runs per channel as in k_radiometer, so slab c of every output holds k_radiometer's bits
// for channel c's table, closure and k_gas.  No atomics, no scratch.
template <class T, int NJ, int CT>
__global__ void __launch_bounds__(REFL_THREADS)
k_radiometer_multi(ReflConsts c, DopplerConsts dc, RadiometerMultiArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);
    double rr[NJ];
    rain_mass<NJ>(a, base, lane, L, rr);

    for (int c0 = 0; c0 < a.nch; c0 += CT) {
        const int used = a.nch - c0 < CT ? a.nch - c0 : CT;
        double kabs[CT][NJ], kbsc[CT][NJ];
#pragma unroll
        for (int cc = 0; cc < CT; ++cc)
#pragma unroll
            for (int j = 0; j < NJ; ++j) kabs[cc][j] = kbsc[cc][j] = 0.;
        {
            double A[CT][NJ], S[CT][NJ], M[NJ];
            const double *rows[CT];
            const auto rows_of = [&](int x) __attribute__((always_inline)) {
#pragma unroll
                for (int cc = 0; cc < CT; ++cc) rows[cc] = a.rows[c0 + (cc < used ? cc : 0)][x];
            };
            const auto finish = [&](const bool (&has)[NJ], const double (&rq)[NJ]) __attribute__((always_inline)) {
#pragma unroll
                for (int cc = 0; cc < CT; ++cc)
                    if (cc < used) radiometer_species_finish<NJ>(has, rq, A[cc], S[cc], M, kabs[cc], kbsc[cc]);
            };
            rows_of(0);
            radiometer_sums<0, NJ, CT>(a.D[0], a.dD[0], a.nb[0], rows, used, lane, L.lqr,
                                       [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); }, A, S, M);
            finish(L.lqr, rr);
            rows_of(1);
            radiometer_sums<1, NJ, CT>(a.D[1], a.dD[1], a.nb[1], rows, used, lane, L.lqs,
                                       [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); }, A, S, M);
            finish(L.lqs, L.rs);
            rows_of(2);
            radiometer_sums<2, NJ, CT>(a.D[2], a.dD[2], a.nb[2], rows, used, lane, L.lqg,
                                       [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); }, A, S, M);
            finish(L.lqg, L.rg);
        }
        // the tail once in the code, channel after channel: the channel's registers are picked by wave-uniform selects
#pragma unroll 1
        for (int cc = 0; cc < used; ++cc) {
            double ka[NJ], kb[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                ka[j] = kabs[0][j]; kb[j] = kbsc[0][j];
#pragma unroll
                for (int u = 1; u < CT; ++u)
                    if (u == cc) { ka[j] = kabs[u][j]; kb[j] = kbsc[u][j]; }
            }
            const int ci = c0 + cc;
            const int64_t cslab = int64_t(ci) * a.col_ch_stride;
            const RadChannel<T> ch{a.out, int64_t(ci) * a.prof_ch_stride, a.tb_toa ? a.tb_toa + cslab : nullptr,
                                   a.tb_ground ? a.tb_ground + cslab : nullptr, a.tau_abs ? a.tau_abs + cslab : nullptr,
                                   a.k_gas ? a.k_gas + int64_t(ci) * a.k_gas_ch_stride + col * a.k_gas_col_stride : nullptr,
                                   a.kc[ci], a.rho_w[ci], a.mu[ci], a.emissivity[ci], a.t_cosmic[ci]};
            radiometer_tail<T, NJ>(a, ch, col, base, nz, lane, L, ka, kb);
        }
    }
}

// ---- the polarimetric radar (include/kidmp_polarimetric.h) ----
// One wavefront per column.  The load and the scan are k_mie_radar's (radar_level, graupel_running_min), lanes over
// levels.  Then species by species -- rain, snow, graupel -- the seven sums over the table's bins (bin_loop), which leave
// behind only the species' share of Zh, Zv, C and kdp.  A uniform species (a.uniform[x], wave-uniform) walks no bins and
// forms no density: the table's scalars stand in for the ratios of its sums.  A request for one species' own profiles alone
// walks that species only.  No atomics, no scratch, no scan but the graupel minimum, nothing but the fastmath tables in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_polarimetric(ReflConsts c, DopplerConsts dc, PolArgs<T> a, int64_t ncol, int nz)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the scan needs every lane
    const int64_t base = col * int64_t(nz);
    T *const *out = a.out;
    const bool all = out[POL_DBZ_H] || out[POL_ZDR] || out[POL_KDP] || out[POL_RHOHV];   // what takes every species
    const auto wants = [&](int x) __attribute__((always_inline)) { return all || out[POL_DBZ_H_X + x] || out[POL_ZDR_X + x] || out[POL_KDP_X + x]; };

    double ze_r[NJ], ze_s[NJ], ze_g[NJ], rho[NJ], rs[NJ], rg[NJ], n0[NJ], N0_r[NJ], lamr[NJ];
    lvl::SnowSpectrum ss[NJ];
    bool lqr[NJ], lqs[NJ], lqg[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        ze_r[j] = ze_s[j] = ze_g[j] = 1.E-22;
        rho[j] = 1.;
        rs[j] = rg[j] = R1;
        N0_r[j] = lamr[j] = 0.;
        ss[j] = lvl::SnowSpectrum{0., 0., 0., 0.};
        lqr[j] = lqs[j] = lqg[j] = false;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k >= nz) continue;
        const RadarLevel r = radar_level(c, a, base + k);            // ---- load, M:4991-5028 ----
        ze_r[j] = r.ze_rain;
        ze_s[j] = r.ze_snow;
        rho[j] = r.rho;
        rs[j] = r.rs;
        rg[j] = r.rg;
        N0_r[j] = r.N0_r;
        lamr[j] = r.lamr;
        lqr[j] = r.L_qr; lqs[j] = r.L_qs; lqg[j] = r.L_qg;
        if (r.L_qs && !a.uniform[1]) ss[j] = lvl::snow_spectrum(r.sl, lvl::snow_moment(c.sa, c.sb, dc.cse1, r.sl));
        n0[j] = r.n0_exp;
    }
    graupel_running_min<NJ>(n0, lane);
    double N0_g[NJ], lamg[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        N0_g[j] = lamg[j] = 0.;
        if (!lqg[j]) continue;
        double ilamg;
        ze_g[j] = lvl::graupel_ze(c, n0[j], rg[j], ilamg, lamg[j], N0_g[j]);
    }

    // what the species leave behind: Zh = (zh_r + zh_s) + zh_g, Zv, C and kdp likewise
    double Zh[NJ], Zv[NJ], Cr[NJ], Ci[NJ], Kd[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) Zh[j] = Zv[j] = Cr[j] = Ci[j] = Kd[j] = 0.;
    double H[NJ], V[NJ], Xr[NJ], Xi[NJ], S[NJ], K[NJ], M[NJ];
    const auto zero = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) H[j] = V[j] = Xr[j] = Xi[j] = S[j] = K[j] = M[j] = 0.;
    };
    const auto add = [&](int j, double n, const double (&r)[POL_NROWS]) __attribute__((always_inline)) {
        H[j] += n * r[0];
        V[j] += n * r[1];
        Xr[j] += n * r[2];
        Xi[j] += n * r[3];
        S[j] += n * r[4];
        K[j] += n * r[5];
        M[j] += n * r[6];
    };
    const auto finish = [&](int x, const bool (&has)[NJ], const double (&ze)[NJ], const double (&rq)[NJ]) __attribute__((always_inline)) {
        const bool uni = a.uniform[x] != 0;                          // wave-uniform
        double o_dbz[NJ], o_zdr[NJ], o_kdp[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            double rh = 1., rv = 1., rcr = 1., rci = 0., rk = 0.;
            if (uni) {
                if (has[j]) { rh = a.scal[x][0]; rv = a.scal[x][1]; rcr = a.scal[x][2]; rci = a.scal[x][3]; rk = a.scal[x][4]; }
            } else {
                if (has[j] && S[j] > 0.) { rh = H[j] / S[j]; rv = V[j] / S[j]; rcr = Xr[j] / S[j]; rci = Xi[j] / S[j]; }
                if (has[j] && M[j] > 0.) rk = K[j] / M[j];
            }
            const double zh = ze[j] * rh, zv = ze[j] * rv;
            const double kd = has[j] ? (a.kfac * rq[j]) * rk : 0.;
            Zh[j] = Zh[j] + zh;
            Zv[j] = Zv[j] + zv;
            Cr[j] = Cr[j] + ze[j] * rcr;
            Ci[j] = Ci[j] + ze[j] * rci;
            Kd[j] = Kd[j] + kd;
            o_dbz[j] = lvl::dbz_of(zh);
            o_zdr[j] = 10. * fm::log10(zh / zv);
            o_kdp[j] = kd;
        }
        store_profile<T, NJ>(out[POL_DBZ_H_X + x], base, nz, lane, o_dbz);
        store_profile<T, NJ>(out[POL_ZDR_X + x], base, nz, lane, o_zdr);
        store_profile<T, NJ>(out[POL_KDP_X + x], base, nz, lane, o_kdp);
    };
    if (wants(0)) {
        double rr[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) rr[j] = lqr[j] ? double(a.qr[base + 64 * j + lane]) * rho[j] : 0.;
        if (!a.uniform[0]) {
            zero();
            bin_loop<0, NJ, POL_NROWS>(a, lane, lqr, [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(N0_r[j], lamr[j], D, dD); }, add);
        }
        finish(0, lqr, ze_r, rr);
    }
    if (wants(1)) {
        if (!a.uniform[1]) {
            zero();
            bin_loop<1, NJ, POL_NROWS>(a, lane, lqs, [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(ss[j], D, Dmu, dD); }, add);
        }
        finish(1, lqs, ze_s, rs);
    }
    if (wants(2)) {
        if (!a.uniform[2]) {
            zero();
            bin_loop<2, NJ, POL_NROWS>(a, lane, lqg, [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(N0_g[j], lamg[j], D, dD); }, add);
        }
        finish(2, lqg, ze_g, rg);
    }
    if (!all) return;                                                // wave-uniform: one species' own profiles alone

    double dbz[NJ], zdr[NJ], rhohv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        dbz[j] = lvl::dbz_of(Zh[j]);                                 // M:5196
        zdr[j] = 10. * fm::log10(Zh[j] / Zv[j]);
        rhohv[j] = fmin(1., fm::sqrt_pos(Cr[j] * Cr[j] + Ci[j] * Ci[j]) / fm::sqrt_pos(Zh[j] * Zv[j]));
    }
    store_profile<T, NJ>(out[POL_DBZ_H], base, nz, lane, dbz);
    store_profile<T, NJ>(out[POL_ZDR], base, nz, lane, zdr);
    store_profile<T, NJ>(out[POL_KDP], base, nz, lane, Kd);
    store_profile<T, NJ>(out[POL_RHOHV], base, nz, lane, rhohv);
}

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

// One wavefront per column: the 15 numbers of include/kidmp_summary.h from one read of the column, no profile written.
// dBZ and re_qc of every level are those of k_reflectivity and k_effective_radii (the same functions on the same
// operands) and stay in registers.  Every sum is a per-lane sum over the level groups in ascending order followed by
// wave_sum: an order fixed by nz alone.  Levels are chosen with ballots, heights are masked sums of dz.  Lanes 0-15
// store the column's 16 doubles as one 128-byte line.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_column_summary(ReflConsts c, RadConsts rc, SummaryArgs<T> a, int64_t ncol, int nz, double *__restrict__ summary)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only
    const int64_t base = col * int64_t(nz);
    const double Nt_c = a.set_nc_col ? a.set_nc_col[col] * 1.e6 : rc.Nt_c;
    const T *__restrict__ dzc = a.dz + col * a.dz_col_stride;

    double dbz[NJ], dz[NJ], sum[7] = {0., 0., 0., 0., 0., 0., 0.};   // WVP, CWP, RWP, IWP, SWP, GWP, TAU_C of the lane
    bool cloudy[NJ], frozen[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { dbz[j] = -double(__builtin_inf()); dz[j] = 0.; cloudy[j] = frozen[j] = false; }
    column_dbz<T, NJ>(c, nz, lane, base, a.t, a.p, a.qv, a.qr, a.nr, a.qs, a.qg, dbz,
                      [&](int j, int64_t i, double temp, double pres, double qv_in, double qv, double rho, double qs, bool,
                          const lvl::SnowLevel &) __attribute__((always_inline)) {
                          const double qc = double(a.qc[i]), qi = a.qi ? double(a.qi[i]) : 0.;
                          const double h = double(dzc[i - base]);
                          dz[j] = h;
                          const double cw = rho * qc * h;
                          sum[0] += rho * qv * h;
                          sum[1] += cw;
                          sum[2] += rho * double(a.qr[i]) * h;
                          sum[3] += rho * qi * h;
                          sum[4] += rho * qs * h;
                          sum[5] += rho * (a.qg ? double(a.qg[i]) : 0.) * h;
                          double re;                                 // calc_effectRad's own density: qv unclamped, M:4860
                          const double rho_r = qv_in == qv ? rho : lvl::air_density(pres, temp, qv_in);
                          if (lvl::cloud_water_radius(rc, Nt_c, rho_r, qc, a.nc ? double(a.nc[i]) : 0., re))
                              sum[6] += 1.5 * cw / (1000.0 * re);
                          cloudy[j] = qc + qi > a.q_cloud;
                          frozen[j] = temp < a.t_freeze;
                      });
#pragma unroll
    for (int s = 0; s < 7; ++s) sum[s] = wave_sum(sum[s]);

    const double nan = __builtin_nan("");
    double lmax = dbz[0];
#pragma unroll
    for (int j = 1; j < NJ; ++j) lmax = fmax(lmax, dbz[j]);
    const double dbz_max = wave_max(lmax);
    bool at_max[NJ], echo[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { at_max[j] = dbz[j] == dbz_max; echo[j] = dbz[j] >= a.dbz_echo; }   // false past nz: -inf
    int n_cloud, n_echo;
    const int k_max = lowest_level<NJ>(at_max), k_echo = highest_level<NJ>(echo, n_echo);
    const int k_base = lowest_level<NJ>(cloudy), k_top = highest_level<NJ>(cloudy, n_cloud), k_frz = lowest_level<NJ>(frozen);
    // k_max < 0 only for NaN input: the slot is then NaN, and no index is formed from it
    const double z_max = k_max < 0 ? nan : height_below<NJ>(dz, lane, k_max) + 0.5 * level_of<NJ>(dz, k_max);
    const double z_echo = k_echo < 0 ? nan : height_below<NJ>(dz, lane, k_echo + 1);
    const double z_base = k_base < 0 ? nan : height_below<NJ>(dz, lane, k_base);
    const double z_top = k_top < 0 ? nan : height_below<NJ>(dz, lane, k_top + 1);
    const double z_frz = k_frz < 0 ? nan : height_below<NJ>(dz, lane, k_frz) + 0.5 * level_of<NJ>(dz, k_frz);
    const double dbz_sfc = readlane(dbz[0], 0);

    const double slot[SUMMARY_N] = {sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], dbz_max, z_max, z_echo, dbz_sfc,
                                    z_base, z_top, double(n_cloud), z_frz, 0.};
    double out = slot[0];
#pragma unroll
    for (int s = 1; s < SUMMARY_N; ++s) out = lane == s ? slot[s] : out;
    if (lane < SUMMARY_N) summary[col * SUMMARY_N + lane] = out;
}

namespace {

// rad null: k_reflectivity; else k_column_outputs
template <class T, int NJ>
hipError_t launch_nj(const ReflConsts &c, const RadiiArgs<T> *rad, int64_t ncol, int nz, const T *t, const T *p,
                     const T *qv, const T *qr, const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t s)
{
    const int64_t nblk = (ncol + REFL_WAVES - 1) / REFL_WAVES;
    if (rad)
        hipLaunchKernelGGL((k_column_outputs<T, NJ>), dim3((unsigned)nblk), dim3(REFL_THREADS), 0, s, c, *rad, ncol, nz, t,
                           p, qv, qr, nr, qs, qg, dbz);
    else
        hipLaunchKernelGGL((k_reflectivity<T, NJ>), dim3((unsigned)nblk), dim3(REFL_THREADS), 0, s, c, ncol, nz, t, p, qv,
                           qr, nr, qs, qg, dbz);
    return hipGetLastError();
}

template <class T>
hipError_t launch_any(const ReflConsts &c, const RadiiArgs<T> *rad, int64_t ncol, int nz, const T *t, const T *p,
                      const T *qv, const T *qr, const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    switch ((nz + 63) / 64) {
    case 1: return launch_nj<T, 1>(c, rad, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    case 2: return launch_nj<T, 2>(c, rad, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    case 3: return launch_nj<T, 3>(c, rad, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    case 4: return launch_nj<T, 4>(c, rad, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

template <class T>
hipError_t launch_column_summary(const ReflConsts &c, const RadConsts &rc, int64_t ncol, int nz, const SummaryArgs<T> &a,
                                 double *summary, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_column_summary<T, 1>), grid, block, 0, s, c, rc, a, ncol, nz, summary); break;
    case 2: hipLaunchKernelGGL((k_column_summary<T, 2>), grid, block, 0, s, c, rc, a, ncol, nz, summary); break;
    case 3: hipLaunchKernelGGL((k_column_summary<T, 3>), grid, block, 0, s, c, rc, a, ncol, nz, summary); break;
    case 4: hipLaunchKernelGGL((k_column_summary<T, 4>), grid, block, 0, s, c, rc, a, ncol, nz, summary); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_column_summary<double>(const ReflConsts &, const RadConsts &, int64_t, int, const SummaryArgs<double> &,
                                                  double *, hipStream_t);
template hipError_t launch_column_summary<float>(const ReflConsts &, const RadConsts &, int64_t, int, const SummaryArgs<float> &,
                                                 double *, hipStream_t);

template <class T>
hipError_t launch_fall_speeds(const Consts *c, int64_t ncol, int nz, const FallArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_fall_speeds<T, 1>), grid, block, 0, s, c, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_fall_speeds<T, 2>), grid, block, 0, s, c, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_fall_speeds<T, 3>), grid, block, 0, s, c, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_fall_speeds<T, 4>), grid, block, 0, s, c, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_fall_speeds<double>(const Consts *, int64_t, int, const FallArgs<double> &, hipStream_t);
template hipError_t launch_fall_speeds<float>(const Consts *, int64_t, int, const FallArgs<float> &, hipStream_t);

template <class T>
hipError_t launch_size_spectra(const Consts *c, int64_t ncol, int nz, const SpectraArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    const int64_t nblk = (ncol + REFL_WAVES - 1) / REFL_WAVES;
    // few columns and many bins: a column's bins go to several blocks, up to SPECTRA_MAX_SHARES, until the grid holds
    // SPECTRA_MIN_BLOCKS workgroups (four to a compute unit)
    int maxnb = 1;
    for (int x = 0; x < SPECTRA_NSPEC; ++x)
        if (a.spec[x] && a.nb[x] > maxnb) maxnb = a.nb[x];
    int64_t shares = (SPECTRA_MIN_BLOCKS + nblk - 1) / nblk;
    shares = shares > SPECTRA_MAX_SHARES ? SPECTRA_MAX_SHARES : shares;
    shares = shares > maxnb ? maxnb : shares;
    const dim3 grid((unsigned)nblk, (unsigned)shares), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_size_spectra<T, 1>), grid, block, 0, s, c, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_size_spectra<T, 2>), grid, block, 0, s, c, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_size_spectra<T, 3>), grid, block, 0, s, c, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_size_spectra<T, 4>), grid, block, 0, s, c, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_size_spectra<double>(const Consts *, int64_t, int, const SpectraArgs<double> &, hipStream_t);
template hipError_t launch_size_spectra<float>(const Consts *, int64_t, int, const SpectraArgs<float> &, hipStream_t);

bool spectra_consts_supported(const Consts &hc)
{
    // beyond fall_consts_supported: mu_r = mu_g = mu_i = 0 (no D**mu factor; cre(2) = cge(2) = cie(1) = 1), and the
    // cloud-water exponents cce(1,n) = n + 1, cce(2,n) = bm_r + n + 1 taken as integers
    bool ok = fall_consts_supported(hc) && mu_r == 0.0 && mu_g == 0.0 && mu_i == 0.0 && hc.cre[1] == 1. && hc.cge[1] == 1. && hc.cie[0] == 1.;
    for (int n = 1; n <= 15; ++n) ok = ok && hc.cce[0][n - 1] == n + 1. && hc.cce[1][n - 1] == bm_r + n + 1.;
    return ok;
}

template <class T>
hipError_t launch_lidar_profiles(const Consts *c, int64_t ncol, int nz, const LidarArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_lidar_profiles<T, 1>), grid, block, 0, s, c, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_lidar_profiles<T, 2>), grid, block, 0, s, c, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_lidar_profiles<T, 3>), grid, block, 0, s, c, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_lidar_profiles<T, 4>), grid, block, 0, s, c, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_lidar_profiles<double>(const Consts *, int64_t, int, const LidarArgs<double> &, hipStream_t);
template hipError_t launch_lidar_profiles<float>(const Consts *, int64_t, int, const LidarArgs<float> &, hipStream_t);

bool lidar_consts_supported(const Consts &hc)
{
    // beyond spectra_consts_supported: ext_s = (pi/2) smob needs bm_s = 2, and pi N0/lam**3 needs mu = 0 with Gamma(3) = 2
    return spectra_consts_supported(hc) && bm_s == 2.0 && mu_r == 0.0 && mu_g == 0.0 && mu_i == 0.0;
}

template <class T>
hipError_t launch_doppler_moments(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const DopplerArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_doppler_moments<T, 1>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_doppler_moments<T, 2>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_doppler_moments<T, 3>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_doppler_moments<T, 4>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_doppler_moments<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const DopplerArgs<double> &, hipStream_t);
template hipError_t launch_doppler_moments<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const DopplerArgs<float> &, hipStream_t);

template <class T>
hipError_t launch_doppler_spectrum(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const DSpectrumArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    if (a.nv < 1 || a.nv > DSPECTRUM_MAX_NV) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_doppler_spectrum<T, 1>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_doppler_spectrum<T, 2>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_doppler_spectrum<T, 3>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_doppler_spectrum<T, 4>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_doppler_spectrum<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const DSpectrumArgs<double> &, hipStream_t);
template hipError_t launch_doppler_spectrum<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const DSpectrumArgs<float> &, hipStream_t);

template <class T>
hipError_t launch_bright_band(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const BrightBandArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > BRIGHTBAND_MAX_BINS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_bright_band<T, 1>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_bright_band<T, 2>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_bright_band<T, 3>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_bright_band<T, 4>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_bright_band<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const BrightBandArgs<double> &, hipStream_t);
template hipError_t launch_bright_band<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const BrightBandArgs<float> &, hipStream_t);

template <class T>
hipError_t launch_mie_radar(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const MieArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_mie_radar<T, 1>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_mie_radar<T, 2>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_mie_radar<T, 3>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_mie_radar<T, 4>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_mie_radar<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const MieArgs<double> &, hipStream_t);
template hipError_t launch_mie_radar<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const MieArgs<float> &, hipStream_t);

template <class T>
hipError_t launch_radiometer(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const RadiometerArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_radiometer<T, 1>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_radiometer<T, 2>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_radiometer<T, 3>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_radiometer<T, 4>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_radiometer<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const RadiometerArgs<double> &, hipStream_t);
template hipError_t launch_radiometer<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const RadiometerArgs<float> &, hipStream_t);

// The channels one pass carries, by the number of level groups.  Every channel place of a tile costs about half a
// single-channel launch whether a channel fills it or not, and registers beyond 256 cost the second wave per SIMD, so the
// tile is not the widest that fits: at two level groups 4 (radiometer) and 3 (radar) were the fastest of the candidates
// measured, the other counts follow the compiler's report.  No instantiation has scratch; the
// radar's NJ = 3 takes 2 because 3 needs 64 AGPRs, NJ = 4 takes 3 because 2 is the one candidate the compiler spilled.
constexpr int rad_tile(int) { return 4; }
constexpr int mie_tile(int nj) { return nj == 3 ? 2 : 3; }
int multichannel_tile(int which, int nz)
{
    const int nj = (nz + 63) / 64;
    if (nj < 1 || nj > 4 || (which != 0 && which != 1)) return 0;
    return which == 0 ? rad_tile(nj) : mie_tile(nj);
}

template <class T>
hipError_t launch_radiometer_multi(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const RadiometerMultiArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    if (a.nch < 1 || a.nch > MC_MAX_CHANNELS) return hipErrorInvalidValue;
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_radiometer_multi<T, 1, rad_tile(1)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_radiometer_multi<T, 2, rad_tile(2)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_radiometer_multi<T, 3, rad_tile(3)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_radiometer_multi<T, 4, rad_tile(4)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_radiometer_multi<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const RadiometerMultiArgs<double> &, hipStream_t);
template hipError_t launch_radiometer_multi<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const RadiometerMultiArgs<float> &, hipStream_t);

template <class T>
hipError_t launch_mie_radar_multi(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const MieMultiArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    if (a.nch < 1 || a.nch > MC_MAX_CHANNELS) return hipErrorInvalidValue;
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_mie_radar_multi<T, 1, mie_tile(1)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_mie_radar_multi<T, 2, mie_tile(2)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_mie_radar_multi<T, 3, mie_tile(3)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_mie_radar_multi<T, 4, mie_tile(4)>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_mie_radar_multi<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const MieMultiArgs<double> &, hipStream_t);
template hipError_t launch_mie_radar_multi<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const MieMultiArgs<float> &, hipStream_t);

template <class T>
hipError_t launch_polarimetric(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const PolArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (!a.uniform[x] && (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES)), block(REFL_THREADS);
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_polarimetric<T, 1>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_polarimetric<T, 2>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_polarimetric<T, 3>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    case 4: hipLaunchKernelGGL((k_polarimetric<T, 4>), grid, block, 0, s, c, dc, a, ncol, nz); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_polarimetric<double>(const ReflConsts &, const DopplerConsts &, int64_t, int, const PolArgs<double> &, hipStream_t);
template hipError_t launch_polarimetric<float>(const ReflConsts &, const DopplerConsts &, int64_t, int, const PolArgs<float> &, hipStream_t);

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

bool fall_consts_supported(const Consts &hc)
{
    // the exponents lvl:: takes as roots and integer powers (thompson_init, M:452-553, from bm_*, bv_*, mu_*)
    return hc.obmr == 1. / 3. && hc.obmi == 1. / 3. && hc.oge1 == 0.25 && hc.cre[2] == 4. && hc.cre[5] == 5.
           && hc.cre[11] == 2.5 && hc.cre[6] == 3.5 && hc.cse[0] == 3. && bm_s == 2.0 && bm_i == 3.0 && bm_r == 3.0 && bv_i == 1.0;
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
