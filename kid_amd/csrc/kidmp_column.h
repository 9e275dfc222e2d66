// kidmp_column.h -- internal to the wave-per-column diagnostics (not installed): included by thompson_reflectivity.hip and by
// every unit that holds a kernel of this layout -- kidmp_summary, kidmp_fall, kidmp_spectra, kidmp_lidar, kidmp_doppler,
// kidmp_dspectrum, kidmp_brightband, kidmp_polarimetric .hip directly, kidmp_mie, kidmp_radiometer and kidmp_multichannel
// .hip through kidmp_channel_call.h.  One wavefront per column (four per workgroup), lanes over levels: level k = 64 j + lane
// in level group j, NJ = ceil(nz/64) groups per lane, the kernel templated on NJ.  Here: the workgroup shape and the kernels'
// common entry, the wave and column primitives, the state as mp_thompson and as calc_refl10cm load it, the loops over a
// table's diameter bins, and the host's launch of "the instantiation for nz levels".  The per-level arithmetic is
// thompson_levels.h.  Division is IEEE: none of these units takes the column kernel's flags.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "thompson_params.h"
#include "thompson_levels.h"
#include "kidmp_wave.h"

namespace kidmp {

// ---- the exponents the loads below take as roots and integer powers ----
inline bool fall_consts_supported(const Consts &hc)
{
    // the exponents lvl:: takes as roots and integer powers (thompson_init, M:452-553, from bm_*, bv_*, mu_*)
    return hc.obmr == 1. / 3. && hc.obmi == 1. / 3. && hc.oge1 == 0.25 && hc.cre[2] == 4. && hc.cre[5] == 5.
           && hc.cre[11] == 2.5 && hc.cre[6] == 3.5 && hc.cse[0] == 3. && bm_s == 2.0 && bm_i == 3.0 && bm_r == 3.0 && bv_i == 1.0;
}

inline bool spectra_consts_supported(const Consts &hc)
{
    // beyond fall_consts_supported: mu_r = mu_g = mu_i = 0 (no D**mu factor; cre(2) = cge(2) = cie(1) = 1), and the
    // cloud-water exponents cce(1,n) = n + 1, cce(2,n) = bm_r + n + 1 taken as integers
    bool ok = fall_consts_supported(hc) && mu_r == 0.0 && mu_g == 0.0 && mu_i == 0.0 && hc.cre[1] == 1. && hc.cge[1] == 1. && hc.cie[0] == 1.;
    for (int n = 1; n <= 15; ++n) ok = ok && hc.cce[0][n - 1] == n + 1. && hc.cce[1][n - 1] == bm_r + n + 1.;
    return ok;
}

// what block O reads, picked from the context's Consts: on the device from its copy in HBM (scalar loads on demand: as
// kernel arguments the 50 values pressed on the SGPRs), on the host for whoever wants to look
__host__ __device__ inline FallConsts fall_consts(const Consts &hc)
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

constexpr int SPECTRA_NSPEC = 5;                     // the species of mp_thompson's load, in the order c, i, r, s, g

// Linkage is what it was when all of this stood in one file: the first group internal (anonymous namespace), the second plain
// inline functions of kidmp::.  The inliner treats the two differently, and the kernels' code is held to the instruction.
namespace {

constexpr int REFL_WAVES = 4;                        // columns (wavefronts) per workgroup
constexpr int REFL_THREADS = 64 * REFL_WAVES;
using wave::readlane;                                // kidmp_wave.h
using wave::wave_prefix_sum;
using wave::wave_max;

// What every kernel of this layout opens with: the fastmath tables into LDS (log10 / 10**x / x**y read them from there), then
// the wave's lane and, returned, its column.  A wave whose column is not below ncol returns at once, after the barrier:
// whole wavefronts only, the scans need every lane.  That test and base = col*nz stay in the kernel: every form of this
// helper that made them its own changed the register allocation or the schedule of some instantiation.
__device__ __forceinline__ int64_t enter_column(int &lane)
{
#if KFM_TABLES
    fm::tab::load_tables(int(threadIdx.x), REFL_THREADS);
    __syncthreads();
#endif
    lane = int(threadIdx.x) & 63;
    return int64_t(blockIdx.x) * REFL_WAVES + (int(threadIdx.x) >> 6);
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

// butterfly over the wave: every lane ends with the same bits (a + b == b + a), in an order that depends on nothing
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
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

__device__ inline double wave_min(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}

// sum over the wave in the order the header fixes: a butterfly over xor 32, 16, ..., 1; every lane ends with the same bits
__device__ inline double wave_sum_down(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

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

// ---- the host's side ----
// the grid: REFL_WAVES columns per workgroup; shares: the workgroups that divide a column group's work (the size spectra)
inline dim3 column_grid(int64_t ncol, unsigned shares = 1) { return dim3((unsigned)((ncol + REFL_WAVES - 1) / REFL_WAVES), shares); }

// A kernel templated on the level-group count: launch(std::integral_constant<int, NJ>) enqueues the instantiation for nz
// levels.  An empty batch launches nothing; more than four level groups (nz > KIDMP_MAX_NZ), or none, are refused.
template <class F>
hipError_t launch_level_groups(int64_t ncol, int nz, F &&launch)
{
    if (ncol <= 0) return hipSuccess;
    switch ((nz + 63) / 64) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace kidmp
