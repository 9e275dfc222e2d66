// kidmp_mie_channel.h -- internal to kidmp_mie.hip and kidmp_multichannel.hip: what k_mie_radar and k_mie_radar_multi share,
// so that slab c of the multi-channel kernel holds the single-channel kernel's bits by construction.
#pragma once
#include "kidmp_channel_call.h"
#include "kidmp_column.h"

namespace kidmp {

// ---- the cloud radar (include/kidmp_mie.h) ----
constexpr double MIE_PIA = 20. / 2.302585092994045684;              // two-way dB per unit of one-way optical depth: 2*(10/ln 10)

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

}  // namespace kidmp
