// kidmp_radiometer_channel.h -- internal to kidmp_radiometer.hip and kidmp_multichannel.hip: what k_radiometer and
// k_radiometer_multi share, so that slab c of the multi-channel kernel holds the single-channel kernel's bits by construction.
#pragma once
#include "kidmp_channel_call.h"
#include "kidmp_column.h"
#include "kidmp_radiometer_layer.h"

namespace kidmp {

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

}  // namespace kidmp
