// kidmp_brightband.hip -- the entries of include/kidmp_brightband.h: the reflectivity with its melting layer of device
// arrays in one launch of k_bright_band (below), and of host arrays in chunks through the context's
// staging memory.
#include <cmath>
#include <cstddef>

#include "kidmp_ctx.h"
#include "../../include/kidmp_brightband.h"

#include "kidmp_brightband_mix.h"
#include "kidmp_column.h"

namespace kidmp {

// The bright band (include/kidmp_brightband.h): calc_refl10cm with melting snow and graupel below the melting level, from
// k_doppler_moments' load.  Null means: qs, qg -- zero; an output -- not wanted.  out: dbz, dbz_s, dbz_g, enh_s, enh_g,
// fmelt_s, fmelt_g [ncol][nz]; k0 [ncol].  D, dD: device arrays of nb[x] doubles by species snow, graupel.  warm: an iiwarm
// context, no melting level.  One launch; the lanes sweep the diameter bins of each active (level, species) pair.
constexpr int BRIGHTBAND_NOUT = 7, BRIGHTBAND_NSPEC = 2, BRIGHTBAND_MAX_BINS = 256;
template <class T> struct BrightBandArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg;
    T *out[BRIGHTBAND_NOUT];
    int32_t *k0;
    const double *D[BRIGHTBAND_NSPEC], *dD[BRIGHTBAND_NSPEC];
    int32_t nb[BRIGHTBAND_NSPEC];
    BBMix mix;
    int warm;
};

// ---- the bright band (include/kidmp_brightband.h) ----
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
    int lane;
    const int64_t col = enter_column(lane);
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

namespace {
template <class T>
hipError_t launch_bright_band(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const BrightBandArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // an empty batch is not looked at
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > BRIGHTBAND_MAX_BINS) return hipErrorInvalidValue;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_bright_band<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, dc, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

using namespace kidmp;

static_assert(sizeof(kidmp_brightband_out) == BRIGHTBAND_NOUT * sizeof(double *) + sizeof(int32_t *)
                  && sizeof(kidmp32_brightband_out) == BRIGHTBAND_NOUT * sizeof(float *) + sizeof(int32_t *)
                  && BRIGHTBAND_NSPEC == KIDMP_BB_NSPECIES && BRIGHTBAND_MAX_BINS == KIDMP_BB_MAX_BINS && nbins <= KIDMP_BB_MAX_BINS,
              "include/kidmp_brightband.h");

namespace {
constexpr int NIN = 7, NREQ = 5;                          // t, p, qv, qr, nr | qs, qg
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qr", "nr", "qs", "qg"};
const char *const OUT_NAMES[BRIGHTBAND_NOUT] = {"dbz", "dbz_s", "dbz_g", "enh_s", "enh_g", "fmelt_s", "fmelt_g"};

// the scheme's own grid of a species inside a Bins (host or device copy alike): snow, graupel
const double *bins_D(const Bins *b, int x) { return x == 0 ? b->Ds : b->Dg; }
const double *bins_dD(const Bins *b, int x) { return x == 0 ? b->dts : b->dtg; }

template <class T> struct BrightBandCall {
    const T *in[NIN];
    T *out[BRIGHTBAND_NOUT];
    int32_t *k0;
    const double *D[BRIGHTBAND_NSPEC], *dD[BRIGHTBAND_NSPEC];   // the caller's; both null: the scheme's own
    int32_t nb[BRIGHTBAND_NSPEC];
    kidmp_brightband_cfg cfg;
};
template <class T, class O>
BrightBandCall<T> brightband_call(const T *t, const T *p, const T *qv, const T *qr, const T *nr, const T *qs, const T *qg,
                                  const kidmp_brightband_cfg *cfg, const kidmp_brightband_grids *grids, const O *out)
{
    BrightBandCall<T> c{{t, p, qv, qr, nr, qs, qg}, {}, nullptr, {}, {}, {}, {}};
    if (cfg) c.cfg = *cfg;
    else kidmp_brightband_defaults(&c.cfg);
    if (out) {
        T *const o[BRIGHTBAND_NOUT] = {out->dbz, out->dbz_s, out->dbz_g, out->enh_s, out->enh_g, out->fmelt_s, out->fmelt_g};
        for (int v = 0; v < BRIGHTBAND_NOUT; ++v) c.out[v] = o[v];
        c.k0 = out->k0;
    }
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x) {
        c.nb[x] = nbins;
        if (grids && (grids->D[x] || grids->dD[x])) { c.D[x] = grids->D[x]; c.dD[x] = grids->dD[x]; c.nb[x] = grids->nb[x]; }
    }
    return c;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_brightband(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const BrightBandCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    const kidmp_brightband_cfg &g = a.cfg;
    const double members[] = {g.eps_w_re, g.eps_w_im, g.eps_i, g.rho_w, g.rho_i, g.kw2};
    for (double m : members)
        if (!std::isfinite(m)) return fail(ctx, KIDMP_EINVAL, w + ": a member of the configuration is not finite");
    if (!(g.rho_w > 0.) || !(g.rho_i > 0.) || !(g.kw2 > 0.)) return fail(ctx, KIDMP_EINVAL, w + ": rho_w, rho_i and kw2 must be above 0");
    if (g.topology != KIDMP_BB_WATER_MATRIX && g.topology != KIDMP_BB_ICE_MATRIX) return fail(ctx, KIDMP_EINVAL, w + ": unknown topology");
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x) {
        if ((a.D[x] == nullptr) != (a.dD[x] == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": a grid needs both D and dD");
        if (a.nb[x] < 1 || a.nb[x] > KIDMP_BB_MAX_BINS) return fail(ctx, KIDMP_EINVAL, w + ": nb outside [1, KIDMP_BB_MAX_BINS]");
    }
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = a.k0 != nullptr;
    for (int v = 0; v < BRIGHTBAND_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: out is NULL or every member is");
    for (int v = 0; v < NREQ; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (!doppler_consts_supported(ctx->hc) || !spectra_consts_supported(ctx->hc))
        return fail(ctx, KIDMP_ESTATE, w + ": exponents differ from the kernel's");
    return KIDMP_OK;
}

// one launch over device pointers
template <class T>
hipError_t enqueue_brightband(kidmp_ctx *ctx, int64_t ncol, int nz, const BrightBandCall<T> &a, hipStream_t s)
{
    const T *const *q = a.in;
    BrightBandArgs<T> args{q[0], q[1], q[2], q[3], q[4], q[5], q[6], {}, a.k0, {}, {}, {}, {}, ctx->cfg.iiwarm != 0};
    for (int v = 0; v < BRIGHTBAND_NOUT; ++v) args.out[v] = a.out[v];
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x) {
        args.D[x] = a.D[x] ? a.D[x] : bins_D(ctx->d_bins, x);
        args.dD[x] = a.dD[x] ? a.dD[x] : bins_dD(ctx->d_bins, x);
        args.nb[x] = a.D[x] ? a.nb[x] : nbins;
    }
    const kidmp_brightband_cfg &g = a.cfg;
    args.mix = BBMix{g.eps_w_re, g.eps_w_im, g.eps_i, bb_K_real(g.eps_i), g.rho_w, g.rho_i, g.topology == KIDMP_BB_ICE_MATRIX};
    return launch_bright_band<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int brightband_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const BrightBandCall<T> &a, void *stream)
{
    if (int rc = check_brightband<T>(ctx, who, ncol, nz, a)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NIN; ++v)
        if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    for (int v = 0; v < BRIGHTBAND_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], OUT_NAMES[v])) return rc;
    if (int rc = check_device_array(ctx, who, a.k0, "k0")) return rc;
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x) {
        if (int rc = check_device_array(ctx, who, a.D[x], "D")) return rc;
        if (int rc = check_device_array(ctx, who, a.dD[x], "dD")) return rc;
    }
    HIPTRY(ctx, enqueue_brightband<T>(ctx, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip.  The caller's grids go up once, only the inputs given go up per chunk and only
// what was asked for comes down.
template <class T>
int brightband_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const BrightBandCall<T> &h)
{
    if (int rc = check_brightband<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    constexpr int A_D = 0, A_DD = BRIGHTBAND_NSPEC, A_IN = 2 * BRIGHTBAND_NSPEC, A_OUT = A_IN + NIN, A_K0 = A_OUT + BRIGHTBAND_NOUT;
    StageArray a[A_K0 + 1];
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x) {
        a[A_D + x] = stage_once(h.D[x], h.nb[x]);
        a[A_DD + x] = stage_once(h.dD[x], h.nb[x]);
    }
    for (int v = 0; v < NIN; ++v) a[A_IN + v] = stage_array(h.in[v], nz, STAGE_UP);
    for (int v = 0; v < BRIGHTBAND_NOUT; ++v) a[A_OUT + v] = stage_array(h.out[v], nz, STAGE_DOWN);
    a[A_K0] = stage_array(h.k0, 1, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    BrightBandCall<T> d{};
    d.cfg = h.cfg;
    for (int x = 0; x < BRIGHTBAND_NSPEC; ++x) {
        d.nb[x] = h.nb[x];
        d.D[x] = staged<double>(a[A_D + x]);
        d.dD[x] = staged<double>(a[A_DD + x]);
    }
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[A_IN + v]);
    for (int v = 0; v < BRIGHTBAND_NOUT; ++v) d.out[v] = staged<T>(a[A_OUT + v]);
    d.k0 = staged<int32_t>(a[A_K0]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_brightband<T>(ctx, n, nz, d, ctx->stream); });
}
}  // namespace

extern "C" {
void kidmp_brightband_defaults(kidmp_brightband_cfg *cfg)
{
    if (!cfg) return;
    const double k = std::sqrt(0.176);
    *cfg = kidmp_brightband_cfg{79.5, 24.9, (1. + 2. * k) / (1. - k), 1000., 900., 0.93, KIDMP_BB_WATER_MATRIX};
}
int kidmp_bright_band_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                             const double *qr, const double *nr, const double *qs, const double *qg, const kidmp_brightband_cfg *cfg,
                             const kidmp_brightband_grids *grids, const kidmp_brightband_out *out, void *stream)
{
    return brightband_device<double>(ctx, "kidmp_bright_band_device", ncol, nz,
                                     brightband_call<double>(t, p, qv, qr, nr, qs, qg, cfg, grids, out), stream);
}
int kidmp32_bright_band_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                               const float *qr, const float *nr, const float *qs, const float *qg, const kidmp_brightband_cfg *cfg,
                               const kidmp_brightband_grids *grids, const kidmp32_brightband_out *out, void *stream)
{
    return brightband_device<float>(ctx, "kidmp32_bright_band_device", ncol, nz,
                                    brightband_call<float>(t, p, qv, qr, nr, qs, qg, cfg, grids, out), stream);
}
int kidmp_bright_band_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                           const double *qr, const double *nr, const double *qs, const double *qg, const kidmp_brightband_cfg *cfg,
                           const kidmp_brightband_grids *grids, const kidmp_brightband_out *out)
{
    return brightband_host<double>(ctx, "kidmp_bright_band_host", ncol, nz,
                                   brightband_call<double>(t, p, qv, qr, nr, qs, qg, cfg, grids, out));
}
int kidmp32_bright_band_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                             const float *qr, const float *nr, const float *qs, const float *qg, const kidmp_brightband_cfg *cfg,
                             const kidmp_brightband_grids *grids, const kidmp32_brightband_out *out)
{
    return brightband_host<float>(ctx, "kidmp32_bright_band_host", ncol, nz,
                                  brightband_call<float>(t, p, qv, qr, nr, qs, qg, cfg, grids, out));
}
}  // extern "C"
