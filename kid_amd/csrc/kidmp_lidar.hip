// kidmp_lidar.hip -- the entries of include/kidmp_lidar.h: extinction, backscatter, optical depth and attenuated
// backscatter of device arrays in one launch of k_lidar_profiles (below), and of host arrays in chunks
// through the context's staging memory.
#include "kidmp_ctx.h"
#include "../../include/kidmp_lidar.h"

#include <cmath>

#include "kidmp_column.h"

namespace kidmp {

// The lidar operator (include/kidmp_lidar.h): extinction, backscatter, optical depth and attenuated backscatter of every
// level, and eight numbers per column, from the size spectra's load.  Null means: nc -- Nt_c (the context is not
// aerosol-aware); qi and ni, qs, qg -- the species is absent everywhere (iiwarm); an output or the summary -- not wanted;
// dz -- not read when nothing past out[LIDAR_NLOCAL - 1] and no summary is wanted.  out in the order of kidmp_lidar_out.
constexpr int LIDAR_NOUT = 14, LIDAR_NLOCAL = 8, LIDAR_SUMMARY_N = 8;      // out[0..7] need no neighbour: no scan
constexpr int LIDAR_TAU_UP = 8, LIDAR_TAU_DN = 9, LIDAR_ATT_UP = 10, LIDAR_ATT_DN = 11, LIDAR_SR_UP = 12, LIDAR_SR_DN = 13;
template <class T> struct LidarArgs {
    const T *t, *p, *qv, *qc, *nc, *qi, *ni, *qr, *nr, *qs, *qg, *dz;
    int64_t dz_col_stride;
    T *out[LIDAR_NOUT];
    double *summary;                                 // [ncol][LIDAR_SUMMARY_N]
    double s_ratio[SPECTRA_NSPEC], eta, c_mol, beta_detect, trans_lost;
    const double *set_nc_col;
    int aero;
};

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
    int lane;
    const int64_t col = enter_column(lane);
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

namespace {
template <class T>
hipError_t launch_lidar_profiles(const Consts *c, int64_t ncol, int nz, const LidarArgs<T> &a, hipStream_t s)
{
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_lidar_profiles<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, a, ncol, nz);
    });
}

bool lidar_consts_supported(const Consts &hc)
{
    // beyond spectra_consts_supported: ext_s = (pi/2) smob needs bm_s = 2, and pi N0/lam**3 needs mu = 0 with Gamma(3) = 2
    return spectra_consts_supported(hc) && bm_s == 2.0 && mu_r == 0.0 && mu_g == 0.0 && mu_i == 0.0;
}
}  // namespace

}  // namespace kidmp

using namespace kidmp;

static_assert(sizeof(kidmp_lidar_out) == LIDAR_NOUT * sizeof(double *) && sizeof(kidmp32_lidar_out) == LIDAR_NOUT * sizeof(float *)
                  && LIDAR_SUMMARY_N == KIDMP_LIDAR_SUMMARY_N && sizeof(kidmp_lidar_cfg) == (SPECTRA_NSPEC + 4) * sizeof(double),
              "include/kidmp_lidar.h");

namespace {
constexpr int NIN = 11;                                   // t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg"};
const char *const OUT_NAMES[LIDAR_NOUT] = {"ext_c", "ext_i", "ext_r", "ext_s", "ext_g", "ext", "bsc", "bsc_mol", "tau_up", "tau_dn",
                                           "att_up", "att_dn", "sr_up", "sr_dn"};
constexpr bool REQUIRED[NIN] = {true, true, true, true, false, false, false, true, true, false, false};
constexpr bool FROZEN_IN[NIN] = {false, false, false, false, false, true, true, false, false, true, true};
const kidmp_lidar_cfg DEFAULT_CFG = {{18.8, 25., 18.8, 25., 25.}, 0.7, 6.2446e-32, 2.e-5, 2.5e-3};

template <class T> struct LidarCall {
    const T *in[NIN];
    const T *dz;
    int64_t dz_col_stride;
    T *out[LIDAR_NOUT];
    double *summary;
};
template <class T, class O>
LidarCall<T> lidar_call(const T *t, const T *p, const T *qv, const T *qc, const T *nc, const T *qi, const T *ni, const T *qr, const T *nr,
                        const T *qs, const T *qg, const T *dz, int64_t dz_col_stride, const O *out, double *summary)
{
    LidarCall<T> c{{t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg}, dz, dz_col_stride, {}, summary};
    if (out) {
        T *const o[LIDAR_NOUT] = {out->ext_c, out->ext_i, out->ext_r, out->ext_s, out->ext_g, out->ext, out->bsc, out->bsc_mol,
                                  out->tau_up, out->tau_dn, out->att_up, out->att_dn, out->sr_up, out->sr_dn};
        for (int v = 0; v < LIDAR_NOUT; ++v) c.out[v] = o[v];
    }
    return c;
}
// whether the call goes beyond the profiles that need no neighbour: then the kernel scans and reads dz
template <class T> bool needs_depth(const LidarCall<T> &a)
{
    bool any = a.summary != nullptr;
    for (int v = LIDAR_NLOCAL; v < LIDAR_NOUT; ++v) any = any || a.out[v];
    return any;
}

// what the device and the host entries check alike, before anything is touched; use receives the configuration
template <class T>
int check_lidar(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const LidarCall<T> &a, const kidmp_lidar_cfg *cfg, kidmp_lidar_cfg &use)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (int rc = check_nc_count(ctx, who, ncol)) return rc;
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (a.dz_col_stride != 0 && a.dz_col_stride < nz) return fail(ctx, KIDMP_EINVAL, w + ": dz_col_stride must be 0 or >= nz");
    use = cfg ? *cfg : DEFAULT_CFG;
    bool finite = std::isfinite(use.eta) && std::isfinite(use.c_mol) && std::isfinite(use.beta_detect) && std::isfinite(use.trans_lost);
    for (int x = 0; x < SPECTRA_NSPEC; ++x) finite = finite && std::isfinite(use.s_ratio[x]);
    if (!finite) return fail(ctx, KIDMP_EINVAL, w + ": a member of cfg is not finite");
    for (int x = 0; x < SPECTRA_NSPEC; ++x)
        if (!(use.s_ratio[x] > 0.)) return fail(ctx, KIDMP_EINVAL, w + ": a lidar ratio must be positive");
    if (!(use.eta > 0. && use.eta <= 1.)) return fail(ctx, KIDMP_EINVAL, w + ": eta outside (0, 1]");
    if (use.c_mol < 0.) return fail(ctx, KIDMP_EINVAL, w + ": c_mol < 0");
    if (use.c_mol == 0. && (a.out[LIDAR_SR_UP] || a.out[LIDAR_SR_DN]))
        return fail(ctx, KIDMP_EINVAL, w + ": a scattering ratio needs c_mol > 0");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = a.summary != nullptr;
    for (int v = 0; v < LIDAR_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: every profile and the summary are NULL");
    for (int v = 0; v < NIN; ++v)
        if (REQUIRED[v] && !a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (needs_depth(a) && !a.dz) return fail(ctx, KIDMP_EINVAL, w + ": optical depths need dz");
    if (!ctx->cfg.iiwarm)
        for (int v = 0; v < NIN; ++v)
            if (FROZEN_IN[v] && !a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": a mixed-phase context needs qi, ni, qs and qg");
    if (ctx->cfg.is_aerosol_aware && !a.in[4]) return fail(ctx, KIDMP_EINVAL, w + ": an aerosol-aware context needs nc");
    if (!lidar_consts_supported(ctx->hc)) return fail(ctx, KIDMP_ESTATE, w + ": size-distribution exponents differ from the closed forms'");
    return KIDMP_OK;
}

// one launch over device pointers; nc_first: the batch's first column within a bound per-column droplet number.  An
// iiwarm context reads no frozen input; a context that is not aerosol-aware does not read nc.
template <class T>
hipError_t enqueue_lidar(kidmp_ctx *ctx, int64_t ncol, int nz, const LidarCall<T> &a, const kidmp_lidar_cfg &g, int64_t nc_first, hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0, aero = ctx->cfg.is_aerosol_aware != 0;
    const T *const *q = a.in;
    LidarArgs<T> args{q[0], q[1], q[2], q[3], aero ? q[4] : nullptr, warm ? nullptr : q[5], warm ? nullptr : q[6], q[7], q[8],
                      warm ? nullptr : q[9], warm ? nullptr : q[10], a.dz, a.dz_col_stride, {}, a.summary,
                      {g.s_ratio[0], g.s_ratio[1], g.s_ratio[2], g.s_ratio[3], g.s_ratio[4]}, g.eta, g.c_mol, g.beta_detect, g.trans_lost,
                      ctx->d_nc_col ? ctx->d_nc_col + nc_first : nullptr, aero ? 1 : 0};
    for (int v = 0; v < LIDAR_NOUT; ++v) args.out[v] = a.out[v];
    return launch_lidar_profiles<T>(ctx->d_consts, ncol, nz, args, s);
}

template <class T>
int lidar_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const LidarCall<T> &a, const kidmp_lidar_cfg *cfg, void *stream)
{
    kidmp_lidar_cfg g;
    if (int rc = check_lidar<T>(ctx, who, ncol, nz, a, cfg, g)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0;
    for (int v = 0; v < NIN; ++v)
        if (!(warm && FROZEN_IN[v]))
            if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    if (int rc = check_device_array(ctx, who, a.dz, "dz")) return rc;
    for (int v = 0; v < LIDAR_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], OUT_NAMES[v])) return rc;
    if (int rc = check_device_array(ctx, who, a.summary, "summary")) return rc;
    HIPTRY(ctx, enqueue_lidar<T>(ctx, ncol, nz, a, g, 0, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip.  Only what the kernel reads goes up and only what was asked for comes down.
template <class T>
int lidar_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const LidarCall<T> &h, const kidmp_lidar_cfg *cfg)
{
    kidmp_lidar_cfg g;
    if (int rc = check_lidar<T>(ctx, who, ncol, nz, h, cfg, g)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0, aero = ctx->cfg.is_aerosol_aware != 0;
    constexpr int A_DZ = NIN, A_OUT = NIN + 1, A_SUM = A_OUT + LIDAR_NOUT;
    StageArray a[A_SUM + 1];
    for (int v = 0; v < NIN; ++v) a[v] = stage_array((warm && FROZEN_IN[v]) || (v == 4 && !aero) ? nullptr : h.in[v], nz, STAGE_UP);
    a[A_DZ] = stage_rows(needs_depth(h) ? h.dz : nullptr, nz, h.dz_col_stride);
    for (int v = 0; v < LIDAR_NOUT; ++v) a[A_OUT + v] = stage_array(h.out[v], nz, STAGE_DOWN);
    a[A_SUM] = stage_array(h.summary, KIDMP_LIDAR_SUMMARY_N, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    LidarCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[v]);
    d.dz = staged<T>(a[A_DZ]);
    d.dz_col_stride = h.dz_col_stride ? nz : 0;           // staged rows are packed
    for (int v = 0; v < LIDAR_NOUT; ++v) d.out[v] = staged<T>(a[A_OUT + v]);
    d.summary = staged<double>(a[A_SUM]);
    return stage_run(ctx, plan, [&](int64_t c0, int64_t n) { return enqueue_lidar<T>(ctx, n, nz, d, g, c0, ctx->stream); });
}
}  // namespace

extern "C" {
int kidmp_lidar_profiles_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                const double *qc, const double *nc, const double *qi, const double *ni, const double *qr, const double *nr,
                                const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
                                const kidmp_lidar_out *out, double *summary, void *stream)
{
    return lidar_device<double>(ctx, "kidmp_lidar_profiles_device", ncol, nz,
                                lidar_call<double>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz, dz_col_stride, out, summary), cfg, stream);
}
int kidmp32_lidar_profiles_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                  const float *qc, const float *nc, const float *qi, const float *ni, const float *qr, const float *nr,
                                  const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
                                  const kidmp32_lidar_out *out, double *summary, void *stream)
{
    return lidar_device<float>(ctx, "kidmp32_lidar_profiles_device", ncol, nz,
                               lidar_call<float>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz, dz_col_stride, out, summary), cfg, stream);
}
int kidmp_lidar_profiles_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                              const double *qc, const double *nc, const double *qi, const double *ni, const double *qr, const double *nr,
                              const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
                              const kidmp_lidar_out *out, double *summary)
{
    return lidar_host<double>(ctx, "kidmp_lidar_profiles_host", ncol, nz,
                              lidar_call<double>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz, dz_col_stride, out, summary), cfg);
}
int kidmp32_lidar_profiles_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                const float *qc, const float *nc, const float *qi, const float *ni, const float *qr, const float *nr,
                                const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
                                const kidmp32_lidar_out *out, double *summary)
{
    return lidar_host<float>(ctx, "kidmp32_lidar_profiles_host", ncol, nz,
                             lidar_call<float>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, dz, dz_col_stride, out, summary), cfg);
}
}  // extern "C"
