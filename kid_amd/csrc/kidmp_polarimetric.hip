// kidmp_polarimetric.hip -- the entries of include/kidmp_polarimetric.h: the spheroid and the per-bin rows on the host
// (kidmp_spheroid.h), the table object that carries them and the uniform species' scalars to the device, and the
// polarimetric radar of device arrays in one launch of k_polarimetric (below) or of host arrays in
// chunks through the context's staging memory.
#include <cmath>
#include <cstddef>

#include "kidmp_mie_table.h"
#include "kidmp_spheroid.h"
#include "../../include/kidmp_polarimetric.h"

#include "kidmp_column.h"

namespace kidmp {

// The polarimetric radar (include/kidmp_polarimetric.h): Z_DR, K_DP and rho_hv of oblate spheroids from k_mie_radar's load
// and a table of seven rows per diameter bin (s_h, s_v, c_re, c_im, s_0, k, mass).  Null means: qs, qg -- zero; an output
// -- not wanted.  out in the order of kidmp_pol_out.  uniform[x] != 0: the species walks no bins and takes scal[x] (s_h/s_0,
// s_v/s_0, c_re/s_0, c_im/s_0, k/mass) in place of the ratios of its sums; its D, dD, rows and nb are not read.
// kfac: 90e3 pi/lambda.  One launch; lanes over levels, a loop over the bins.
constexpr int POL_NOUT = 13, POL_NROWS = 7, POL_NSCAL = 5;
constexpr int POL_DBZ_H = 0, POL_ZDR = 1, POL_KDP = 2, POL_RHOHV = 3, POL_DBZ_H_X = 4, POL_ZDR_X = 7, POL_KDP_X = 10;
template <class T> struct PolArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg;
    T *out[POL_NOUT];
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC], *rows[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    int32_t uniform[MIE_NSPEC];
    double scal[MIE_NSPEC][POL_NSCAL];
    double kfac;
};

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
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
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

namespace {
template <class T>
hipError_t launch_polarimetric(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const PolArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // an empty batch is not looked at
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (!a.uniform[x] && (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS)) return hipErrorInvalidValue;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_polarimetric<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, dc, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

using namespace kidmp;

static_assert(sizeof(kidmp_pol_out) == POL_NOUT * sizeof(double *) && sizeof(kidmp32_pol_out) == POL_NOUT * sizeof(float *)
                  && POL_NROWS == KIDMP_POL_NROWS && POL_ROWS == KIDMP_POL_NROWS && POL_NSCAL == KIDMP_POL_NSCALARS
                  && sizeof(kidmp_pol_cfg) == 12 * sizeof(double) && offsetof(kidmp_pol_cfg, force_quadrature) == 11 * sizeof(double),
              "include/kidmp_polarimetric.h");

// the Mie table's buffer with seven rows per bin, and per species the flag and the scalars of a uniform one
struct kidmp_pol_table : kidmp::MieTableData {
    kidmp_pol_cfg pol;
    int32_t uniform[MIE_NSPEC];
    double scal[MIE_NSPEC][POL_NSCAL];
    double kfac;                                              // 90e3 pi/lambda: degrees per km
};

namespace {
constexpr int NIN = 7, NREQ = 5;                              // t, p, qv, qr, nr | qs, qg
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qr", "nr", "qs", "qg"};
const char *const OUT_NAMES[POL_NOUT] = {"dbz_h", "zdr", "kdp", "rhohv", "dbz_h_r", "dbz_h_s", "dbz_h_g", "zdr_r", "zdr_s", "zdr_g",
                                         "kdp_r", "kdp_s", "kdp_g"};

PolCfg pol_model_cfg(const kidmp_pol_cfg &g)
{
    return PolCfg{{g.axis_r[0], g.axis_r[1], g.axis_r[2], g.axis_r[3], g.axis_r[4]}, g.axis_r_min, g.axis_s, g.axis_g,
                  {g.sigma[0], g.sigma[1], g.sigma[2]}, g.force_quadrature};
}

template <class T> struct PolCall {
    const T *in[NIN];
    T *out[POL_NOUT];
};
template <class T, class O>
PolCall<T> pol_call(const T *t, const T *p, const T *qv, const T *qr, const T *nr, const T *qs, const T *qg, const O *out)
{
    PolCall<T> c{{t, p, qv, qr, nr, qs, qg}, {}};
    if (out) {
        T *const o[POL_NOUT] = {out->dbz_h, out->zdr, out->kdp, out->rhohv, out->dbz_h_r, out->dbz_h_s, out->dbz_h_g, out->zdr_r, out->zdr_s,
                                out->zdr_g, out->kdp_r, out->kdp_s, out->kdp_g};
        for (int v = 0; v < POL_NOUT; ++v) c.out[v] = o[v];
    }
    return c;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_pol(kidmp_ctx *ctx, const char *who, const kidmp_pol_table *tab, int64_t ncol, int32_t nz, const PolCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (!tab || tab->ctx != ctx) return fail(ctx, KIDMP_EINVAL, w + ": the table is NULL or belongs to another context");
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = false;
    for (int v = 0; v < POL_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: out is NULL or every member is");
    for (int v = 0; v < NREQ; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (!doppler_consts_supported(ctx->hc) || !spectra_consts_supported(ctx->hc))
        return fail(ctx, KIDMP_ESTATE, w + ": exponents differ from the kernel's");
    return KIDMP_OK;
}

// one launch over device pointers; an iiwarm context reads no snow and no graupel
template <class T>
hipError_t enqueue_pol(kidmp_ctx *ctx, const kidmp_pol_table *tab, int64_t ncol, int nz, const PolCall<T> &a, hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    const T *const *q = a.in;
    PolArgs<T> args{};
    args.t = q[0]; args.p = q[1]; args.qv = q[2]; args.qr = q[3]; args.nr = q[4];
    args.qs = warm ? nullptr : q[5];
    args.qg = warm ? nullptr : q[6];
    for (int v = 0; v < POL_NOUT; ++v) args.out[v] = a.out[v];
    for (int x = 0; x < MIE_NSPEC; ++x) {
        const double *b = tab->d_buf + tab->off[x];
        args.nb[x] = tab->nb[x];
        args.D[x] = b;
        args.dD[x] = b + tab->nb[x];
        args.rows[x] = b + 2 * size_t(tab->nb[x]);
        args.uniform[x] = tab->uniform[x];
        for (int i = 0; i < POL_NSCAL; ++i) args.scal[x][i] = tab->scal[x][i];
    }
    args.kfac = tab->kfac;
    return launch_polarimetric<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int pol_device(kidmp_ctx *ctx, const char *who, const kidmp_pol_table *tab, int64_t ncol, int32_t nz, const PolCall<T> &a, void *stream)
{
    if (int rc = check_pol<T>(ctx, who, tab, ncol, nz, a)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NIN; ++v)
        if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    for (int v = 0; v < POL_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], OUT_NAMES[v])) return rc;
    HIPTRY(ctx, enqueue_pol<T>(ctx, tab, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip.  Only the inputs the kernel reads go up and only what was asked for comes down.
template <class T>
int pol_host(kidmp_ctx *ctx, const char *who, const kidmp_pol_table *tab, int64_t ncol, int32_t nz, const PolCall<T> &h)
{
    if (int rc = check_pol<T>(ctx, who, tab, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0;
    StageArray a[NIN + POL_NOUT];
    for (int v = 0; v < NIN; ++v) a[v] = stage_array(warm && v >= NREQ ? nullptr : h.in[v], nz, STAGE_UP);
    for (int v = 0; v < POL_NOUT; ++v) a[NIN + v] = stage_array(h.out[v], nz, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    PolCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[v]);
    for (int v = 0; v < POL_NOUT; ++v) d.out[v] = staged<T>(a[NIN + v]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_pol<T>(ctx, tab, n, nz, d, ctx->stream); });
}
}  // namespace

extern "C" {
void kidmp_pol_defaults(kidmp_pol_cfg *cfg)
{
    if (!cfg) return;
    const PolCfg p = pol_defaults();
    *cfg = kidmp_pol_cfg{{p.axis_r[0], p.axis_r[1], p.axis_r[2], p.axis_r[3], p.axis_r[4]}, p.axis_r_min, p.axis_s, p.axis_g,
                         {p.sigma[0], p.sigma[1], p.sigma[2]}, 0};
}

int kidmp_pol_spheroid(double eps_re, double eps_im, double ratio, double sigma, double *rows7_per_unit_D)
{
    const std::string w("kidmp_pol_spheroid");
    if (!rows7_per_unit_D) return fail(nullptr, KIDMP_EINVAL, w + ": null argument");
    if (!(std::isfinite(eps_re) && std::isfinite(eps_im) && std::isfinite(ratio) && std::isfinite(sigma)))
        return fail(nullptr, KIDMP_EINVAL, w + ": an argument is not finite");
    if (eps_im < 0. || (eps_im == 0. && !(eps_re > 0.))) return fail(nullptr, KIDMP_EINVAL, w + ": Im(eps) must not be below 0 and a real permittivity must be above 0");
    if (!(ratio > 0. && ratio <= 1.)) return fail(nullptr, KIDMP_EINVAL, w + ": ratio outside (0, 1]");
    if (sigma < 0.) return fail(nullptr, KIDMP_EINVAL, w + ": sigma must not be below 0");
    double r[POL_ROWS];
    pol_spheroid(BBComplex{eps_re, eps_im}, ratio, pol_moments(sigma), 1., r);
    r[POL_ROWS - 1] = 0.;
    std::memcpy(rows7_per_unit_D, r, sizeof(r));
    return KIDMP_OK;
}

int kidmp_pol_bins(const kidmp_mie_cfg *mie_cfg, const kidmp_pol_cfg *pol_cfg, int32_t species, int32_t nb, const double *D, double *rows)
{
    const std::string w("kidmp_pol_bins");
    if (!mie_cfg || !pol_cfg || !D || !rows) return fail(nullptr, KIDMP_EINVAL, w + ": null argument");
    if (const char *bad = mie_bad_cfg(*mie_cfg)) return fail(nullptr, KIDMP_EINVAL, w + ": " + bad);
    const PolCfg pc = pol_model_cfg(*pol_cfg);
    if (const char *bad = pol_bad_cfg(pc)) return fail(nullptr, KIDMP_EINVAL, w + ": " + bad);
    if (species < 0 || species >= MIE_NSPEC) return fail(nullptr, KIDMP_EINVAL, w + ": unknown species");
    if (nb < 1) return fail(nullptr, KIDMP_EINVAL, w + ": nb < 1");
    std::vector<double> r(size_t(POL_ROWS) * size_t(nb));
    if (!pol_bins(mie_model_cfg(*mie_cfg), pc, species, nb, D, r.data()))
        return fail(nullptr, KIDMP_EINVAL, w + ": a diameter is not finite or not above 0");
    std::memcpy(rows, r.data(), r.size() * sizeof(double));
    return KIDMP_OK;
}

int kidmp_pol_table_create(kidmp_ctx *ctx, const kidmp_mie_cfg *mie_cfg, const kidmp_pol_cfg *pol_cfg, const kidmp_mie_grids *grids,
                           kidmp_pol_table **table)
{
    const std::string w("kidmp_pol_table_create");
    if (table) *table = nullptr;
    if (int rc = require_ready(ctx)) return rc;
    if (!table) return fail(ctx, KIDMP_EINVAL, w + ": null argument");
    kidmp_pol_cfg g;
    if (pol_cfg) g = *pol_cfg;
    else kidmp_pol_defaults(&g);
    const PolCfg pc = pol_model_cfg(g);
    if (const char *bad = pol_bad_cfg(pc)) return fail(ctx, KIDMP_EINVAL, w + ": " + bad);
    MieTableData d;
    const auto bins = [&](const MieCfg &mc, int x, int nb, const double *D, double *rows) { return pol_bins(mc, pc, x, nb, D, rows); };
    if (int rc = mie_table_build(ctx, w, mie_cfg, grids, POL_ROWS, bins, &d)) return rc;
    kidmp_pol_table *t = new kidmp_pol_table;
    static_cast<MieTableData &>(*t) = d;
    t->pol = g;
    t->kfac = (90.e3 * MIE_PI) / d.cfg.wavelength;
    // the scalars: the ratios of the rows of the species' first bin, formed as the table's own first bin was
    const MieCfg mc = mie_model_cfg(d.cfg);
    for (int x = 0; x < MIE_NSPEC; ++x) {
        const double D0 = grids && grids->D[x] ? grids->D[x][0] : mie_bins_D(ctx->hb, x)[0];
        double r[POL_ROWS];
        (void)pol_bins(mc, pc, x, 1, &D0, r);
        t->uniform[x] = !g.force_quadrature && pol_uniform(x) ? 1 : 0;
        for (int i = 0; i < 4; ++i) t->scal[x][i] = r[i] / r[4];
        t->scal[x][4] = r[5] / r[6];
    }
    *table = t;
    return KIDMP_OK;
}

void kidmp_pol_table_destroy(kidmp_pol_table *table)
{
    if (!table) return;
    mie_table_free(table);
    delete table;
}

int kidmp_pol_table_get(const kidmp_pol_table *table, int32_t species, int32_t *nb, double *D, double *dD, double *rows,
                        kidmp_mie_cfg *mie_cfg, kidmp_pol_cfg *pol_cfg, int32_t *uniform, double *scalars)
{
    const std::string w("kidmp_pol_table_get");
    if (!table) return fail(nullptr, KIDMP_EINVAL, w + ": null table");
    if (int rc = mie_table_read(table, w, species, nb, D, dD, rows, mie_cfg)) return rc;
    if (pol_cfg) *pol_cfg = table->pol;
    if (uniform) *uniform = table->uniform[species];
    if (scalars) std::memcpy(scalars, table->scal[species], sizeof(table->scal[species]));
    return KIDMP_OK;
}

int kidmp_polarimetric_device(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz, const double *t, const double *p,
                              const double *qv, const double *qr, const double *nr, const double *qs, const double *qg,
                              const kidmp_pol_out *out, void *stream)
{ return pol_device<double>(ctx, "kidmp_polarimetric_device", table, ncol, nz, pol_call<double>(t, p, qv, qr, nr, qs, qg, out), stream); }
int kidmp32_polarimetric_device(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz, const float *t, const float *p,
                                const float *qv, const float *qr, const float *nr, const float *qs, const float *qg,
                                const kidmp32_pol_out *out, void *stream)
{ return pol_device<float>(ctx, "kidmp32_polarimetric_device", table, ncol, nz, pol_call<float>(t, p, qv, qr, nr, qs, qg, out), stream); }
int kidmp_polarimetric_host(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz, const double *t, const double *p,
                            const double *qv, const double *qr, const double *nr, const double *qs, const double *qg,
                            const kidmp_pol_out *out)
{ return pol_host<double>(ctx, "kidmp_polarimetric_host", table, ncol, nz, pol_call<double>(t, p, qv, qr, nr, qs, qg, out)); }
int kidmp32_polarimetric_host(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz, const float *t, const float *p,
                              const float *qv, const float *qr, const float *nr, const float *qs, const float *qg,
                              const kidmp32_pol_out *out)
{ return pol_host<float>(ctx, "kidmp32_polarimetric_host", table, ncol, nz, pol_call<float>(t, p, qv, qr, nr, qs, qg, out)); }
}  // extern "C"
