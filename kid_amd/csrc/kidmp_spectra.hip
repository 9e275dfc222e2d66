// kidmp_spectra.hip -- the entries of include/kidmp_spectra.h: each species' distribution parameters and its numbers per
// diameter bin, of device arrays in one launch of k_size_spectra (below), and of host arrays in chunks
// through the context's staging memory.
#include <cstddef>

#include "kidmp_ctx.h"
#include "../../include/kidmp_spectra.h"

#include "kidmp_column.h"

namespace kidmp {

// The size spectra (include/kidmp_spectra.h): each species' distribution parameters [ncol][nz] and its numbers per bin
// [ncol][nb][nz].  Species in the order c, i, r, s, g; par in the order of kidmp_spectra_out.  Null means: nc -- Nt_c (the
// context is not aerosol-aware); qi and ni, qs, qg -- the species is absent everywhere (iiwarm); an output -- not wanted;
// set_nc_col -- the context's Nt_c.  D, dD: device arrays of nb[x] doubles, read only where spec[x] is wanted.
constexpr int SPECTRA_NPAR = 11;                    // SPECTRA_NSPEC: kidmp_column.h
constexpr int SPECTRA_LAM_C = 0, SPECTRA_LAM_I = 3, SPECTRA_LAM_R = 5, SPECTRA_SMOB = 7, SPECTRA_LAM_G = 9;   // each followed by its n0 / smoc (and nu_c)
constexpr int SPECTRA_MAX_SHARES = 16, SPECTRA_MIN_BLOCKS = 1024;
template <class T> struct SpectraArgs {
    const T *t, *p, *qv, *qc, *nc, *qi, *ni, *qr, *nr, *qs, *qg;
    T *par[SPECTRA_NPAR];
    T *spec[SPECTRA_NSPEC];
    const double *D[SPECTRA_NSPEC], *dD[SPECTRA_NSPEC];
    int32_t nb[SPECTRA_NSPEC];
    const double *set_nc_col;                        // null, or the batch's share of a bound per-column droplet number (cm**-3)
    int aero;                                        // the context's is_aerosol_aware: nc is read and size-limited (M:1398-1409)
};

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
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
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

namespace {
// d_consts: the context's Consts in device memory (kidmp_ctx::d_consts)
template <class T>
hipError_t launch_size_spectra(const Consts *c, int64_t ncol, int nz, const SpectraArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // no column group: nothing to share out
    const int64_t nblk = column_grid(ncol).x;
    // few columns and many bins: a column's bins go to several blocks, up to SPECTRA_MAX_SHARES, until the grid holds
    // SPECTRA_MIN_BLOCKS workgroups (four to a compute unit)
    int maxnb = 1;
    for (int x = 0; x < SPECTRA_NSPEC; ++x)
        if (a.spec[x] && a.nb[x] > maxnb) maxnb = a.nb[x];
    int64_t shares = (SPECTRA_MIN_BLOCKS + nblk - 1) / nblk;
    shares = shares > SPECTRA_MAX_SHARES ? SPECTRA_MAX_SHARES : shares;
    shares = shares > maxnb ? maxnb : shares;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_size_spectra<T, NJ>), column_grid(ncol, (unsigned)shares), dim3(REFL_THREADS), 0, s,
                           c, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

using namespace kidmp;

static_assert(sizeof(kidmp_spectra_out) == SPECTRA_NPAR * sizeof(double *) && sizeof(kidmp32_spectra_out) == SPECTRA_NPAR * sizeof(float *)
                  && sizeof(kidmp_spectra_bins) == SPECTRA_NSPEC * sizeof(double *) && sizeof(kidmp32_spectra_bins) == SPECTRA_NSPEC * sizeof(float *)
                  && SPECTRA_NSPEC == KIDMP_SPECTRA_NSPECIES && nbins == KIDMP_SPECTRA_DEFAULT_BINS && nbins <= KIDMP_SPECTRA_MAX_BINS,
              "include/kidmp_spectra.h");

namespace {
constexpr int NIN = 11;                                   // t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg"};
const char *const PAR_NAMES[SPECTRA_NPAR] = {"lam_c", "n0_c", "nu_c", "lam_i", "n0_i", "lam_r", "n0_r", "smob", "smoc", "lam_g", "n0_g"};
const char *const BIN_NAMES[SPECTRA_NSPEC] = {"n_c", "n_i", "n_r", "n_s", "n_g"};
constexpr bool REQUIRED[NIN] = {true, true, true, true, false, false, false, true, true, false, false};
constexpr bool FROZEN_IN[NIN] = {false, false, false, false, false, true, true, false, false, true, true};
constexpr int SPECIES_OF_PAR[SPECTRA_NPAR] = {0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4};
constexpr size_t MAX_STAGE = size_t(256) << 20;           // the host entries' staging: chunks are sized to stay below it

// the scheme's own grid of a species inside a Bins (host or device copy alike)
const double *bins_D(const Bins *b, int x) { return x == 0 ? b->Dc : x == 1 ? b->Di : x == 2 ? b->Dr : x == 3 ? b->Ds : b->Dg; }
const double *bins_dD(const Bins *b, int x) { return x == 0 ? b->dtc : x == 1 ? b->dti : x == 2 ? b->dtr : x == 3 ? b->dts : b->dtg; }

template <class T> struct SpectraCall {
    const T *in[NIN];
    T *par[SPECTRA_NPAR];
    T *spec[SPECTRA_NSPEC];
    const double *D[SPECTRA_NSPEC], *dD[SPECTRA_NSPEC];   // the caller's; both null: the scheme's own
    int32_t nb[SPECTRA_NSPEC];
};
template <class T, class P, class B>
SpectraCall<T> spectra_call(const T *t, const T *p, const T *qv, const T *qc, const T *nc, const T *qi, const T *ni, const T *qr, const T *nr,
                            const T *qs, const T *qg, const P *par, const B *bins, const kidmp_spectra_grids *grids)
{
    SpectraCall<T> c{{t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg}, {}, {}, {}, {}, {}};
    if (par) {
        T *const o[SPECTRA_NPAR] = {par->lam_c, par->n0_c, par->nu_c, par->lam_i, par->n0_i, par->lam_r, par->n0_r, par->smob, par->smoc,
                                    par->lam_g, par->n0_g};
        for (int v = 0; v < SPECTRA_NPAR; ++v) c.par[v] = o[v];
    }
    if (bins) {
        T *const o[SPECTRA_NSPEC] = {bins->n_c, bins->n_i, bins->n_r, bins->n_s, bins->n_g};
        for (int x = 0; x < SPECTRA_NSPEC; ++x) c.spec[x] = o[x];
    }
    for (int x = 0; x < SPECTRA_NSPEC; ++x) {
        c.nb[x] = nbins;
        if (grids && (grids->D[x] || grids->dD[x])) { c.D[x] = grids->D[x]; c.dD[x] = grids->dD[x]; c.nb[x] = grids->nb[x]; }
    }
    return c;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_spectra(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const SpectraCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool wanted[SPECTRA_NSPEC] = {};
    for (int v = 0; v < SPECTRA_NPAR; ++v) wanted[SPECIES_OF_PAR[v]] |= a.par[v] != nullptr;
    for (int x = 0; x < SPECTRA_NSPEC; ++x) wanted[x] |= a.spec[x] != nullptr;
    if (!(wanted[0] || wanted[1] || wanted[2] || wanted[3] || wanted[4]))
        return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: every parameter and every spectrum are NULL");
    for (int v = 0; v < NIN; ++v)
        if (REQUIRED[v] && !a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (!ctx->cfg.iiwarm && (wanted[1] || wanted[3] || wanted[4]))
        for (int v = 0; v < NIN; ++v)
            if (FROZEN_IN[v] && !a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": a frozen output in a mixed-phase context needs qi, ni, qs and qg");
    if (ctx->cfg.is_aerosol_aware && wanted[0] && !a.in[4]) return fail(ctx, KIDMP_EINVAL, w + ": an aerosol-aware context needs nc for cloud water");
    for (int x = 0; x < SPECTRA_NSPEC; ++x) {
        if (!a.spec[x]) continue;
        if ((a.D[x] == nullptr) != (a.dD[x] == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": a grid needs both D and dD");
        if (a.nb[x] < 1 || a.nb[x] > KIDMP_SPECTRA_MAX_BINS) return fail(ctx, KIDMP_EINVAL, w + ": nb outside [1, KIDMP_SPECTRA_MAX_BINS]");
    }
    if (wanted[0])
        if (int rc = check_nc_count(ctx, who, ncol)) return rc;
    if (!spectra_consts_supported(ctx->hc)) return fail(ctx, KIDMP_ESTATE, w + ": size-distribution exponents differ from the kernel's");
    return KIDMP_OK;
}

// one launch over device pointers; nc_first: the batch's first column within a bound per-column droplet number.  An
// iiwarm context reads no frozen input; a context that is not aerosol-aware does not read nc.
template <class T>
hipError_t enqueue_spectra(kidmp_ctx *ctx, int64_t ncol, int nz, const SpectraCall<T> &a, int64_t nc_first, hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0, aero = ctx->cfg.is_aerosol_aware != 0;
    const T *const *q = a.in;
    SpectraArgs<T> args{q[0], q[1], q[2], q[3], aero ? q[4] : nullptr, warm ? nullptr : q[5], warm ? nullptr : q[6], q[7], q[8],
                        warm ? nullptr : q[9], warm ? nullptr : q[10], {}, {}, {}, {}, {}, ctx->d_nc_col ? ctx->d_nc_col + nc_first : nullptr,
                        aero ? 1 : 0};
    for (int v = 0; v < SPECTRA_NPAR; ++v) args.par[v] = a.par[v];
    for (int x = 0; x < SPECTRA_NSPEC; ++x) {
        args.spec[x] = a.spec[x];
        args.D[x] = a.D[x] ? a.D[x] : bins_D(ctx->d_bins, x);
        args.dD[x] = a.dD[x] ? a.dD[x] : bins_dD(ctx->d_bins, x);
        args.nb[x] = a.D[x] ? a.nb[x] : nbins;
    }
    return launch_size_spectra<T>(ctx->d_consts, ncol, nz, args, s);
}

template <class T>
int spectra_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const SpectraCall<T> &a, void *stream)
{
    if (int rc = check_spectra<T>(ctx, who, ncol, nz, a)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0;
    for (int v = 0; v < NIN; ++v)
        if (!(warm && FROZEN_IN[v]))
            if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    for (int v = 0; v < SPECTRA_NPAR; ++v)
        if (int rc = check_device_array(ctx, who, a.par[v], PAR_NAMES[v])) return rc;
    for (int x = 0; x < SPECTRA_NSPEC; ++x) {
        if (!a.spec[x]) continue;
        if (int rc = check_device_array(ctx, who, a.spec[x], BIN_NAMES[x])) return rc;
        if (int rc = check_device_array(ctx, who, a.D[x], "D")) return rc;
        if (int rc = check_device_array(ctx, who, a.dD[x], "dD")) return rc;
    }
    HIPTRY(ctx, enqueue_spectra<T>(ctx, ncol, nz, a, 0, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip, the chunk narrowed to stay below MAX_STAGE.  The caller's grids go up once,
// only what the kernel reads goes up per chunk and only what was asked for comes down.
template <class T>
int spectra_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const SpectraCall<T> &h)
{
    if (int rc = check_spectra<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0, aero = ctx->cfg.is_aerosol_aware != 0;
    constexpr int A_D = 0, A_DD = SPECTRA_NSPEC, A_IN = 2 * SPECTRA_NSPEC, A_PAR = A_IN + NIN, A_SPEC = A_PAR + SPECTRA_NPAR;
    StageArray a[A_SPEC + SPECTRA_NSPEC];
    for (int x = 0; x < SPECTRA_NSPEC; ++x) {                 // a grid travels with its spectrum alone
        a[A_D + x] = stage_once(h.spec[x] ? h.D[x] : nullptr, h.nb[x]);
        a[A_DD + x] = stage_once(h.spec[x] ? h.dD[x] : nullptr, h.nb[x]);
        a[A_SPEC + x] = stage_array(h.spec[x], int64_t(h.nb[x]) * nz, STAGE_DOWN);
    }
    for (int v = 0; v < NIN; ++v) a[A_IN + v] = stage_array((warm && FROZEN_IN[v]) || (v == 4 && !aero) ? nullptr : h.in[v], nz, STAGE_UP);
    for (int v = 0; v < SPECTRA_NPAR; ++v) a[A_PAR + v] = stage_array(h.par[v], nz, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol), MAX_STAGE);
    if (int rc = stage_open(ctx, plan)) return rc;
    SpectraCall<T> d{};
    for (int x = 0; x < SPECTRA_NSPEC; ++x) {
        d.nb[x] = h.nb[x];
        d.D[x] = staged<double>(a[A_D + x]);
        d.dD[x] = staged<double>(a[A_DD + x]);
        d.spec[x] = staged<T>(a[A_SPEC + x]);
    }
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[A_IN + v]);
    for (int v = 0; v < SPECTRA_NPAR; ++v) d.par[v] = staged<T>(a[A_PAR + v]);
    return stage_run(ctx, plan, [&](int64_t c0, int64_t n) { return enqueue_spectra<T>(ctx, n, nz, d, c0, ctx->stream); });
}
}  // namespace

extern "C" {
int kidmp_spectra_default_grid(kidmp_ctx *ctx, int32_t species, double *D, double *dD, int32_t cap)
{
    const char *who = "kidmp_spectra_default_grid";
    if (int rc = require_ready(ctx)) return rc;
    if (species < 0 || species >= SPECTRA_NSPEC) return fail(ctx, KIDMP_EINVAL, std::string(who) + ": species outside [0, KIDMP_SPECTRA_NSPECIES)");
    if (!D && !dD) return nbins;
    if (!D || !dD) return fail(ctx, KIDMP_EINVAL, std::string(who) + ": a grid needs both D and dD");
    if (cap < nbins) return fail(ctx, KIDMP_EINVAL, std::string(who) + ": cap is smaller than the grid");
    std::memcpy(D, bins_D(&ctx->hb, species), nbins * sizeof(double));
    std::memcpy(dD, bins_dD(&ctx->hb, species), nbins * sizeof(double));
    return nbins;
}
int kidmp_size_spectra_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                              const double *qc, const double *nc, const double *qi, const double *ni, const double *qr, const double *nr,
                              const double *qs, const double *qg, const kidmp_spectra_out *par, const kidmp_spectra_bins *bins,
                              const kidmp_spectra_grids *grids, void *stream)
{
    return spectra_device<double>(ctx, "kidmp_size_spectra_device", ncol, nz,
                                  spectra_call<double>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, par, bins, grids), stream);
}
int kidmp32_size_spectra_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                const float *qc, const float *nc, const float *qi, const float *ni, const float *qr, const float *nr,
                                const float *qs, const float *qg, const kidmp32_spectra_out *par, const kidmp32_spectra_bins *bins,
                                const kidmp_spectra_grids *grids, void *stream)
{
    return spectra_device<float>(ctx, "kidmp32_size_spectra_device", ncol, nz,
                                 spectra_call<float>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, par, bins, grids), stream);
}
int kidmp_size_spectra_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                            const double *qc, const double *nc, const double *qi, const double *ni, const double *qr, const double *nr,
                            const double *qs, const double *qg, const kidmp_spectra_out *par, const kidmp_spectra_bins *bins,
                            const kidmp_spectra_grids *grids)
{
    return spectra_host<double>(ctx, "kidmp_size_spectra_host", ncol, nz,
                                spectra_call<double>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, par, bins, grids));
}
int kidmp32_size_spectra_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                              const float *qc, const float *nc, const float *qi, const float *ni, const float *qr, const float *nr,
                              const float *qs, const float *qg, const kidmp32_spectra_out *par, const kidmp32_spectra_bins *bins,
                              const kidmp_spectra_grids *grids)
{
    return spectra_host<float>(ctx, "kidmp32_size_spectra_host", ncol, nz,
                               spectra_call<float>(t, p, qv, qc, nc, qi, ni, qr, nr, qs, qg, par, bins, grids));
}
}  // extern "C"
