// kidmp_spectra.hip -- the entries of include/kidmp_spectra.h: each species' distribution parameters and its numbers per
// diameter bin, of device arrays in one launch of k_size_spectra (thompson_reflectivity.hip), and of host arrays in chunks
// through the context's staging memory.
#include <cstddef>

#include "kidmp_ctx.h"
#include "../../include/kidmp_spectra.h"

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
