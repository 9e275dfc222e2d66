// kidmp_brightband.hip -- the entries of include/kidmp_brightband.h: the reflectivity with its melting layer of device
// arrays in one launch of k_bright_band (thompson_reflectivity.hip), and of host arrays in chunks through the context's
// staging memory.
#include <cmath>
#include <cstddef>

#include "kidmp_ctx.h"
#include "../../include/kidmp_brightband.h"

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
