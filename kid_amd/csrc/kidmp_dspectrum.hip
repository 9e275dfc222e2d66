// kidmp_dspectrum.hip -- the entries of include/kidmp_dspectrum.h: the Doppler spectrum of device arrays in one launch of
// k_doppler_spectrum (thompson_reflectivity.hip), and of host arrays in chunks through the context's staging memory.
#include <cmath>
#include <cstddef>

#include "kidmp_ctx.h"
#include "../../include/kidmp_dspectrum.h"

using namespace kidmp;

static_assert(sizeof(kidmp_dspectrum_out) == DSPECTRUM_NOUT * sizeof(double *) && sizeof(kidmp32_dspectrum_out) == DSPECTRUM_NOUT * sizeof(float *)
                  && DSPECTRUM_NSPEC == KIDMP_DSPECTRUM_NSPECIES && DSPECTRUM_MAX_NV == KIDMP_DSPECTRUM_MAX_NV && nbins <= KIDMP_DSPECTRUM_MAX_BINS,
              "include/kidmp_dspectrum.h");

namespace {
constexpr int NIN = 8, NREQ = 5, NSPECTRA = 4;            // t, p, qv, qr, nr | qs, qg, w;  total, rain, snow, graupel | below, above
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qr", "nr", "qs", "qg", "w"};
const char *const OUT_NAMES[DSPECTRUM_NOUT] = {"total", "rain", "snow", "graupel", "below", "above"};
constexpr size_t MAX_STAGE = size_t(256) << 20;           // the host entries' staging: chunks are sized to stay below it

// the scheme's own grid of a species inside a Bins (host or device copy alike): rain, snow, graupel
const double *bins_D(const Bins *b, int x) { return x == 0 ? b->Dr : x == 1 ? b->Ds : b->Dg; }
const double *bins_dD(const Bins *b, int x) { return x == 0 ? b->dtr : x == 1 ? b->dts : b->dtg; }

template <class T> struct DSpectrumCall {
    const T *in[NIN];
    T *out[DSPECTRUM_NOUT];
    const double *D[DSPECTRUM_NSPEC], *dD[DSPECTRUM_NSPEC];   // the caller's; both null: the scheme's own
    int32_t nb[DSPECTRUM_NSPEC];
    double v0, dv;
    int32_t nv;
};
template <class T, class O>
DSpectrumCall<T> dspectrum_call(const T *t, const T *p, const T *qv, const T *qr, const T *nr, const T *qs, const T *qg, const T *w,
                                double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const O *out)
{
    DSpectrumCall<T> c{{t, p, qv, qr, nr, qs, qg, w}, {}, {}, {}, {}, v0, dv, nv};
    if (out) {
        T *const o[DSPECTRUM_NOUT] = {out->total, out->rain, out->snow, out->graupel, out->below, out->above};
        for (int v = 0; v < DSPECTRUM_NOUT; ++v) c.out[v] = o[v];
    }
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        c.nb[x] = nbins;
        if (grids && (grids->D[x] || grids->dD[x])) { c.D[x] = grids->D[x]; c.dD[x] = grids->dD[x]; c.nb[x] = grids->nb[x]; }
    }
    return c;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_dspectrum(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DSpectrumCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (a.nv < 1 || a.nv > KIDMP_DSPECTRUM_MAX_NV) return fail(ctx, KIDMP_EINVAL, w + ": nv outside [1, KIDMP_DSPECTRUM_MAX_NV]");
    if (!(a.dv > 0.) || !std::isfinite(a.dv) || !std::isfinite(1. / a.dv)) return fail(ctx, KIDMP_EINVAL, w + ": dv must be finite and above 0");
    if (!std::isfinite(a.v0)) return fail(ctx, KIDMP_EINVAL, w + ": v0 must be finite");
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        if ((a.D[x] == nullptr) != (a.dD[x] == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": a grid needs both D and dD");
        if (a.nb[x] < 1 || a.nb[x] > KIDMP_DSPECTRUM_MAX_BINS) return fail(ctx, KIDMP_EINVAL, w + ": nb outside [1, KIDMP_DSPECTRUM_MAX_BINS]");
    }
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = false;
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: out is NULL or every member is");
    for (int v = 0; v < NREQ; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (!doppler_consts_supported(ctx->hc) || !spectra_consts_supported(ctx->hc))
        return fail(ctx, KIDMP_ESTATE, w + ": exponents differ from the kernel's");
    return KIDMP_OK;
}

// one launch over device pointers
template <class T>
hipError_t enqueue_dspectrum(kidmp_ctx *ctx, int64_t ncol, int nz, const DSpectrumCall<T> &a, hipStream_t s)
{
    const T *const *q = a.in;
    DSpectrumArgs<T> args{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], {}, {}, {}, {}, a.v0, 1. / a.dv, a.nv};
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) args.out[v] = a.out[v];
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        args.D[x] = a.D[x] ? a.D[x] : bins_D(ctx->d_bins, x);
        args.dD[x] = a.dD[x] ? a.dD[x] : bins_dD(ctx->d_bins, x);
        args.nb[x] = a.D[x] ? a.nb[x] : nbins;
    }
    return launch_doppler_spectrum<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int dspectrum_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DSpectrumCall<T> &a, void *stream)
{
    if (int rc = check_dspectrum<T>(ctx, who, ncol, nz, a)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NIN; ++v)
        if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    for (int v = 0; v < DSPECTRUM_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], OUT_NAMES[v])) return rc;
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        if (int rc = check_device_array(ctx, who, a.D[x], "D")) return rc;
        if (int rc = check_device_array(ctx, who, a.dD[x], "dD")) return rc;
    }
    HIPTRY(ctx, enqueue_dspectrum<T>(ctx, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip, the chunk narrowed to stay below MAX_STAGE.  The caller's grids go up once,
// only the inputs given go up per chunk and only what was asked for comes down.
template <class T>
int dspectrum_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DSpectrumCall<T> &h)
{
    if (int rc = check_dspectrum<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    constexpr int A_D = 0, A_DD = DSPECTRUM_NSPEC, A_IN = 2 * DSPECTRUM_NSPEC, A_OUT = A_IN + NIN;
    StageArray a[A_OUT + DSPECTRUM_NOUT];
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        a[A_D + x] = stage_once(h.D[x], h.nb[x]);
        a[A_DD + x] = stage_once(h.dD[x], h.nb[x]);
    }
    for (int v = 0; v < NIN; ++v) a[A_IN + v] = stage_array(h.in[v], nz, STAGE_UP);
    for (int v = 0; v < DSPECTRUM_NOUT; ++v)                  // the spectra have nv profiles of nz values per column
        a[A_OUT + v] = stage_array(h.out[v], int64_t(v < NSPECTRA ? h.nv : 1) * nz, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol), MAX_STAGE);
    if (int rc = stage_open(ctx, plan)) return rc;
    DSpectrumCall<T> d{};
    d.v0 = h.v0; d.dv = h.dv; d.nv = h.nv;
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        d.nb[x] = h.nb[x];
        d.D[x] = staged<double>(a[A_D + x]);
        d.dD[x] = staged<double>(a[A_DD + x]);
    }
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[A_IN + v]);
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) d.out[v] = staged<T>(a[A_OUT + v]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_dspectrum<T>(ctx, n, nz, d, ctx->stream); });
}
}  // namespace

extern "C" {
int kidmp_doppler_spectrum_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                  const double *qr, const double *nr, const double *qs, const double *qg, const double *w,
                                  double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp_dspectrum_out *out,
                                  void *stream)
{
    return dspectrum_device<double>(ctx, "kidmp_doppler_spectrum_device", ncol, nz,
                                    dspectrum_call<double>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out), stream);
}
int kidmp32_doppler_spectrum_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                    const float *qr, const float *nr, const float *qs, const float *qg, const float *w,
                                    double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp32_dspectrum_out *out,
                                    void *stream)
{
    return dspectrum_device<float>(ctx, "kidmp32_doppler_spectrum_device", ncol, nz,
                                   dspectrum_call<float>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out), stream);
}
int kidmp_doppler_spectrum_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                const double *qr, const double *nr, const double *qs, const double *qg, const double *w,
                                double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp_dspectrum_out *out)
{
    return dspectrum_host<double>(ctx, "kidmp_doppler_spectrum_host", ncol, nz,
                                  dspectrum_call<double>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out));
}
int kidmp32_doppler_spectrum_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                  const float *qr, const float *nr, const float *qs, const float *qg, const float *w,
                                  double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp32_dspectrum_out *out)
{
    return dspectrum_host<float>(ctx, "kidmp32_doppler_spectrum_host", ncol, nz,
                                 dspectrum_call<float>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out));
}
}  // extern "C"
