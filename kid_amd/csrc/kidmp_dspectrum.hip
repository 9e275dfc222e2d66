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

// host arrays: chunks of columns through the context's staging memory on its compute stream, one after the other
// (spectra_host of kidmp_spectra.hip).  A column's result does not depend on its batch, so any chunking gives the same
// bits.  The caller's grids go up once, only the inputs given go up per chunk and only what was asked for comes down.
template <class T>
int dspectrum_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DSpectrumCall<T> &h)
{
    if (int rc = check_dspectrum<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
    auto rows = [&](int v) { return v < NSPECTRA ? size_t(h.nv) : size_t(1); };   // profiles of nz values per column of output v
    size_t per_col = 0, b_grids = 0;                      // bytes of staging per column, and for the caller's grids
    for (int v = 0; v < NIN; ++v) per_col += h.in[v] ? size_t(nz) * sizeof(T) : 0;
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) per_col += h.out[v] ? rows(v) * size_t(nz) * sizeof(T) : 0;
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x)
        if (h.D[x]) b_grids += 2 * up256(size_t(h.nb[x]) * sizeof(double));
    int64_t CH = pick_host_chunk(ctx, ncol);
    const int64_t fit = int64_t((MAX_STAGE - b_grids - 256 * size_t(NIN + DSPECTRUM_NOUT)) / per_col);
    if (CH > fit) CH = fit > 0 ? fit : 1;
    const size_t b_prof = up256(size_t(CH) * size_t(nz) * sizeof(T));
    size_t need = b_grids;
    for (int v = 0; v < NIN; ++v) need += h.in[v] ? b_prof : 0;
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) need += h.out[v] ? up256(size_t(CH) * rows(v) * size_t(nz) * sizeof(T)) : 0;
    if (int rc = ensure_stage(ctx, need)) return rc;
    char *next = reinterpret_cast<char *>(ctx->d_stage);
    auto take = [&](size_t bytes) { char *p = next; next += bytes; return p; };
    DSpectrumCall<T> d{};
    d.v0 = h.v0; d.dv = h.dv; d.nv = h.nv;
    hipError_t e = hipSuccess;
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        d.nb[x] = h.nb[x];
        if (!h.D[x]) continue;
        const size_t b = size_t(h.nb[x]) * sizeof(double);
        double *dD_ = reinterpret_cast<double *>(take(up256(b))), *ddD_ = reinterpret_cast<double *>(take(up256(b)));
        if (e == hipSuccess) e = hipMemcpyAsync(dD_, h.D[x], b, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ddD_, h.dD[x], b, hipMemcpyHostToDevice, ctx->stream);
        d.D[x] = dD_;
        d.dD[x] = ddD_;
    }
    for (int v = 0; v < NIN; ++v) d.in[v] = h.in[v] ? reinterpret_cast<T *>(take(b_prof)) : nullptr;
    for (int v = 0; v < DSPECTRUM_NOUT; ++v)
        d.out[v] = h.out[v] ? reinterpret_cast<T *>(take(up256(size_t(CH) * rows(v) * size_t(nz) * sizeof(T)))) : nullptr;
    for (int64_t c0 = 0; c0 < ncol && e == hipSuccess; c0 += CH) {
        const int64_t n = c0 + CH <= ncol ? CH : ncol - c0;
        const size_t off = size_t(c0) * size_t(nz), cnt = size_t(n) * size_t(nz);
        for (int v = 0; v < NIN && e == hipSuccess; ++v)
            if (h.in[v]) e = hipMemcpyAsync(const_cast<T *>(d.in[v]), h.in[v] + off, cnt * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = enqueue_dspectrum<T>(ctx, n, nz, d, ctx->stream);
        for (int v = 0; v < DSPECTRUM_NOUT && e == hipSuccess; ++v)
            if (h.out[v]) e = hipMemcpyAsync(h.out[v] + off * rows(v), d.out[v], cnt * rows(v) * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);        // no copy may still be in flight towards the caller's arrays
    HIPTRY(ctx, e);
    HIPTRY(ctx, es);
    return KIDMP_OK;
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
