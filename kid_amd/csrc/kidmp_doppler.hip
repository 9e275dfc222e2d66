// kidmp_doppler.hip -- the entries of include/kidmp_doppler.h: reflectivity, mean Doppler velocity and spectrum width of
// device arrays in one launch of k_doppler_moments (thompson_reflectivity.hip), and of host arrays in chunks through the
// context's staging memory.
#include "kidmp_ctx.h"
#include "../../include/kidmp_doppler.h"

using namespace kidmp;

static_assert(sizeof(kidmp_doppler_out) == DOPPLER_NOUT * sizeof(double *) && sizeof(kidmp32_doppler_out) == DOPPLER_NOUT * sizeof(float *),
              "include/kidmp_doppler.h");

namespace {
constexpr int NIN = 8, NREQ = 5;                          // t, p, qv, qr, nr | qs, qg, w
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qr", "nr", "qs", "qg", "w"};
const char *const OUT_NAMES[DOPPLER_NOUT] = {"dbz", "vd", "sw", "vz_r", "vz_s", "vz_g", "dbz_r", "dbz_s", "dbz_g"};

template <class T> struct DopplerCall {
    const T *in[NIN];
    T *out[DOPPLER_NOUT];
};
template <class T, class O>
DopplerCall<T> doppler_call(const T *t, const T *p, const T *qv, const T *qr, const T *nr, const T *qs, const T *qg, const T *w, const O *out)
{
    DopplerCall<T> c{{t, p, qv, qr, nr, qs, qg, w}, {}};
    if (out) {
        T *const o[DOPPLER_NOUT] = {out->dbz, out->vd, out->sw, out->vz_r, out->vz_s, out->vz_g, out->dbz_r, out->dbz_s, out->dbz_g};
        for (int v = 0; v < DOPPLER_NOUT; ++v) c.out[v] = o[v];
    }
    return c;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_doppler(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DopplerCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = false;
    for (int v = 0; v < DOPPLER_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: out is NULL or every member is");
    for (int v = 0; v < NREQ; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (!doppler_consts_supported(ctx->hc)) return fail(ctx, KIDMP_ESTATE, w + ": exponents differ from the kernel's");
    return KIDMP_OK;
}

template <class T>
hipError_t enqueue_doppler(kidmp_ctx *ctx, int64_t ncol, int nz, const DopplerCall<T> &a, hipStream_t s)
{
    const T *const *q = a.in;
    DopplerArgs<T> args{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], {}};
    for (int v = 0; v < DOPPLER_NOUT; ++v) args.out[v] = a.out[v];
    return launch_doppler_moments<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int doppler_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DopplerCall<T> &a, void *stream)
{
    if (int rc = check_doppler<T>(ctx, who, ncol, nz, a)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NIN; ++v)
        if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    for (int v = 0; v < DOPPLER_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], OUT_NAMES[v])) return rc;
    HIPTRY(ctx, enqueue_doppler<T>(ctx, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: chunks of columns through the context's staging memory on its compute stream, one after the other
// (fall_host of kidmp_fall.hip).  A column's result does not depend on its batch, so any chunking gives the same bits.
// Only the inputs given go up and only what was asked for comes down.
template <class T>
int doppler_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DopplerCall<T> &h)
{
    if (int rc = check_doppler<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const int64_t CH = pick_host_chunk(ctx, ncol);
    const size_t b_prof = (size_t(CH) * size_t(nz) * sizeof(T) + 255) / 256 * 256;
    int slots = 0;
    for (int v = 0; v < NIN; ++v) slots += h.in[v] != nullptr;
    for (int v = 0; v < DOPPLER_NOUT; ++v) slots += h.out[v] != nullptr;
    if (int rc = ensure_stage(ctx, size_t(slots) * b_prof)) return rc;
    char *next = reinterpret_cast<char *>(ctx->d_stage);
    auto slot = [&](bool wanted) { T *p = wanted ? reinterpret_cast<T *>(next) : nullptr; if (wanted) next += b_prof; return p; };
    DopplerCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = slot(h.in[v] != nullptr);
    for (int v = 0; v < DOPPLER_NOUT; ++v) d.out[v] = slot(h.out[v] != nullptr);
    hipError_t e = hipSuccess;
    for (int64_t c0 = 0; c0 < ncol && e == hipSuccess; c0 += CH) {
        const int64_t n = c0 + CH <= ncol ? CH : ncol - c0;
        const size_t off = size_t(c0) * size_t(nz), cnt = size_t(n) * size_t(nz);
        for (int v = 0; v < NIN && e == hipSuccess; ++v)
            if (h.in[v]) e = hipMemcpyAsync(const_cast<T *>(d.in[v]), h.in[v] + off, cnt * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = enqueue_doppler<T>(ctx, n, nz, d, ctx->stream);
        for (int v = 0; v < DOPPLER_NOUT && e == hipSuccess; ++v)
            if (h.out[v]) e = hipMemcpyAsync(h.out[v] + off, d.out[v], cnt * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);        // no copy may still be in flight towards the caller's arrays
    HIPTRY(ctx, e);
    HIPTRY(ctx, es);
    return KIDMP_OK;
}
}  // namespace

extern "C" {
int kidmp_doppler_moments_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                 const double *qr, const double *nr, const double *qs, const double *qg, const double *w,
                                 const kidmp_doppler_out *out, void *stream)
{
    return doppler_device<double>(ctx, "kidmp_doppler_moments_device", ncol, nz, doppler_call<double>(t, p, qv, qr, nr, qs, qg, w, out), stream);
}
int kidmp32_doppler_moments_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                   const float *qr, const float *nr, const float *qs, const float *qg, const float *w,
                                   const kidmp32_doppler_out *out, void *stream)
{
    return doppler_device<float>(ctx, "kidmp32_doppler_moments_device", ncol, nz, doppler_call<float>(t, p, qv, qr, nr, qs, qg, w, out), stream);
}
int kidmp_doppler_moments_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                               const double *qr, const double *nr, const double *qs, const double *qg, const double *w,
                               const kidmp_doppler_out *out)
{
    return doppler_host<double>(ctx, "kidmp_doppler_moments_host", ncol, nz, doppler_call<double>(t, p, qv, qr, nr, qs, qg, w, out));
}
int kidmp32_doppler_moments_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                 const float *qr, const float *nr, const float *qs, const float *qg, const float *w,
                                 const kidmp32_doppler_out *out)
{
    return doppler_host<float>(ctx, "kidmp32_doppler_moments_host", ncol, nz, doppler_call<float>(t, p, qv, qr, nr, qs, qg, w, out));
}
}  // extern "C"
