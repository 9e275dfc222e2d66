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

// host arrays: stage_run of kidmp_host.hip.  Only the inputs given go up and only what was asked for comes down.
template <class T>
int doppler_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DopplerCall<T> &h)
{
    if (int rc = check_doppler<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    StageArray a[NIN + DOPPLER_NOUT];
    for (int v = 0; v < NIN; ++v) a[v] = stage_array(h.in[v], nz, STAGE_UP);
    for (int v = 0; v < DOPPLER_NOUT; ++v) a[NIN + v] = stage_array(h.out[v], nz, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    DopplerCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[v]);
    for (int v = 0; v < DOPPLER_NOUT; ++v) d.out[v] = staged<T>(a[NIN + v]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_doppler<T>(ctx, n, nz, d, ctx->stream); });
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
