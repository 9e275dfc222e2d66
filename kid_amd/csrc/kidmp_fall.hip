// kidmp_fall.hip -- the entries of include/kidmp_fall.h: block-O fall speeds, sedimentation fluxes and CFL substep counts
// of device arrays in one launch of k_fall_speeds (thompson_reflectivity.hip), and of host arrays in chunks through the
// context's staging memory.
#include "kidmp_ctx.h"
#include "../../include/kidmp_fall.h"

using namespace kidmp;

static_assert(sizeof(kidmp_fall_out) == FALL_NOUT * sizeof(double *) && sizeof(kidmp32_fall_out) == FALL_NOUT * sizeof(float *),
              "include/kidmp_fall.h");

namespace {
constexpr int NIN = 10;                                   // t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qr", "nr", "qi", "ni", "qs", "qg", "vts_boost"};
const char *const OUT_NAMES[FALL_NOUT] = {"vt_r", "vt_nr", "vt_i", "vt_ni", "vt_s", "vt_g", "flux_r", "flux_i", "flux_s", "flux_g", "flux_total"};

template <class T> struct FallCall {
    const T *in[NIN];
    const T *dz;
    int64_t dz_col_stride;
    double dt;
    T *out[FALL_NOUT];
    int32_t *nstep;
};
template <class T, class O>
FallCall<T> fall_call(const T *t, const T *p, const T *qv, const T *qr, const T *nr, const T *qi, const T *ni, const T *qs, const T *qg,
                      const T *boost, const T *dz, int64_t dz_col_stride, double dt, const O *out, int32_t *nstep)
{
    FallCall<T> c{{t, p, qv, qr, nr, qi, ni, qs, qg, boost}, dz, dz_col_stride, dt, {}, nstep};
    if (out) {
        T *const o[FALL_NOUT] = {out->vt_r, out->vt_nr, out->vt_i, out->vt_ni, out->vt_s, out->vt_g, out->flux_r, out->flux_i, out->flux_s,
                                 out->flux_g, out->flux_total};
        for (int v = 0; v < FALL_NOUT; ++v) c.out[v] = o[v];
    }
    return c;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_fall(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const FallCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = a.nstep != nullptr;
    for (int v = 0; v < FALL_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: every output and nstep are NULL");
    for (int v = 0; v < 5; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (!ctx->cfg.iiwarm)
        for (int v = 5; v < 9; ++v)
            if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": a mixed-phase context needs qi, ni, qs and qg");
    if (a.nstep) {
        if (!a.dz) return fail(ctx, KIDMP_EINVAL, w + ": nstep needs dz");
        if (!(a.dt > 0.)) return fail(ctx, KIDMP_EINVAL, w + ": nstep needs dt > 0");
        if (a.dz_col_stride != 0 && a.dz_col_stride < nz) return fail(ctx, KIDMP_EINVAL, w + ": dz_col_stride must be 0 or >= nz");
    }
    if (!fall_consts_supported(ctx->hc)) return fail(ctx, KIDMP_ESTATE, w + ": fall-speed exponents differ from the kernel's");
    return KIDMP_OK;
}

// one launch over device pointers.  An iiwarm context reads no frozen input and no boost; without nstep dz is not read.
template <class T>
hipError_t enqueue_fall(kidmp_ctx *ctx, int64_t ncol, int nz, const FallCall<T> &a, hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    const T *const *q = a.in;
    FallArgs<T> args{q[0], q[1], q[2], q[3], q[4], warm ? nullptr : q[5], warm ? nullptr : q[6], warm ? nullptr : q[7], warm ? nullptr : q[8],
                     warm ? nullptr : q[9], a.nstep ? a.dz : nullptr, a.nstep ? a.dz_col_stride : 0, a.dt, {}, a.nstep, warm ? 1 : 0};
    for (int v = 0; v < FALL_NOUT; ++v) args.out[v] = a.out[v];
    return launch_fall_speeds<T>(ctx->d_consts, ncol, nz, args, s);
}

template <class T>
int fall_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const FallCall<T> &a, void *stream)
{
    if (int rc = check_fall<T>(ctx, who, ncol, nz, a)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0;
    for (int v = 0; v < NIN; ++v)
        if (!(warm && v >= 5))
            if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    if (a.nstep) {
        if (int rc = check_device_array(ctx, who, a.dz, "dz")) return rc;
        if (int rc = check_device_array(ctx, who, a.nstep, "nstep")) return rc;
    }
    for (int v = 0; v < FALL_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], OUT_NAMES[v])) return rc;
    HIPTRY(ctx, enqueue_fall<T>(ctx, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip.  Only what the kernel reads goes up (dz with nstep alone) and only what was
// asked for comes down.
template <class T>
int fall_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const FallCall<T> &h)
{
    if (int rc = check_fall<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0;
    constexpr int A_DZ = NIN, A_OUT = NIN + 1, A_NSTEP = A_OUT + FALL_NOUT;
    StageArray a[A_NSTEP + 1];
    for (int v = 0; v < NIN; ++v) a[v] = stage_array(warm && v >= 5 ? nullptr : h.in[v], nz, STAGE_UP);
    a[A_DZ] = stage_rows(h.nstep ? h.dz : nullptr, nz, h.dz_col_stride);
    for (int v = 0; v < FALL_NOUT; ++v) a[A_OUT + v] = stage_array(h.out[v], nz, STAGE_DOWN);
    a[A_NSTEP] = stage_array(h.nstep, 4, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    FallCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[v]);
    d.dz = staged<T>(a[A_DZ]);
    d.dz_col_stride = h.dz_col_stride ? nz : 0;           // staged rows are packed
    d.dt = h.dt;
    for (int v = 0; v < FALL_NOUT; ++v) d.out[v] = staged<T>(a[A_OUT + v]);
    d.nstep = staged<int32_t>(a[A_NSTEP]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_fall<T>(ctx, n, nz, d, ctx->stream); });
}
}  // namespace

extern "C" {
int kidmp_fall_speeds_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                             const double *qr, const double *nr, const double *qi, const double *ni, const double *qs,
                             const double *qg, const double *vts_boost, const double *dz, int64_t dz_col_stride, double dt,
                             const kidmp_fall_out *out, int32_t *nstep, void *stream)
{
    return fall_device<double>(ctx, "kidmp_fall_speeds_device", ncol, nz,
                               fall_call<double>(t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz, dz_col_stride, dt, out, nstep), stream);
}
int kidmp32_fall_speeds_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                               const float *qr, const float *nr, const float *qi, const float *ni, const float *qs,
                               const float *qg, const float *vts_boost, const float *dz, int64_t dz_col_stride, double dt,
                               const kidmp32_fall_out *out, int32_t *nstep, void *stream)
{
    return fall_device<float>(ctx, "kidmp32_fall_speeds_device", ncol, nz,
                              fall_call<float>(t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz, dz_col_stride, dt, out, nstep), stream);
}
int kidmp_fall_speeds_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                           const double *qr, const double *nr, const double *qi, const double *ni, const double *qs,
                           const double *qg, const double *vts_boost, const double *dz, int64_t dz_col_stride, double dt,
                           const kidmp_fall_out *out, int32_t *nstep)
{
    return fall_host<double>(ctx, "kidmp_fall_speeds_host", ncol, nz,
                             fall_call<double>(t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz, dz_col_stride, dt, out, nstep));
}
int kidmp32_fall_speeds_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                             const float *qr, const float *nr, const float *qi, const float *ni, const float *qs,
                             const float *qg, const float *vts_boost, const float *dz, int64_t dz_col_stride, double dt,
                             const kidmp32_fall_out *out, int32_t *nstep)
{
    return fall_host<float>(ctx, "kidmp32_fall_speeds_host", ncol, nz,
                            fall_call<float>(t, p, qv, qr, nr, qi, ni, qs, qg, vts_boost, dz, dz_col_stride, dt, out, nstep));
}
}  // extern "C"
