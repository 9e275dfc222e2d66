// kidmp_summary.hip -- the entries of include/kidmp_summary.h: the per-column summary (water paths, cloud optical depth,
// echo and cloud heights) of device arrays in one launch of k_column_summary (thompson_reflectivity.hip), and of host
// arrays in chunks through the context's staging memory.
#include "kidmp_ctx.h"
#include "../../include/kidmp_summary.h"

#include <cmath>

using namespace kidmp;

static_assert(SUMMARY_N == KIDMP_SUMMARY_N, "include/kidmp_summary.h");

namespace {
constexpr int NPROF = 10;                                 // t, p, qv, qc, nc, qi, qr, nr, qs, qg
const char *const PROF_NAMES[NPROF] = {"t", "p", "qv", "qc", "nc", "qi", "qr", "nr", "qs", "qg"};

template <class T> struct SummaryCall {
    const T *prof[NPROF];
    const T *dz;
    int64_t dz_col_stride;
    double *summary;
};

// what the device and the host entries check alike, before anything is touched; thr receives the thresholds
template <class T>
int check_summary(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const SummaryCall<T> &a, const kidmp_summary_cfg *cfg,
                  kidmp_summary_cfg &thr)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (int rc = check_nc_count(ctx, who, ncol)) return rc;
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (a.dz_col_stride != 0 && a.dz_col_stride < nz) return fail(ctx, KIDMP_EINVAL, w + ": dz_col_stride must be 0 or >= nz");
    thr = cfg ? *cfg : kidmp_summary_cfg{18.0, 1.0e-5, 273.15};
    if (!std::isfinite(thr.dbz_echo) || !std::isfinite(thr.q_cloud) || !std::isfinite(thr.t_freeze))
        return fail(ctx, KIDMP_EINVAL, w + ": a threshold is not finite");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    const bool warm = ctx->cfg.iiwarm != 0;
    for (int v = 0; v < NPROF; ++v) {
        const bool optional = v == 4 || v == 5 || v == 8 || v == 9;
        if (!a.prof[v] && !optional) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    }
    if (!a.dz || !a.summary) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if ((a.prof[8] == nullptr) != (a.prof[9] == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": qs and qg must be given or left out together");
    if (!warm && (!a.prof[5] || !a.prof[8])) return fail(ctx, KIDMP_EINVAL, w + ": a mixed-phase context needs qi, qs and qg");
    if (ctx->cfg.is_aerosol_aware && !a.prof[4]) return fail(ctx, KIDMP_EINVAL, w + ": an aerosol-aware context needs nc");
    if (!refl_consts_supported(ctx->hc)) return fail(ctx, KIDMP_ESTATE, w + ": reflectivity exponents differ from the kernel's");
    return KIDMP_OK;
}

// one launch over device pointers; nc_first: the batch's first column within a bound per-column droplet number
template <class T>
hipError_t enqueue_summary(kidmp_ctx *ctx, int64_t ncol, int nz, const SummaryCall<T> &a, const kidmp_summary_cfg &thr, hipStream_t s,
                           int64_t nc_first)
{
    const bool aero = ctx->cfg.is_aerosol_aware != 0;
    const T *const *q = a.prof;
    const SummaryArgs<T> args{q[0], q[1], q[2], q[3], aero ? q[4] : nullptr, q[5], q[6], q[7], q[8], q[9], a.dz, a.dz_col_stride,
                              thr.dbz_echo, thr.q_cloud, thr.t_freeze, ctx->d_nc_col ? ctx->d_nc_col + nc_first : nullptr};
    return launch_column_summary<T>(refl_consts(ctx->hc), rad_consts(ctx->hc, aero), ncol, nz, args, a.summary, s);
}

template <class T>
int summary_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const SummaryCall<T> &a, const kidmp_summary_cfg *cfg,
                   void *stream)
{
    kidmp_summary_cfg thr;
    if (int rc = check_summary<T>(ctx, who, ncol, nz, a, cfg, thr)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NPROF; ++v)
        if (int rc = check_device_array(ctx, who, a.prof[v], PROF_NAMES[v])) return rc;
    if (int rc = check_device_array(ctx, who, a.dz, "dz")) return rc;
    if (int rc = check_device_array(ctx, who, a.summary, "summary")) return rc;
    HIPTRY(ctx, enqueue_summary<T>(ctx, ncol, nz, a, thr, (hipStream_t)stream, 0));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip; every profile keeps its slot
template <class T>
int summary_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const SummaryCall<T> &h, const kidmp_summary_cfg *cfg)
{
    kidmp_summary_cfg thr;
    if (int rc = check_summary<T>(ctx, who, ncol, nz, h, cfg, thr)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    constexpr int A_DZ = NPROF, A_SUM = NPROF + 1;
    StageArray a[A_SUM + 1];
    for (int v = 0; v < NPROF; ++v) a[v] = stage_keep(stage_array(h.prof[v], nz, STAGE_UP));
    a[A_DZ] = stage_rows(h.dz, nz, h.dz_col_stride);
    a[A_SUM] = stage_array(h.summary, KIDMP_SUMMARY_N, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    SummaryCall<T> d{};
    for (int v = 0; v < NPROF; ++v) d.prof[v] = staged<T>(a[v]);
    d.dz = staged<T>(a[A_DZ]);
    d.dz_col_stride = h.dz_col_stride ? nz : 0;           // staged rows are packed
    d.summary = staged<double>(a[A_SUM]);
    return stage_run(ctx, plan, [&](int64_t c0, int64_t n) { return enqueue_summary<T>(ctx, n, nz, d, thr, ctx->stream, c0); });
}
}  // namespace

extern "C" {
int kidmp_column_summary_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                const double *qc, const double *nc, const double *qi, const double *qr, const double *nr,
                                const double *qs, const double *qg, const double *dz, int64_t dz_col_stride,
                                const kidmp_summary_cfg *cfg, double *summary, void *stream)
{
    return summary_device<double>(ctx, "kidmp_column_summary_device", ncol, nz, {{t, p, qv, qc, nc, qi, qr, nr, qs, qg}, dz, dz_col_stride, summary},
                                  cfg, stream);
}
int kidmp32_column_summary_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                  const float *qc, const float *nc, const float *qi, const float *qr, const float *nr,
                                  const float *qs, const float *qg, const float *dz, int64_t dz_col_stride,
                                  const kidmp_summary_cfg *cfg, double *summary, void *stream)
{
    return summary_device<float>(ctx, "kidmp32_column_summary_device", ncol, nz, {{t, p, qv, qc, nc, qi, qr, nr, qs, qg}, dz, dz_col_stride, summary},
                                 cfg, stream);
}
int kidmp_column_summary_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                              const double *qc, const double *nc, const double *qi, const double *qr, const double *nr,
                              const double *qs, const double *qg, const double *dz, int64_t dz_col_stride,
                              const kidmp_summary_cfg *cfg, double *summary)
{
    return summary_host<double>(ctx, "kidmp_column_summary_host", ncol, nz, {{t, p, qv, qc, nc, qi, qr, nr, qs, qg}, dz, dz_col_stride, summary}, cfg);
}
int kidmp32_column_summary_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                const float *qc, const float *nc, const float *qi, const float *qr, const float *nr,
                                const float *qs, const float *qg, const float *dz, int64_t dz_col_stride,
                                const kidmp_summary_cfg *cfg, double *summary)
{
    return summary_host<float>(ctx, "kidmp32_column_summary_host", ncol, nz, {{t, p, qv, qc, nc, qi, qr, nr, qs, qg}, dz, dz_col_stride, summary}, cfg);
}
}  // extern "C"
