// kidmp_summary.hip -- the entries of include/kidmp_summary.h: the per-column summary (water paths, cloud optical depth,
// echo and cloud heights) of device arrays in one launch of k_column_summary (below), and of host
// arrays in chunks through the context's staging memory.
#include "kidmp_ctx.h"
#include "../../include/kidmp_summary.h"

#include <cmath>

#include "kidmp_column.h"

namespace kidmp {

// The per-column summary (include/kidmp_summary.h): SUMMARY_N doubles per column from one read of its profiles.  Null
// means: nc -- the context is not aerosol-aware; qi, qs and qg -- zero (iiwarm); set_nc_col -- the context's Nt_c.
// dz: element (col, k) = dz[col*dz_col_stride + k], dz_col_stride 0 = one profile for all columns.
constexpr int SUMMARY_N = 16;
template <class T> struct SummaryArgs {
    const T *t, *p, *qv, *qc, *nc, *qi, *qr, *nr, *qs, *qg, *dz;
    int64_t dz_col_stride;
    double dbz_echo, q_cloud, t_freeze;
    const double *set_nc_col;
};

// One wavefront per column: the 15 numbers of include/kidmp_summary.h from one read of the column, no profile written.
// dBZ and re_qc of every level are those of k_reflectivity and k_effective_radii (the same functions on the same
// operands) and stay in registers.  Every sum is a per-lane sum over the level groups in ascending order followed by
// wave_sum: an order fixed by nz alone.  Levels are chosen with ballots, heights are masked sums of dz.  Lanes 0-15
// store the column's 16 doubles as one 128-byte line.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_column_summary(ReflConsts c, RadConsts rc, SummaryArgs<T> a, int64_t ncol, int nz, double *__restrict__ summary)
{
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    const double Nt_c = a.set_nc_col ? a.set_nc_col[col] * 1.e6 : rc.Nt_c;
    const T *__restrict__ dzc = a.dz + col * a.dz_col_stride;

    double dbz[NJ], dz[NJ], sum[7] = {0., 0., 0., 0., 0., 0., 0.};   // WVP, CWP, RWP, IWP, SWP, GWP, TAU_C of the lane
    bool cloudy[NJ], frozen[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { dbz[j] = -double(__builtin_inf()); dz[j] = 0.; cloudy[j] = frozen[j] = false; }
    column_dbz<T, NJ>(c, nz, lane, base, a.t, a.p, a.qv, a.qr, a.nr, a.qs, a.qg, dbz,
                      [&](int j, int64_t i, double temp, double pres, double qv_in, double qv, double rho, double qs, bool,
                          const lvl::SnowLevel &) __attribute__((always_inline)) {
                          const double qc = double(a.qc[i]), qi = a.qi ? double(a.qi[i]) : 0.;
                          const double h = double(dzc[i - base]);
                          dz[j] = h;
                          const double cw = rho * qc * h;
                          sum[0] += rho * qv * h;
                          sum[1] += cw;
                          sum[2] += rho * double(a.qr[i]) * h;
                          sum[3] += rho * qi * h;
                          sum[4] += rho * qs * h;
                          sum[5] += rho * (a.qg ? double(a.qg[i]) : 0.) * h;
                          double re;                                 // calc_effectRad's own density: qv unclamped, M:4860
                          const double rho_r = qv_in == qv ? rho : lvl::air_density(pres, temp, qv_in);
                          if (lvl::cloud_water_radius(rc, Nt_c, rho_r, qc, a.nc ? double(a.nc[i]) : 0., re))
                              sum[6] += 1.5 * cw / (1000.0 * re);
                          cloudy[j] = qc + qi > a.q_cloud;
                          frozen[j] = temp < a.t_freeze;
                      });
#pragma unroll
    for (int s = 0; s < 7; ++s) sum[s] = wave_sum(sum[s]);

    const double nan = __builtin_nan("");
    double lmax = dbz[0];
#pragma unroll
    for (int j = 1; j < NJ; ++j) lmax = fmax(lmax, dbz[j]);
    const double dbz_max = wave_max(lmax);
    bool at_max[NJ], echo[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { at_max[j] = dbz[j] == dbz_max; echo[j] = dbz[j] >= a.dbz_echo; }   // false past nz: -inf
    int n_cloud, n_echo;
    const int k_max = lowest_level<NJ>(at_max), k_echo = highest_level<NJ>(echo, n_echo);
    const int k_base = lowest_level<NJ>(cloudy), k_top = highest_level<NJ>(cloudy, n_cloud), k_frz = lowest_level<NJ>(frozen);
    // k_max < 0 only for NaN input: the slot is then NaN, and no index is formed from it
    const double z_max = k_max < 0 ? nan : height_below<NJ>(dz, lane, k_max) + 0.5 * level_of<NJ>(dz, k_max);
    const double z_echo = k_echo < 0 ? nan : height_below<NJ>(dz, lane, k_echo + 1);
    const double z_base = k_base < 0 ? nan : height_below<NJ>(dz, lane, k_base);
    const double z_top = k_top < 0 ? nan : height_below<NJ>(dz, lane, k_top + 1);
    const double z_frz = k_frz < 0 ? nan : height_below<NJ>(dz, lane, k_frz) + 0.5 * level_of<NJ>(dz, k_frz);
    const double dbz_sfc = readlane(dbz[0], 0);

    const double slot[SUMMARY_N] = {sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], dbz_max, z_max, z_echo, dbz_sfc,
                                    z_base, z_top, double(n_cloud), z_frz, 0.};
    double out = slot[0];
#pragma unroll
    for (int s = 1; s < SUMMARY_N; ++s) out = lane == s ? slot[s] : out;
    if (lane < SUMMARY_N) summary[col * SUMMARY_N + lane] = out;
}

namespace {
template <class T>
hipError_t launch_column_summary(const ReflConsts &c, const RadConsts &rc, int64_t ncol, int nz, const SummaryArgs<T> &a, double *summary, hipStream_t s)
{
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_column_summary<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, rc, a, ncol, nz, summary);
    });
}
}  // namespace

}  // namespace kidmp

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
