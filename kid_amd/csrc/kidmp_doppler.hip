// kidmp_doppler.hip -- the entries of include/kidmp_doppler.h: reflectivity, mean Doppler velocity and spectrum width of
// device arrays in one launch of k_doppler_moments (below), and of host arrays in chunks through the
// context's staging memory.
#include "kidmp_ctx.h"
#include "../../include/kidmp_doppler.h"

#include "kidmp_column.h"

namespace kidmp {

// The Doppler moments of a vertically pointing radar (include/kidmp_doppler.h): reflectivity, mean Doppler velocity and
// spectrum width of every level, from calc_refl10cm's load and size distributions.  Null means: qs, qg -- zero; w -- zero;
// an output -- not wanted.  out: dbz, vd, sw, vz_r, vz_s, vz_g, dbz_r, dbz_s, dbz_g.
constexpr int DOPPLER_NOUT = 9;
template <class T> struct DopplerArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg, *w;
    T *out[DOPPLER_NOUT];
};

// One wavefront per column: the three radar moments of every level (include/kidmp_doppler.h).  The load, the ze_* and the
// order of their sum are column_dbz's, through the same lvl:: functions; beside them the reflectivity-weighted first and
// second moments of each species' fall speed.  Rain and snow are finished before the graupel scan and leave only their
// sums behind; graupel follows the running minimum of its intercept.  Nothing but the fastmath tables is in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_doppler_moments(ReflConsts c, DopplerConsts dc, DopplerArgs<T> a, int64_t ncol, int nz)
{
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);

    // of rain and snow together: ze with the 1.E-22 of an absent species (dbz), ze of the present ones, ze*vz, ze*v2
    double ze_rs[NJ], wt[NJ], m1[NJ], m2[NJ], rhof[NJ], rg[NJ], n0[NJ];
    bool lqg[NJ], any[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        ze_rs[j] = wt[j] = m1[j] = m2[j] = rhof[j] = 0.;
        rg[j] = R1;
        lqg[j] = any[j] = false;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k >= nz) continue;
        const int64_t i = base + k;
        const RadarLevel r = radar_level(c, a, i);                   // ---- load, M:4991-5028 ----
        const bool L_qr = r.L_qr, L_qs = r.L_qs;
        const double ze_rain = r.ze_rain, ze_snow = r.ze_snow;
        lqg[j] = r.L_qg;
        any[j] = L_qr || L_qs || lqg[j];
        rhof[j] = r.rhof;
        rg[j] = r.rg;
        double vz_r = 0., v2_r = 0., vz_s = 0., v2_s = 0.;
        if (L_qr) lvl::rain_doppler(dc, rhof[j], r.lamr, vz_r, v2_r);
        if (L_qs) lvl::snow_doppler(c, dc, rhof[j], r.sl, vz_s, v2_s);
        ze_rs[j] = ze_rain + ze_snow;
        wt[j] = (L_qr ? ze_rain : 0.) + (L_qs ? ze_snow : 0.);
        m1[j] = ze_rain * vz_r + ze_snow * vz_s;                     // an absent species has vz = v2 = +0.0
        m2[j] = ze_rain * v2_r + ze_snow * v2_s;
        n0[j] = r.n0_exp;
        if (a.out[3]) a.out[3][i] = T(vz_r);
        if (a.out[4]) a.out[4][i] = T(vz_s);
        if (a.out[6]) a.out[6][i] = T(lvl::dbz_of(ze_rain));
        if (a.out[7]) a.out[7][i] = T(lvl::dbz_of(ze_snow));
    }

    graupel_running_min<NJ>(n0, lane);

#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        if (k >= nz) continue;
        const int64_t i = base + k;
        double ze_graupel = 1.E-22, vz_g = 0., v2_g = 0.;
        if (lqg[j]) {
            double ilamg;
            ze_graupel = lvl::graupel_ze(c, n0[j], rg[j], ilamg);
            lvl::graupel_doppler(dc, rhof[j], ilamg, vz_g, v2_g);
        }
        if (a.out[0]) a.out[0][i] = T(lvl::dbz_of(ze_rs[j] + ze_graupel));          // M:5196
        if (a.out[5]) a.out[5][i] = T(vz_g);
        if (a.out[8]) a.out[8][i] = T(lvl::dbz_of(ze_graupel));
        double vd = 0., sw = 0.;                                     // a level with no species: +0.0, w is not applied
        if (any[j]) {
            const double W = wt[j] + (lqg[j] ? ze_graupel : 0.);
            const double V = (m1[j] + ze_graupel * vz_g) / W;
            const double var = (m2[j] + ze_graupel * v2_g) / W - V * V;
            vd = V - (a.w ? double(a.w[i]) : 0.);
            sw = var > 0. ? fm::sqrt_pos(var) : 0.;
        }
        if (a.out[1]) a.out[1][i] = T(vd);
        if (a.out[2]) a.out[2][i] = T(sw);
    }
}

namespace {
template <class T>
hipError_t launch_doppler_moments(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const DopplerArgs<T> &a, hipStream_t s)
{
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_doppler_moments<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, dc, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

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
