// kidmp_fall.hip -- the entries of include/kidmp_fall.h: block-O fall speeds, sedimentation fluxes and CFL substep counts
// of device arrays in one launch of k_fall_speeds (below), and of host arrays in chunks through the
// context's staging memory.
#include "kidmp_ctx.h"
#include "../../include/kidmp_fall.h"

#include "kidmp_column.h"

namespace kidmp {

// The fall speeds of block O (M:3206-3354) as a diagnostic of a state (include/kidmp_fall.h).  Null means: qi, ni, qs, qg
// -- not read (warm); boost -- 1.0 where T < T_0, 1.5 elsewhere; an output -- not wanted; nstep -- not wanted, and then
// dz and dt are not read.  out: vt_r, vt_nr, vt_i, vt_ni, vt_s, vt_g, flux_r, flux_i, flux_s, flux_g, flux_total.
constexpr int FALL_NOUT = 11;
template <class T> struct FallArgs {
    const T *t, *p, *qv, *qr, *nr, *qi, *ni, *qs, *qg, *boost, *dz;
    int64_t dz_col_stride;
    double dt;
    T *out[FALL_NOUT];
    int32_t *nstep;                                  // [ncol][4]: rain, ice, snow, graupel
    int warm;                                        // iiwarm: the frozen speeds and fluxes are +0.0 (M:3346-3352)
};

namespace {

// ---- the fall speeds (include/kidmp_fall.h) ----
__device__ inline int wave_max_int(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}
template <int D>
__device__ inline int row_shl_int(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x100 + D, 0xf, 0xf, false); }

// One step of the inheritance scan: a lane whose level lacks the species takes what lane l + D of its row holds.
template <int D, bool TWO>
__device__ inline void carry_step(double &a, double &b, int &h, int r)
{
    const double oa = row_shl<D>(a), ob = TWO ? row_shl<D>(b) : 0.;
    const int oh = row_shl_int<D>(h);
    const bool take = r + D < 16 && !h;
    a = take ? oa : a;
    if (TWO) b = take ? ob : b;
    h = take ? oh : h;
}
// vtrk(k) = vtrk(k+1) where the level lacks the species (M:3235, 3267, 3307, 3333) over the 64 levels of a wave: a suffix
// scan with the associative operator "keep mine if my level has the species, else take the one above".  Only moves: a
// lane ends with the bits of the nearest lane at or above it whose `has` is set, and the return value tells whether
// there is one.  (ta, tb, th): lane 0's result, wave-uniform -- what the whole wave hands down to the levels below it.
// One predicate carries both values (TWO: the mass- and the number-weighted speed).  Whole wavefronts only.
template <bool TWO>
__device__ inline bool wave_carry_down(double &a, double &b, bool has, int lane, double &ta, double &tb, bool &th)
{
    int h = has;
    const int r = lane & 15;
    carry_step<1, TWO>(a, b, h, r);
    carry_step<2, TWO>(a, b, h, r);
    carry_step<4, TWO>(a, b, h, r);
    carry_step<8, TWO>(a, b, h, r);
    // lane 16 q holds what row q hands down
    const double a1 = readlane(a, 16), a2 = readlane(a, 32), a3 = readlane(a, 48);
    const double b1 = TWO ? readlane(b, 16) : 0., b2 = TWO ? readlane(b, 32) : 0., b3 = TWO ? readlane(b, 48) : 0.;
    const int h1 = __builtin_amdgcn_readlane(h, 16), h2 = __builtin_amdgcn_readlane(h, 32), h3 = __builtin_amdgcn_readlane(h, 48);
    const double u2a = a3, u1a = h2 ? a2 : a3, u0a = h1 ? a1 : u1a;     // what the rows above row q hand down
    const double u2b = b3, u1b = h2 ? b2 : b3, u0b = h1 ? b1 : u1b;
    const int u2h = h3, u1h = h2 | h3, u0h = h1 | u1h;
    const int q = lane >> 4;
    const int uh = q == 0 ? u0h : q == 1 ? u1h : q == 2 ? u2h : 0;
    if (!h && uh) {
        a = q == 0 ? u0a : q == 1 ? u1a : u2a;
        if (TWO) b = q == 0 ? u0b : q == 1 ? u1b : u2b;
        h = 1;
    }
    ta = readlane(a, 0);
    tb = TWO ? readlane(b, 0) : 0.;
    th = __builtin_amdgcn_readlane(h, 0) != 0;
    return h != 0;
}
// the column: the level groups chained from the top, the value above the top level is 0 (M:3209-3216)
template <int NJ, bool TWO>
__device__ inline void carry_down_column(double (&a)[NJ], double (&b)[NJ], const bool (&has)[NJ], int lane)
{
    double ca = 0., cb = 0.;
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {
        double ta, tb;
        bool th;
        const bool h = wave_carry_down<TWO>(a[j], b[j], has[j], lane, ta, tb, th);
        if (!h) { a[j] = ca; if (TWO) b[j] = cb; }
        if (th) { ca = ta; cb = tb; }
    }
}
// nstep of one species: MAX over the levels with v > 1.E-3 of INT(DT/delta_tp + 1.) (M:3239-3243); 0 is reported as 1,
// as NINT(1./onstep) gives it (M:3365)
template <int NJ>
__device__ inline int column_substeps(const double (&v)[NJ], const double (&dz)[NJ], double dt, int nz, int lane)
{
    int ns = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (64 * j + lane < nz && v[j] > 1.E-3) ns = max(ns, lvl::fall_substeps(dt, dz[j], v[j]));
    ns = wave_max_int(ns);
    return ns > 0 ? ns : 1;
}

}  // namespace

// One wavefront per column: block O (M:3206-3354) of the state as mp_thompson loads it -- the fall speeds of rain, ice,
// snow and graupel at every level, the sedimentation fluxes v * rho q and, on request, the CFL substep counts
// (include/kidmp_fall.h).  Species by species: the level's own speed, the inheritance scan, the stores; rain first,
// because snow and graupel read the inherited rain speed.  Nothing but the fastmath tables is in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_fall_speeds(const Consts *__restrict__ hc, FallArgs<T> a, int64_t ncol, int nz)
{
    const FallConsts c = fall_consts(*hc);
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    const bool count = a.nstep != nullptr;

    double temp[NJ], rho[NJ], rhof[NJ], mvd[NJ], dz[NJ], vtr[NJ], ftot[NJ];
    double va[NJ], vb[NJ], rq[NJ], fx[NJ];                           // the species at hand: its two speeds, its content rho*q, its flux
    bool has[NJ];
    int ns_r = 1, ns_i = 1, ns_s = 1, ns_g = 1;

    // ---- load (M:1387-1391, M:1447-1474) and rain (M:3221-3237) ----
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        temp[j] = 0.; rho[j] = 1.; rhof[j] = 0.; mvd[j] = 0.; dz[j] = 1.; va[j] = vb[j] = 0.; rq[j] = R1; has[j] = false;
        if (k >= nz) continue;
        const int64_t i = base + k;
        temp[j] = double(a.t[i]);
        rho[j] = lvl::air_density(double(a.p[i]), temp[j], fmax(1.E-10, double(a.qv[i])));
        rhof[j] = fm::sqrt_pos(rho_not / rho[j]);                    // M:3219
        if (count) dz[j] = double(a.dz[col * a.dz_col_stride + k]);
        const lvl::RainLoad r = lvl::rain_load(c, rho[j], double(a.qr[i]), double(a.nr[i]));
        has[j] = r.rr > R1;                                          // block O asks the content, M:3221
        rq[j] = r.rr;
        if (r.has) mvd[j] = r.mvd;                                   // 0: no rain (block E asks L_qr, M:1639)
        if (has[j]) lvl::rain_fall_speeds(c, rhof[j], r.lamr, va[j], vb[j]);
    }
    carry_down_column<NJ, true>(va, vb, has, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) { vtr[j] = va[j]; fx[j] = va[j] * rq[j]; ftot[j] = fx[j]; }      // sed_r, M:3368
    store_profile<T, NJ>(a.out[0], base, nz, lane, va);
    store_profile<T, NJ>(a.out[1], base, nz, lane, vb);
    store_profile<T, NJ>(a.out[6], base, nz, lane, fx);
    if (count) {
        double vm[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) vm[j] = fmax(va[j], vb[j]);     // M:3239
        ns_r = column_substeps<NJ>(vm, dz, a.dt, nz, lane);
    }

    if (a.warm) {                                                    // M:3346-3352: exact zeros
#pragma unroll
        for (int j = 0; j < NJ; ++j) va[j] = 0.;
#pragma unroll
        for (int o = 2; o < 10; ++o)
            if (o != 6) store_profile<T, NJ>(a.out[o], base, nz, lane, va);
    } else {
        // ---- cloud ice, M:1420-1445 and M:3253-3269 ----
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            va[j] = vb[j] = 0.; rq[j] = R1; has[j] = false;
            if (k >= nz) continue;
            const lvl::IceLoad r = lvl::ice_load(c, rho[j], double(a.qi[base + k]), double(a.ni[base + k]));
            has[j] = r.ri > R1;                                      // M:3256
            rq[j] = r.ri;
            if (has[j]) lvl::ice_fall_speeds(c, rhof[j], r.lami, va[j], vb[j]);
        }
        carry_down_column<NJ, true>(va, vb, has, lane);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { fx[j] = va[j] * rq[j]; ftot[j] = ftot[j] + fx[j]; }
        store_profile<T, NJ>(a.out[2], base, nz, lane, va);
        store_profile<T, NJ>(a.out[3], base, nz, lane, vb);
        store_profile<T, NJ>(a.out[7], base, nz, lane, fx);
        if (count) ns_i = column_substeps<NJ>(va, dz, a.dt, nz, lane);

        // ---- snow, M:1475-1483, block D and M:3285-3308 ----
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            va[j] = 0.; rq[j] = R1; has[j] = false;
            if (k >= nz) continue;
            const double qs = double(a.qs[base + k]);
            if (qs > R1) rq[j] = qs * rho[j];                        // M:1475-1483
            has[j] = rq[j] > R1;                                     // M:3288
            if (!has[j]) continue;
            const double boost = a.boost ? double(a.boost[base + k]) : temp[j] < T_0 ? 1.0 : 1.5;   // M:2027, M:1751
            const double vts = lvl::snow_fall_speed(c, rhof[j], lvl::snow_level(temp[j], rq[j], c.oams));
            va[j] = lvl::snow_boosted(vts, boost, temp[j], vtr[j]);
        }
        carry_down_column<NJ, false>(va, vb, has, lane);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { fx[j] = va[j] * rq[j]; ftot[j] = ftot[j] + fx[j]; }
        store_profile<T, NJ>(a.out[4], base, nz, lane, va);
        store_profile<T, NJ>(a.out[8], base, nz, lane, fx);
        if (count) ns_s = column_substeps<NJ>(va, dz, a.dt, nz, lane);

        // ---- graupel, M:1484-1492, block E (M:1633-1654) and M:3322-3334 ----
        double n0[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            va[j] = 0.; rq[j] = R1; has[j] = false;
            if (k >= nz) continue;
            const double qg = double(a.qg[base + k]);
            if (qg > R1) rq[j] = qg * rho[j];                        // M:1484-1492
            has[j] = rq[j] > R1;                                     // M:3325
        }
        graupel_intercepts<NJ>(temp, mvd, rq, nz, lane, n0);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (has[j]) va[j] = lvl::graupel_fall_speed(c, rhof[j], n0[j], rq[j], temp[j], vtr[j]);
        carry_down_column<NJ, false>(va, vb, has, lane);
#pragma unroll
        for (int j = 0; j < NJ; ++j) { fx[j] = va[j] * rq[j]; ftot[j] = ftot[j] + fx[j]; }
        store_profile<T, NJ>(a.out[5], base, nz, lane, va);
        store_profile<T, NJ>(a.out[9], base, nz, lane, fx);
        if (count) ns_g = column_substeps<NJ>(va, dz, a.dt, nz, lane);
    }
    store_profile<T, NJ>(a.out[10], base, nz, lane, ftot);
    if (count && lane < 4) a.nstep[col * 4 + lane] = lane == 0 ? ns_r : lane == 1 ? ns_i : lane == 2 ? ns_s : ns_g;
}

namespace {
// d_consts: the context's Consts in device memory (kidmp_ctx::d_consts)
template <class T>
hipError_t launch_fall_speeds(const Consts *c, int64_t ncol, int nz, const FallArgs<T> &a, hipStream_t s)
{
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_fall_speeds<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

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
