// kidmp_kinematic.hip -- the entries of include/kidmp_kinematic.h: prescribed-w vertical advection of KiD's nine fields in
// the adv / div form the adapter consumes (k_kid_advect) and the state update that closes the time loop (k_kid_update).
// The schemes (van Leer; ULTIMATE QUICKEST, section 4.6g, include/kidmp_advection.h, whose two
// entries are at the end) are fixed to the operation.  Built with the library's plain flags (IEEE division, no
// contraction): every operation below rounds once.
#include "kidmp_ctx.h"
#include "kidmp_face.h"
#include "kidmp_stream.h"
#include "kidmp_wave.h"
#include "../../include/kidmp_kinematic.h"

using namespace kidmp;
using namespace kidmp::streaming;
using namespace kidmp::wave;

namespace {
constexpr int ADV_WAVES = 4;                             // columns (wavefronts) per workgroup
constexpr int ADV_THREADS = 64 * ADV_WAVES;
const char *const FIELD_NAMES[KID_NF] = {"theta", "qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg"};

template <class T, int N> struct AdvectArgs {            // N members: KiD's nine fields, or the three aerosols
    const T *state[N];
    T *adv[N], *div[N], *sum[N];                         // null: not wanted
    const T *w, *rho, *dz;
    int64_t w_col_stride;
    T *courant;
    double dt;
};
template <class T, int N> struct UpdateArgs {
    T *state[N];                                         // null: skipped
    const T *t[3][N];                                    // null: a zero operand
    int64_t n;
    T dt;
    uint32_t clip;                                       // bit m: member m is clipped (never theta)
};

// One wavefront per column, level k = 64 j + lane.  Cell k owns its lower face k: the mass flux M and the Courant number c
// of that face are formed once per column and kept in registers with what every member shares (den, the divergence
// factor, the upwind side); then each present member is loaded once, its neighbours k-1, k-2 and k+1 come from the
// neighbouring lanes, its face value and flux are formed once per lane and the flux of face k+1 comes from the lane
// above.  The lane that holds level nz-1 forms the top face itself.  No LDS, no scratch.  S: the scheme of the interior
// faces' value (kidmp_face.h), whose per-face coefficients g and rc join hc in the per-column registers.
template <class T, int NJ, int N, int S>
__global__ void __launch_bounds__(ADV_THREADS)
k_kid_advect(const AdvectArgs<T, N> a, int64_t ncol, int nz)
{
    const int lane = int(threadIdx.x) & 63;
    const int64_t col = int64_t(blockIdx.x) * ADV_WAVES + (int(threadIdx.x) >> 6);
    if (col >= ncol) return;                                         // whole wavefronts only: the shifts need every lane
    const int64_t base = col * int64_t(nz);
    const T *const w = a.w + col * a.w_col_stride;

    constexpr int NG = face::coef_count<S>(NJ);
    double M[NJ], Mup[NJ], den[NJ], hc[NJ], dM[NJ];                  // hc = 0.5*(1.0 - c) of face k
    double g[NG], rc[NG];                                            // ULTIMATE: (1.0 - c*c)/6.0 and 1.0/c of face k
    bool up[NJ], second[NJ];                                         // w[k] >= 0; uu of face k inside the column
    double cmax = 0.;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        M[j] = Mup[j] = hc[j] = g[j % NG] = rc[j % NG] = 0.;
        den[j] = 1.;
        up[j] = true;
        second[j] = false;
        if (k >= nz) continue;
        const double rho = double(a.rho[k]), dz = double(a.dz[k]), wk = double(w[k]);
        const double rho_lo = k ? double(a.rho[k - 1]) : rho, dz_lo = k ? double(a.dz[k - 1]) : dz;
        const double rf = k ? 0.5 * (rho_lo + rho) : rho;
        up[j] = wk >= 0.;
        second[j] = up[j] ? k >= 2 : k + 1 < nz;
        M[j] = rf * wk;
        const double c = (fabs(wk) * a.dt) / (up[j] ? dz_lo : dz);
        face::coef<S>(c, hc[j], g[j % NG], rc[j % NG]);
        den[j] = rho * dz;
        cmax = fmax(cmax, c);
        if (k == nz - 1) {                                           // the model top: rf = rho[nz-1], dz[nz-1]
            const double wt = double(w[nz]);
            Mup[j] = rho * wt;
            cmax = fmax(cmax, (fabs(wt) * a.dt) / dz);
        }
    }
    {
        double above[NJ];
        level_above<NJ>(M, above);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (64 * j + lane != nz - 1) Mup[j] = above[j];
            dM[j] = (Mup[j] - M[j]) / den[j];
        }
    }
    if (a.courant) {
        cmax = wave_max(cmax);
        if (lane == 0) a.courant[col] = T(cmax);
    }

#pragma unroll
    for (int m = 0; m < N; ++m) {
        if (!a.state[m] || !(a.adv[m] || a.div[m] || a.sum[m])) continue;
        double q[NJ], q1[NJ], q2[NJ], qa[NJ], F[NJ], Fup[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            q[j] = k < nz ? double(a.state[m][base + k]) : 0.;
        }
        level_below<NJ>(q, q1);                                      // q[k-1]
        level_below<NJ>(q1, q2);                                     // q[k-2]
        level_above<NJ>(q, qa);                                      // q[k+1]
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            const double qu = up[j] ? q1[j] : q[j], qd = up[j] ? q[j] : q1[j], quu = up[j] ? q2[j] : qa[j];
            // formed before the select, not in its arm: there the division would make the select a branch
            const double qi = face::value<S>(hc[j], g[j % NG], rc[j % NG], second[j], qu, qd, quu);
            const double qf = k ? qi : q[j];                         // qf[0] = q[0]
            F[j] = M[j] * qf;
        }
        level_above<NJ>(F, Fup);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            if (k >= nz) continue;
            if (k == nz - 1) Fup[j] = Mup[j] * q[j];                 // qf[nz] = q[nz-1]
            const double adv = -((Fup[j] - F[j]) / den[j]);
            const double div = q[j] * dM[j];
            if (a.adv[m]) a.adv[m][base + k] = T(adv);
            if (a.div[m]) a.div[m][base + k] = T(div);
            if (a.sum[m]) a.sum[m][base + k] = T(adv + div);
        }
    }
}

// X = X + ((t1 + t2) + t3)*dt in T, then the clip of everything but theta: one element (V of them) per lane-slot
template <class T, int V, int NF, int N>
__global__ __launch_bounds__(256) void k_kid_update(const UpdateArgs<T, N> a)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, nvec = a.n / V;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const int64_t e = i * V;
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            if (!a.state[m]) continue;
            Vec<T, V> x = ld<T, V>(a.state[m], e);
            const Vec<T, V> t1 = ld<T, V>(a.t[0][m], e), t2 = ld<T, V>(a.t[1][m], e), t3 = ld<T, V>(a.t[2][m], e);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                x.v[j] = x.v[j] + ((t1.v[j] + t2.v[j]) + t3.v[j]) * a.dt;
                if (a.clip >> m & 1u) x.v[j] = x.v[j] < T(0) ? T(0) : x.v[j];
            }
            st<T, V>(a.state[m], e, x);
        }
    }
}

template <class T, int N, int S>
void launch_advect(dim3 grid, dim3 block, hipStream_t st, const AdvectArgs<T, N> &a, int64_t ncol, int nz)
{
    switch ((nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_kid_advect<T, 1, N, S>), grid, block, 0, st, a, ncol, nz); break;
    case 2: hipLaunchKernelGGL((k_kid_advect<T, 2, N, S>), grid, block, 0, st, a, ncol, nz); break;
    case 3: hipLaunchKernelGGL((k_kid_advect<T, 3, N, S>), grid, block, 0, st, a, ncol, nz); break;
    default: hipLaunchKernelGGL((k_kid_advect<T, 4, N, S>), grid, block, 0, st, a, ncol, nz); break;
    }
}

template <class T, class F> void members(const F *f, T *(&out)[KID_NF], int nf)
{
    for (int m = 0; m < KID_NF; ++m) out[m] = nullptr;
    if (!f) return;
    T *const p[KID_NF] = {f->theta, f->qv, f->qc, f->qr, f->nr, f->qi, f->ni, f->qs, f->qg};
    for (int m = 0; m < nf; ++m) out[m] = p[m];
}

// what both entries refuse alike, before anything is touched; KIDMP_OK with ncol == 0 means: nothing to do
int check_shape(kidmp_ctx *ctx, const std::string &w, int64_t ncol, int32_t nz, double dt)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (!(dt > 0.)) return fail(ctx, KIDMP_EINVAL, w + ": dt must be > 0");
    if (ncol > int64_t(0x7fffffff)) return fail(ctx, KIDMP_EINVAL, w + ": more columns than one launch takes");
    return KIDMP_OK;
}

template <class T, class F>
int advect_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, double dt, const F *state, const T *w, int64_t w_col_stride,
                  const T *rho, const T *dz, const F *adv, const F *div, const F *sum, T *courant, void *stream)
{
    const int nf = ctx && ctx->cfg.iiwarm ? KID_NWARM : KID_NF;      // the frozen members are not looked at in a warm context
    KidMembers<T, KID_NF> f{};
    members<T>(state, f.state, nf);
    members<T>(adv, f.adv, nf);
    members<T>(div, f.div, nf);
    members<T>(sum, f.sum, nf);
    return kid_advect_members<T, KID_NF>(ctx, who, ncol, nz, dt, f, KID_NWARM, "theta, qv, qc, qr and nr of state are required",
                                         FIELD_NAMES, w, w_col_stride, rho, dz, courant, stream);
}

template <class T, class F>
int update_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, T dt, const F *state, const F *t1, const F *t2, const F *t3,
                  int32_t clip, void *stream)
{
    const bool warm = ctx && ctx->cfg.iiwarm != 0;
    const int nf = warm ? KID_NWARM : KID_NF;
    KidUpdate<T, KID_NF> f{};
    members<T>(state, f.state, nf);
    const F *const t[3] = {t1, t2, t3};
    for (int i = 0; i < 3; ++i) {
        T *p[KID_NF];
        members<T>(t[i], p, nf);
        for (int m = 0; m < KID_NF; ++m) f.t[i][m] = p[m];
    }
    return kid_update_members<T, KID_NF>(ctx, who, ncol, nz, dt, f, nf, FIELD_NAMES, clip ? 0x1feu : 0u, stream);   // not theta
}
}  // namespace

template <class T, int N>
int kidmp::kid_advect_members(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, double dt, const KidMembers<T, N> &f, int nreq,
                              const char *required, const char *const *names, const T *w, int64_t w_col_stride, const T *rho,
                              const T *dz, T *courant, void *stream)
{
    const std::string me(who);
    if (int rc = check_shape(ctx, me, ncol, nz, dt)) return rc;
    if (w_col_stride != 0 && w_col_stride < int64_t(nz) + 1) return fail(ctx, KIDMP_EINVAL, me + ": w_col_stride must be 0 or >= nz+1");
    if (ncol == 0) return KIDMP_OK;                                  // an empty batch has nothing to point at
    if (!w || !rho || !dz) return fail(ctx, KIDMP_EINVAL, me + ": null argument (state, w, rho and dz are required)");
    AdvectArgs<T, N> a{};
    bool any = courant != nullptr;
    for (int m = 0; m < N; ++m) {
        if (m < nreq && !f.state[m]) return fail(ctx, KIDMP_EINVAL, me + ": " + required);
        a.state[m] = f.state[m];
        if (f.state[m]) { a.adv[m] = f.adv[m]; a.div[m] = f.div[m]; a.sum[m] = f.sum[m]; }   // not advected: its outputs are not written
        any = any || a.adv[m] || a.div[m] || a.sum[m];
    }
    if (!any) return fail(ctx, KIDMP_EINVAL, me + ": nothing requested: no output member of a present field and no courant");
    GUARD(ctx);
    for (int m = 0; m < N; ++m) {
        if (int rc = check_device_array(ctx, who, a.state[m], names[m])) return rc;
        if (int rc = check_device_array(ctx, who, a.adv[m], "a member of adv")) return rc;
        if (int rc = check_device_array(ctx, who, a.div[m], "a member of div")) return rc;
        if (int rc = check_device_array(ctx, who, a.sum[m], "a member of sum")) return rc;
    }
    const void *more[] = {w, rho, dz, courant};
    const char *what[] = {"w", "rho", "dz", "courant"};
    for (int i = 0; i < 4; ++i)
        if (int rc = check_device_array(ctx, who, more[i], what[i])) return rc;
    a.w = w; a.rho = rho; a.dz = dz; a.w_col_stride = w_col_stride; a.courant = courant; a.dt = dt;
    const dim3 grid((unsigned)((ncol + ADV_WAVES - 1) / ADV_WAVES)), block(ADV_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (ctx->advection == KIDMP_ADVECT_ULTIMATE) launch_advect<T, N, KIDMP_ADVECT_ULTIMATE>(grid, block, st, a, ncol, nz);
    else                                         launch_advect<T, N, KIDMP_ADVECT_VANLEER>(grid, block, st, a, ncol, nz);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}

template <class T, int N>
int kidmp::kid_update_members(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, T dt, const KidUpdate<T, N> &f, int nloop,
                              const char *const *names, uint32_t clip_mask, void *stream)
{
    const std::string me(who);
    if (int rc = check_shape(ctx, me, ncol, nz, double(dt))) return rc;
    if (ncol == 0) return KIDMP_OK;
    UpdateArgs<T, N> a{};
    bool any = false;
    for (int m = 0; m < N; ++m) { a.state[m] = f.state[m]; any = any || a.state[m]; }
    if (!any) return fail(ctx, KIDMP_EINVAL, me + ": nothing requested: state has no member");
    for (int i = 0; i < 3; ++i)
        for (int m = 0; m < N; ++m) a.t[i][m] = a.state[m] ? f.t[i][m] : nullptr;
    GUARD(ctx);
    constexpr int V = 16 / int(sizeof(T));
    bool wide = nz % V == 0;
    for (int m = 0; m < N; ++m) {
        if (int rc = check_device_array(ctx, who, a.state[m], names[m])) return rc;
        wide = wide && aligned16(a.state[m]);
        for (int i = 0; i < 3; ++i) {
            if (int rc = check_device_array(ctx, who, a.t[i][m], "a member of a tendency")) return rc;
            wide = wide && aligned16(a.t[i][m]);
        }
    }
    a.n = ncol * int64_t(nz); a.dt = dt; a.clip = clip_mask;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(wide ? grid_for(a.n / V) : grid_for(a.n)), block(256);
    if constexpr (N == KID_NF) {
        if (wide) {
            if (nloop == KID_NWARM) hipLaunchKernelGGL((k_kid_update<T, V, KID_NWARM, N>), grid, block, 0, s, a);
            else                    hipLaunchKernelGGL((k_kid_update<T, V, KID_NF, N>), grid, block, 0, s, a);
        } else {
            if (nloop == KID_NWARM) hipLaunchKernelGGL((k_kid_update<T, 1, KID_NWARM, N>), grid, block, 0, s, a);
            else                    hipLaunchKernelGGL((k_kid_update<T, 1, KID_NF, N>), grid, block, 0, s, a);
        }
    } else {
        if (wide) hipLaunchKernelGGL((k_kid_update<T, V, N, N>), grid, block, 0, s, a);
        else      hipLaunchKernelGGL((k_kid_update<T, 1, N, N>), grid, block, 0, s, a);
    }
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}

#define KIDMP_INSTANTIATE(T, N) \
    template int kidmp::kid_advect_members<T, N>(kidmp_ctx *, const char *, int64_t, int32_t, double, const KidMembers<T, N> &, int, \
        const char *, const char *const *, const T *, int64_t, const T *, const T *, T *, void *); \
    template int kidmp::kid_update_members<T, N>(kidmp_ctx *, const char *, int64_t, int32_t, T, const KidUpdate<T, N> &, int, \
        const char *const *, uint32_t, void *);
KIDMP_INSTANTIATE(double, KID_NA)
KIDMP_INSTANTIATE(float, KID_NA)
#undef KIDMP_INSTANTIATE

extern "C" {
int kidmp_set_advection(kidmp_ctx *ctx, int32_t scheme)
{
    if (!ctx) return fail(nullptr, KIDMP_ESTATE, "kidmp_set_advection: no context");
    if (scheme != KIDMP_ADVECT_VANLEER && scheme != KIDMP_ADVECT_ULTIMATE)
        return fail(ctx, KIDMP_EINVAL, "kidmp_set_advection: scheme must be KIDMP_ADVECT_VANLEER or KIDMP_ADVECT_ULTIMATE");
    ctx->advection = scheme;
    return KIDMP_OK;
}
int kidmp_advection(const kidmp_ctx *ctx) { return ctx ? int(ctx->advection) : fail(nullptr, KIDMP_ESTATE, "kidmp_advection: no context"); }

int kidmp_kid_advect_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_fields *state,
                            const double *w, int64_t w_col_stride, const double *rho, const double *dz,
                            const kidmp_kid_fields *adv, const kidmp_kid_fields *div, const kidmp_kid_fields *sum, double *courant,
                            void *stream)
{
    return advect_device<double>(ctx, "kidmp_kid_advect_device", ncol, nz, dt, state, w, w_col_stride, rho, dz, adv, div, sum, courant, stream);
}
int kidmp32_kid_advect_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp32_kid_fields *state,
                              const float *w, int64_t w_col_stride, const float *rho, const float *dz,
                              const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div, const kidmp32_kid_fields *sum, float *courant,
                              void *stream)
{
    return advect_device<float>(ctx, "kidmp32_kid_advect_device", ncol, nz, dt, state, w, w_col_stride, rho, dz, adv, div, sum, courant, stream);
}
int kidmp_kid_update_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_fields *state,
                            const kidmp_kid_fields *t1, const kidmp_kid_fields *t2, const kidmp_kid_fields *t3, int32_t clip, void *stream)
{
    return update_device<double>(ctx, "kidmp_kid_update_device", ncol, nz, dt, state, t1, t2, t3, clip, stream);
}
int kidmp32_kid_update_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, const kidmp32_kid_fields *state,
                              const kidmp32_kid_fields *t1, const kidmp32_kid_fields *t2, const kidmp32_kid_fields *t3, int32_t clip,
                              void *stream)
{
    return update_device<float>(ctx, "kidmp32_kid_update_device", ncol, nz, dt, state, t1, t2, t3, clip, stream);
}
}  // extern "C"
