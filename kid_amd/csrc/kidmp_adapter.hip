// kidmp_adapter.hip -- mphys_thompson09_interfacen (W:28-310) on the device: the gather of the step's inputs from KiD's
// theta-form fields (W:46-97, with the U2 defaults of DESIGN.md section 2) and the back-out of the tendencies (W:198-245)
// as two streaming kernels around the column step, and the device entries of include/kidmp.h over them.
// Built with the library's plain flags (IEEE division, no contraction): every operation below rounds once, in T.
#include <cmath>

#include "kidmp_ctx.h"
#include "kidmp_stream.h"

using namespace kidmp;
using namespace kidmp::streaming;

namespace {
// KID_WORK_OF for device code
__host__ __device__ constexpr int work_of(int m)
{
    constexpr int t[KID_NF] = {11, 0, 1, 3, 7, 2, 6, 4, 5};
    return t[m];
}
static_assert(work_of(0) == KID_WORK_OF[0] && work_of(4) == KID_WORK_OF[4] && work_of(8) == KID_WORK_OF[8], "kidmp_ctx.h");

template <class T> struct GatherArgs {
    const T *state[KID_NF], *adv[KID_NF], *div[KID_NF];
    const T *exner, *dz;                             // dz: KiD's one profile [nz]
    T *work[KID_NWORK];
    T *ppt;
    int64_t n, ncol;                                 // n = ncol*nz elements
    int32_t nz;
    T dt, p0, expo, Nt_c;                            // expo = 1./r_on_cp, formed in T
    const double *set_nc_col;                        // kidmp_set_column_nc: the batch's first column, or null
    // AERO (include/kidmp_aerosol.h): nc, nwfa, nifa with their forcing, and the cell-centre updraft
    const T *aer[KID_NA], *aer_adv[KID_NA], *aer_div[KID_NA];
    const T *w;
    int64_t w_col_stride;
};
template <class T> struct BackoutArgs {
    const T *state[KID_NF], *adv[KID_NF], *div[KID_NF];
    const T *exner;
    T *work[KID_NWORK];                              // read; AERO with a surface source: level 0 of profile 9 is written
    T *mphys[KID_NF];
    int64_t n;
    T dt;
    const T *aer[KID_NA], *aer_adv[KID_NA], *aer_div[KID_NA];       // AERO, as in GatherArgs
    T *aer_mphys[KID_NA];
    const T *nwfa_src;
    int32_t nz;
};

// p = p0 * exner**(1./r_on_cp) (W:62).  binary64: the device libm's pow (under 1 ulp).  binary32: pow in binary64 rounded
// once is a correctly rounded powf, which is what the native reference calls.
__device__ inline double pres_of(double p0, double exner, double expo) { return p0 * pow(exner, expo); }
__device__ inline float pres_of(float p0, float exner, float expo) { return p0 * float(pow(double(exner), double(expo))); }

// W:46-97 + U2.  One element (V of them) per lane-slot; NF = KID_NWARM in an iiwarm context, where the four frozen
// profiles are exact zeros (W:46-52) and their inputs are not looked at.  AERO: profiles 8, 9 and 10 are the caller's nc,
// nwfa and nifa moved on like the other moments instead of the U2 defaults, and profile 13 is the caller's updraft.
template <class T, int V, int NF, bool AERO>
__global__ __launch_bounds__(256) void k_kid_gather(const GatherArgs<T> a)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (int64_t i = tid; i < 4 * a.ncol; i += stride) a.ppt[i] = T(0);          // W:55-58: OUT, not INOUT
    const int64_t nvec = a.n / V;
    for (int64_t i = tid; i < nvec; i += stride) {
        const int64_t e = i * V;                                                 // (nz % V == 0: the V elements share a column)
        const int64_t col = a.n <= 0x7fffffff ? int64_t(int32_t(e) / a.nz) : e / a.nz;
        Vec<T, V> x[NF], xa[NF], xd[NF];
#pragma unroll
        for (int m = 0; m < NF; ++m) { x[m] = ld<T, V>(a.state[m], e); xa[m] = ld<T, V>(a.adv[m], e); xd[m] = ld<T, V>(a.div[m], e); }
        const Vec<T, V> ex = ld<T, V>(a.exner, e), dz = ld<T, V>(a.dz, e - col * a.nz);
        Vec<T, V> g[NF], p, n3[KID_NA], w, zero;                                 // n3: nc, nwfa, nifa
        if constexpr (AERO) {
            Vec<T, V> y[KID_NA], ya[KID_NA], yd[KID_NA];
#pragma unroll
            for (int m = 0; m < KID_NA; ++m) { y[m] = ld<T, V>(a.aer[m], e); ya[m] = ld<T, V>(a.aer_adv[m], e); yd[m] = ld<T, V>(a.aer_div[m], e); }
            w = ld<T, V>(a.w, col * a.w_col_stride + (e - col * a.nz));          // (wide: the stride is a multiple of V)
#pragma unroll
            for (int j = 0; j < V; ++j)
#pragma unroll
                for (int m = 0; m < KID_NA; ++m) n3[m].v[j] = y[m].v[j] + (ya[m].v[j] + yd[m].v[j]) * a.dt;   // as W:60-93
        }
        const T Nt_c = !AERO && a.set_nc_col ? T(a.set_nc_col[col] * 1.e6) : a.Nt_c;      // as k_default_aerosols
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma unroll
            for (int m = 0; m < NF; ++m) g[m].v[j] = x[m].v[j] + (xa[m].v[j] + xd[m].v[j]) * a.dt;    // W:60-93
            g[0].v[j] = g[0].v[j] * ex.v[j];                                     // t = (theta + ...)*exner, W:60
            p.v[j] = pres_of(a.p0, ex.v[j], a.expo);
            zero.v[j] = T(0);
            if constexpr (!AERO) {
                const T rho = T(0.622) * p.v[j] / (T(Rgas) * g[0].v[j] * (g[1].v[j] + T(0.622)));   // M:959
                n3[0].v[j] = Nt_c / rho;                                         // M:960
                n3[1].v[j] = T(11.1E6) / rho;                                    // M:961
                n3[2].v[j] = T(naIN1) * T(0.01) / rho;                           // M:962
                w.v[j] = T(0);
            }
        }
#pragma unroll
        for (int m = 0; m < NF; ++m) st<T, V>(a.work[work_of(m)], e, g[m]);
#pragma unroll
        for (int m = NF; m < KID_NF; ++m) st<T, V>(a.work[work_of(m)], e, zero);
#pragma unroll
        for (int m = 0; m < KID_NA; ++m) st<T, V>(a.work[KID_AER_WORK0 + m], e, n3[m]);
        st<T, V>(a.work[12], e, p); st<T, V>(a.work[13], e, w); st<T, V>(a.work[14], e, dz);
    }
}

// W:198-245 on the post-step workspace.  AERO: first the surface source of M:1001 into level 0 of profile 9 (the V
// elements of a lane-slot share a column, so level 0 is element 0 of the slot that begins a column), then the three
// aerosol tendencies like the others.
template <class T, int V, int NF, bool AERO>
__global__ __launch_bounds__(256) void k_kid_backout(const BackoutArgs<T> a)
{
    const int64_t stride = int64_t(gridDim.x) * blockDim.x, nvec = a.n / V;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const int64_t e = i * V;
        Vec<T, V> x[NF], xa[NF], xd[NF], x1[NF];
#pragma unroll
        for (int m = 0; m < NF; ++m) {
            x[m] = ld<T, V>(a.state[m], e); xa[m] = ld<T, V>(a.adv[m], e); xd[m] = ld<T, V>(a.div[m], e);
            x1[m] = ld<T, V>(a.work[work_of(m)], e);
        }
        const Vec<T, V> ex = ld<T, V>(a.exner, e);
        Vec<T, V> r[NF];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            r[0].v[j] = (x1[0].v[j] / ex.v[j] - x[0].v[j]) / a.dt - (xa[0].v[j] + xd[0].v[j]);       // W:199-201
#pragma unroll
            for (int m = 1; m < NF; ++m) r[m].v[j] = (x1[m].v[j] - x[m].v[j]) / a.dt - (xa[m].v[j] + xd[m].v[j]);
        }
#pragma unroll
        for (int m = 0; m < NF; ++m) st<T, V>(a.mphys[m], e, r[m]);
        if constexpr (AERO) {
            Vec<T, V> y[KID_NA], ya[KID_NA], yd[KID_NA], y1[KID_NA];
#pragma unroll
            for (int m = 0; m < KID_NA; ++m) {
                y[m] = ld<T, V>(a.aer[m], e); ya[m] = ld<T, V>(a.aer_adv[m], e); yd[m] = ld<T, V>(a.aer_div[m], e);
                y1[m] = ld<T, V>(a.work[KID_AER_WORK0 + m], e);
            }
            if (a.nwfa_src) {
                const int64_t col = a.n <= 0x7fffffff ? int64_t(int32_t(e) / a.nz) : e / a.nz;
                if (e == col * a.nz) {
                    y1[1].v[0] = y1[1].v[0] + a.nwfa_src[col] * a.dt;
                    a.work[KID_AER_WORK0 + 1][e] = y1[1].v[0];
                }
            }
#pragma unroll
            for (int m = 0; m < KID_NA; ++m) {
                Vec<T, V> s;
#pragma unroll
                for (int j = 0; j < V; ++j) s.v[j] = (y1[m].v[j] - y[m].v[j]) / a.dt - (ya[m].v[j] + yd[m].v[j]);
                st<T, V>(a.aer_mphys[m], e, s);
            }
        }
    }
}

template <class T, class A> bool wide_ok(const A &a, int32_t nz, const void *const *more, int nmore)
{
    constexpr int V = 16 / int(sizeof(T));
    if (nz % V) return false;
    for (int m = 0; m < KID_NF; ++m)
        if (!aligned16(a.state[m]) || !aligned16(a.adv[m]) || !aligned16(a.div[m])) return false;
    for (int v = 0; v < KID_NWORK; ++v)
        if (!aligned16(a.work[v])) return false;
    for (int i = 0; i < nmore; ++i)
        if (!aligned16(more[i])) return false;
    for (int m = 0; m < KID_NA; ++m)                     // null unless AERO
        if (!aligned16(a.aer[m]) || !aligned16(a.aer_adv[m]) || !aligned16(a.aer_div[m])) return false;
    return true;
}

template <class T> hipError_t launch_gather(const GatherArgs<T> &a, bool warm, bool aero, hipStream_t s)
{
    constexpr int V = 16 / int(sizeof(T));
    const void *more[] = {a.exner, a.dz, a.w};
    const bool wide = wide_ok<T>(a, a.nz, more, 3) && a.w_col_stride % V == 0;
    const dim3 grid(wide ? grid_for(a.n / V) : grid_for(a.n)), block(256);
#define KID_GATHER(W, NF_) do { if (aero) hipLaunchKernelGGL((k_kid_gather<T, W, NF_, true>), grid, block, 0, s, a); \
                                else      hipLaunchKernelGGL((k_kid_gather<T, W, NF_, false>), grid, block, 0, s, a); } while (0)
    if (wide) { if (warm) KID_GATHER(V, KID_NWARM); else KID_GATHER(V, KID_NF); }
    else      { if (warm) KID_GATHER(1, KID_NWARM); else KID_GATHER(1, KID_NF); }
#undef KID_GATHER
    return hipGetLastError();
}
template <class T> hipError_t launch_backout(const BackoutArgs<T> &a, int32_t nz, bool warm, bool aero, hipStream_t s)
{
    constexpr int V = 16 / int(sizeof(T));
    const void *more[KID_NF + KID_NA + 1] = {a.exner};
    for (int m = 0; m < KID_NF; ++m) more[m + 1] = a.mphys[m];
    for (int m = 0; m < KID_NA; ++m) more[KID_NF + 1 + m] = a.aer_mphys[m];
    const bool wide = wide_ok<T>(a, nz, more, KID_NF + KID_NA + 1);
    const dim3 grid(wide ? grid_for(a.n / V) : grid_for(a.n)), block(256);
#define KID_BACKOUT(W, NF_) do { if (aero) hipLaunchKernelGGL((k_kid_backout<T, W, NF_, true>), grid, block, 0, s, a); \
                                 else      hipLaunchKernelGGL((k_kid_backout<T, W, NF_, false>), grid, block, 0, s, a); } while (0)
    if (wide) { if (warm) KID_BACKOUT(V, KID_NWARM); else KID_BACKOUT(V, KID_NF); }
    else      { if (warm) KID_BACKOUT(1, KID_NWARM); else KID_BACKOUT(1, KID_NF); }
#undef KID_BACKOUT
    return hipGetLastError();
}

template <class T, class F, class O>
int kid_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, T dt, T p0, T r_on_cp, const F *state, const F *adv,
               const F *div, const T *exner, const T *dz, const F *mphys, T *ppt, double *rates, int32_t *nstep, const O *out,
               int32_t arith, void *work, size_t work_bytes, void *stream, bool gather_only = false)
{
    KidCall<T> c{};
    ColumnOutputs<T> o{};
    if (out) o = {out->dbz, out->re_qc, out->re_qi, out->re_qs};
    if (int rc = kid_check<T, F>(ctx, who, ncol, nz, double(dt), state, adv, div, exner, dz, mphys, ppt, o, arith, c)) return rc;
    if (ncol == 0) return KIDMP_OK;
    c.dt = dt; c.p0 = p0; c.r_on_cp = r_on_cp; c.rates = rates; c.nstep = nstep;
    return kid_device_call<T>(ctx, who, c, work, work_bytes, stream, gather_only);
}
}  // namespace

template <class T>
int kidmp::kid_device_call(kidmp_ctx *ctx, const char *who, const KidCall<T> &c, void *work, size_t work_bytes, void *stream, bool gather_only)
{
    const std::string w(who);
    if (!work || work_bytes < size_t(KID_NWORK) * kid_stride(c.ncol, c.nz, sizeof(T)))
        return fail(ctx, KIDMP_EINVAL, w + ": the workspace is missing or smaller than kidmp_kid_workspace_bytes(ncol, nz)");
    if (!aligned16(work)) return fail(ctx, KIDMP_EINVAL, w + ": the workspace must be 16-byte aligned");
    GUARD(ctx);
    const void *ptrs[] = {c.state.f[0], c.mphys.f[0], c.exner, c.dz, c.ppt, work, c.rates, c.nstep};
    const char *names[] = {"state", "mphys", "exner", "dz", "ppt", "work", "rates", "nstep"};
    for (int i = 0; i < 8; ++i)
        if (int rc = check_on_device(ctx, ptrs[i], names[i])) return rc;
    if (c.aer.on) {
        const void *more[] = {c.aer.state[0], c.aer.state[1], c.aer.state[2], c.aer.adv[0], c.aer.adv[1], c.aer.adv[2],
                              c.aer.div[0], c.aer.div[1], c.aer.div[2], c.aer.mphys[0], c.aer.mphys[1], c.aer.mphys[2],
                              c.aer.w, c.aer.nwfa_src};
        const char *what[] = {"aer->nc", "aer->nwfa", "aer->nifa", "aer_adv->nc", "aer_adv->nwfa", "aer_adv->nifa", "aer_div->nc",
                              "aer_div->nwfa", "aer_div->nifa", "aer_mphys->nc", "aer_mphys->nwfa", "aer_mphys->nifa", "w", "nwfa_src"};
        for (int i = 0; i < 14; ++i)
            if (int rc = check_on_device(ctx, more[i], what[i])) return rc;
    }
    return kid_enqueue<T>(ctx, c, work, (hipStream_t)stream, -1, gather_only);
}
template int kidmp::kid_device_call<double>(kidmp_ctx *, const char *, const KidCall<double> &, void *, size_t, void *, bool);
template int kidmp::kid_device_call<float>(kidmp_ctx *, const char *, const KidCall<float> &, void *, size_t, void *, bool);

template <class T, class F>
int kidmp::kid_check(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, double dt, const F *state, const F *adv, const F *div,
                     const T *exner, const T *dz, const F *mphys, T *ppt, const ColumnOutputs<T> &out, int32_t arith, KidCall<T> &c)
{
    if (int rc = require_ready(ctx)) return rc;
    const std::string w(who);
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (!(dt > 0.)) return fail(ctx, KIDMP_EINVAL, w + ": dt must be > 0");
    if (std::is_same<T, float>::value && !valid_arith(arith)) return fail(ctx, KIDMP_EINVAL, BAD_ARITH);
    if (ncol > int64_t(0x7fffffff)) return fail(ctx, KIDMP_EINVAL, w + ": more columns than one launch takes");
    c.ncol = ncol; c.nz = nz; c.arith = arith; c.exner = exner; c.dz = dz; c.ppt = ppt; c.out = out;
    if (ncol == 0) return KIDMP_OK;                              // an empty batch has nothing to point at
    if (!state || !mphys || !exner || !dz || !ppt) return fail(ctx, KIDMP_EINVAL, w + ": null argument (state, mphys, exner, dz and ppt are required)");
    const int nf = ctx->cfg.iiwarm ? KID_NWARM : KID_NF;         // the frozen members are not looked at in a warm context
    T *const s[KID_NF] = {state->theta, state->qv, state->qc, state->qr, state->nr, state->qi, state->ni, state->qs, state->qg};
    T *const m[KID_NF] = {mphys->theta, mphys->qv, mphys->qc, mphys->qr, mphys->nr, mphys->qi, mphys->ni, mphys->qs, mphys->qg};
    for (int i = 0; i < KID_NF; ++i) {
        c.state.f[i] = i < nf ? s[i] : nullptr;
        c.mphys.f[i] = i < nf ? m[i] : nullptr;
        c.adv.f[i] = c.div.f[i] = nullptr;
    }
    for (int i = 0; i < nf; ++i)
        if (!s[i] || !m[i])
            return fail(ctx, KIDMP_EINVAL, w + (i < KID_NWARM ? ": a required member of state or mphys is null"
                                                              : ": a mixed-phase context needs qi, ni, qs and qg of state and mphys"));
    if (adv) { T *const a[KID_NF] = {adv->theta, adv->qv, adv->qc, adv->qr, adv->nr, adv->qi, adv->ni, adv->qs, adv->qg};
               for (int i = 0; i < nf; ++i) c.adv.f[i] = a[i]; }
    if (div) { T *const d[KID_NF] = {div->theta, div->qv, div->qc, div->qr, div->nr, div->qi, div->ni, div->qs, div->qg};
               for (int i = 0; i < nf; ++i) c.div.f[i] = d[i]; }
    if (int rc = check_nc_count(ctx, who, ncol)) return rc;
    return check_outputs_request<T>(ctx, who, out);
}
template int kidmp::kid_check<double, kidmp_kid_fields>(kidmp_ctx *, const char *, int64_t, int32_t, double, const kidmp_kid_fields *,
    const kidmp_kid_fields *, const kidmp_kid_fields *, const double *, const double *, const kidmp_kid_fields *, double *,
    const ColumnOutputs<double> &, int32_t, KidCall<double> &);
template int kidmp::kid_check<float, kidmp32_kid_fields>(kidmp_ctx *, const char *, int64_t, int32_t, double, const kidmp32_kid_fields *,
    const kidmp32_kid_fields *, const kidmp32_kid_fields *, const float *, const float *, const kidmp32_kid_fields *, float *,
    const ColumnOutputs<float> &, int32_t, KidCall<float> &);

template <class T>
int kidmp::kid_enqueue(kidmp_ctx *ctx, const KidCall<T> &c, void *work, hipStream_t s, int64_t nc_first, bool gather_only)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    const size_t stride = kid_stride(c.ncol, c.nz, sizeof(T));
    T *w[KID_NWORK];
    for (int v = 0; v < KID_NWORK; ++v) w[v] = reinterpret_cast<T *>(static_cast<char *>(work) + size_t(v) * stride);
    GatherArgs<T> g{};
    BackoutArgs<T> b{};
    for (int m = 0; m < KID_NF; ++m) {
        g.state[m] = b.state[m] = c.state.f[m]; g.adv[m] = b.adv[m] = c.adv.f[m]; g.div[m] = b.div[m] = c.div.f[m];
        b.mphys[m] = c.mphys.f[m];
    }
    for (int v = 0; v < KID_NWORK; ++v) { g.work[v] = w[v]; b.work[v] = w[v]; }
    g.exner = b.exner = c.exner; g.dz = c.dz; g.ppt = c.ppt;
    g.n = b.n = c.ncol * int64_t(c.nz); g.ncol = c.ncol; g.nz = c.nz;
    g.dt = b.dt = c.dt; g.p0 = c.p0; g.expo = T(1) / c.r_on_cp; g.Nt_c = T(ctx->hc.Nt_c);
    g.set_nc_col = ctx->d_nc_col ? ctx->d_nc_col + (nc_first > 0 ? nc_first : 0) : nullptr;
    const bool aero = c.aer.on;
    if (aero) {
        for (int m = 0; m < KID_NA; ++m) {
            g.aer[m] = b.aer[m] = c.aer.state[m]; g.aer_adv[m] = b.aer_adv[m] = c.aer.adv[m]; g.aer_div[m] = b.aer_div[m] = c.aer.div[m];
            b.aer_mphys[m] = c.aer.mphys[m];
        }
        g.w = c.aer.w; g.w_col_stride = c.aer.w_col_stride; b.nwfa_src = c.aer.nwfa_src; b.nz = c.nz;
    }
    HIPTRY(ctx, launch_gather<T>(g, warm, aero, s));
    if (gather_only) return KIDMP_OK;
    if (int rc = step_device<T>(ctx, c.ncol, c.nz, c.dt, w, w[12], w[13], w[14], c.ppt, c.rates, c.nstep, c.arith, s, nc_first)) return rc;
    if (c.out.dbz || c.out.re_qc)                                // of the post-step state, as the host pipeline forms them
        HIPTRY(ctx, launch_outputs<T>(ctx, c.ncol, c.nz, {w[11], w[12], w[0], w[1], w[8], w[2], w[6], w[3], w[7], w[4], w[5]}, c.out, s,
                                      nc_first > 0 ? nc_first : 0));
    HIPTRY(ctx, launch_backout<T>(b, c.nz, warm, aero, s));
    return KIDMP_OK;
}
template int kidmp::kid_enqueue<double>(kidmp_ctx *, const KidCall<double> &, void *, hipStream_t, int64_t, bool);
template int kidmp::kid_enqueue<float>(kidmp_ctx *, const KidCall<float> &, void *, hipStream_t, int64_t, bool);

extern "C" {
size_t kidmp_kid_workspace_bytes(int64_t ncol, int32_t nz) { return size_t(KID_NWORK) * kid_stride(ncol, nz, sizeof(double)); }
size_t kidmp32_kid_workspace_bytes(int64_t ncol, int32_t nz) { return size_t(KID_NWORK) * kid_stride(ncol, nz, sizeof(float)); }
size_t kidmp_kid_workspace_offset(int64_t ncol, int32_t nz, int32_t v)
{ return v < 0 || v >= KID_NWORK ? 0 : size_t(v) * kid_stride(ncol, nz, sizeof(double)); }
size_t kidmp32_kid_workspace_offset(int64_t ncol, int32_t nz, int32_t v)
{ return v < 0 || v >= KID_NWORK ? 0 : size_t(v) * kid_stride(ncol, nz, sizeof(float)); }

int kidmp_kid_interface_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                               const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                               const double *exner, const double *dz, const kidmp_kid_fields *mphys, double *ppt,
                               double *rates, int32_t *nstep, const kidmp_outputs *out,
                               void *work, size_t work_bytes, void *stream)
{
    return kid_device<double>(ctx, "kidmp_kid_interface_device", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, ppt,
                              rates, nstep, out, 0, work, work_bytes, stream);
}
int kidmp32_kid_interface_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                                 const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                                 const float *exner, const float *dz, const kidmp32_kid_fields *mphys, float *ppt,
                                 double *rates, int32_t *nstep, const kidmp32_outputs *out, int32_t arith,
                                 void *work, size_t work_bytes, void *stream)
{
    return kid_device<float>(ctx, "kidmp32_kid_interface_device", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, ppt,
                             rates, nstep, out, arith, work, work_bytes, stream);
}
// the gather alone (`state` stands in for mphys, which is not looked at)
int kidmp_kid_gather_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                            const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                            const double *exner, const double *dz, double *ppt, void *work, size_t work_bytes, void *stream)
{
    return kid_device<double, kidmp_kid_fields, kidmp_outputs>(ctx, "kidmp_kid_gather_device", ncol, nz, dt, p0, r_on_cp, state, adv, div,
                                                               exner, dz, state, ppt, nullptr, nullptr, nullptr, 0, work, work_bytes,
                                                               stream, true);
}
int kidmp32_kid_gather_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                              const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                              const float *exner, const float *dz, float *ppt, void *work, size_t work_bytes, void *stream)
{
    return kid_device<float, kidmp32_kid_fields, kidmp32_outputs>(ctx, "kidmp32_kid_gather_device", ncol, nz, dt, p0, r_on_cp, state, adv,
                                                                  div, exner, dz, state, ppt, nullptr, nullptr, nullptr, KIDMP_ARITH_P32N,
                                                                  work, work_bytes, stream, true);
}
}  // extern "C"
