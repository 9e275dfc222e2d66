// kidmp_slab.hip -- the entries of include/kidmp_slab.h: prescribed-(u, w) advection of KiD's nine fields on a batch of
// periodic x-z slabs in the adv / div form the adapter consumes (k_kid_advect_slab).  The schemes (DESIGN.md sections 4.6d
// and 4.6g) are the 1-D entry's in z with the same face value in x, fixed to the operation.  Built with the library's
// plain flags (IEEE division, no contraction): every operation below rounds once.
#include "kidmp_ctx.h"
#include "kidmp_face.h"
#include "kidmp_wave.h"
#include "../../include/kidmp_slab.h"

using namespace kidmp;
using namespace kidmp::wave;

namespace {
constexpr int SLAB_WAVES = 4;                            // W: consecutive cells of one slab (wavefronts) per workgroup
constexpr int SLAB_THREADS = 64 * SLAB_WAVES;
const char *const FIELD_NAMES[KID_NF] = {"theta", "qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg"};

template <class T, int N> struct SlabArgs {              // N members: KiD's nine fields, or the three aerosols
    const T *state[N];
    T *adv[N], *div[N], *sum[N];                         // null: not wanted
    const T *u, *w, *rho, *dz;
    T *courant;
    double dt, dx;
    int32_t nx, nz, shared_flow;
    uint32_t nstrip;                                     // ceil(nx / W)
};

// One wavefront per column, level k = 64 j + lane, as in k_kid_advect; a workgroup owns W consecutive cells of one slab,
// the grid is nslab x ceil(nx / W).  The z part is k_kid_advect's, operation for operation.  What every member shares is
// formed once per column and kept in registers: in z the faces' M, hc, dM and den, in x the mass flux Mx, 0.5*(1 - cx)
// (and what else the scheme S of kidmp_face.h shares) and the upwind side of the cell's two faces i and i+1, dMx and
// denx.  Then each present member is loaded once; its neighbours in z come from the neighbouring lanes, its neighbours in x (cells i-2 .. i+2, periodic) are plain loads
// that the caches serve: the waves of a workgroup and of its neighbours read the same columns at about the same time.
// A stage of the strip in LDS, W = 8 and x faces shared between neighbouring waves were all measured and were no faster
// (the kernel is bound by its binary64 arithmetic), so there is no LDS and no barrier here, and
// a wave beyond the slab's end (nx no multiple of W) may simply leave.  No scratch.
template <class T, int NJ, int N, int S>
__global__ void __launch_bounds__(SLAB_THREADS)
k_kid_advect_slab(const SlabArgs<T, N> a)
{
    const int lane = int(threadIdx.x) & 63;
    const int nx = a.nx, nz = a.nz;
    const int64_t col0 = int64_t(blockIdx.x / a.nstrip) * nx;        // the slab's first column
    const int cell = int(blockIdx.x % a.nstrip) * SLAB_WAVES + (int(threadIdx.x) >> 6);
    if (cell >= nx) return;                                          // whole wavefronts only: the shifts need every lane
    const int cell_r = cell + 1 < nx ? cell + 1 : 0;
    const int64_t base = (col0 + cell) * int64_t(nz);
    int64_t xbase[4];                                                // the columns of cells i-2, i-1, i+1, i+2 (nx >= 3)
    {
        const int d[4] = {nx - 2, nx - 1, 1, 2};
#pragma unroll
        for (int t = 0; t < 4; ++t) xbase[t] = (col0 + (cell + d[t]) % nx) * int64_t(nz);
    }
    const int64_t fcol = a.shared_flow ? cell : col0 + cell, fcol_r = a.shared_flow ? cell_r : col0 + cell_r;
    const T *const w = a.w + fcol * (int64_t(nz) + 1);
    const T *const u0 = a.u + fcol * int64_t(nz), *const u1 = a.u + fcol_r * int64_t(nz);

    constexpr int NG = face::coef_count<S>(NJ);
    double M[NJ], Mup[NJ], den[NJ], hc[NJ], dM[NJ];                  // z, as in k_kid_advect: hc = 0.5*(1.0 - c) of face k
    double g[NG], rc[NG];
    bool up[NJ], second[NJ];
    double Mx0[NJ], Mx1[NJ], hx0[NJ], hx1[NJ], dMx[NJ], denx[NJ];    // x: faces i (0) and i+1 (1) of this cell
    double gx0[NG], gx1[NG], rx0[NG], rx1[NG];
    bool ux0[NJ], ux1[NJ];
    {
        double cz[NJ], czup[NJ], cxm[NJ], above[NJ], cabove[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            M[j] = Mup[j] = hc[j] = cz[j] = czup[j] = cxm[j] = 0.;
            Mx0[j] = Mx1[j] = hx0[j] = hx1[j] = 0.;
            g[j % NG] = rc[j % NG] = gx0[j % NG] = gx1[j % NG] = rx0[j % NG] = rx1[j % NG] = 0.;
            den[j] = denx[j] = 1.;
            up[j] = ux0[j] = ux1[j] = true;
            second[j] = false;
            if (k >= nz) continue;
            const double rho = double(a.rho[k]), dz = double(a.dz[k]), wk = double(w[k]);
            const double rho_lo = k ? double(a.rho[k - 1]) : rho, dz_lo = k ? double(a.dz[k - 1]) : dz;
            const double rf = k ? 0.5 * (rho_lo + rho) : rho;
            up[j] = wk >= 0.;
            second[j] = up[j] ? k >= 2 : k + 1 < nz;
            M[j] = rf * wk;
            cz[j] = (fabs(wk) * a.dt) / (up[j] ? dz_lo : dz);
            face::coef<S>(cz[j], hc[j], g[j % NG], rc[j % NG]);
            den[j] = rho * dz;
            if (k == nz - 1) {                                       // the model top: rf = rho[nz-1], dz[nz-1]
                const double wt = double(w[nz]);
                Mup[j] = rho * wt;
                czup[j] = (fabs(wt) * a.dt) / dz;
            }
            const double ul = double(u0[k]), ur = double(u1[k]);
            ux0[j] = ul >= 0.;
            ux1[j] = ur >= 0.;
            Mx0[j] = rho * ul;
            Mx1[j] = rho * ur;
            const double cx0 = (fabs(ul) * a.dt) / a.dx, cx1 = (fabs(ur) * a.dt) / a.dx;
            face::coef<S>(cx0, hx0[j], gx0[j % NG], rx0[j % NG]);
            face::coef<S>(cx1, hx1[j], gx1[j % NG], rx1[j % NG]);
            denx[j] = rho * a.dx;
            cxm[j] = fmax(cx0, cx1);
        }
        level_above<NJ>(M, above);
        level_above<NJ>(cz, cabove);
        double cmax = 0.;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            if (k != nz - 1) { Mup[j] = above[j]; czup[j] = cabove[j]; }
            dM[j] = (Mup[j] - M[j]) / den[j];
            dMx[j] = (Mx1[j] - Mx0[j]) / denx[j];
            if (k < nz) cmax = fmax(cmax, fmax(cz[j], czup[j]) + cxm[j]);    // the cell's unsplit stability number
        }
        if (a.courant) {
            cmax = wave_max(cmax);
            if (lane == 0) a.courant[col0 + cell] = T(cmax);
        }
    }

#pragma unroll
    for (int m = 0; m < N; ++m) {
        if (!a.state[m] || !(a.adv[m] || a.div[m] || a.sum[m])) continue;
        double q[NJ], q1[NJ], q2[NJ], qa[NJ], F[NJ], Fup[NJ], dFx[NJ];
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
            // the x faces of this cell: i between cells i-1 and i, i+1 between cells i and i+1
            const bool in = k < nz;
            const double l2 = in ? double(a.state[m][xbase[0] + k]) : 0., l1 = in ? double(a.state[m][xbase[1] + k]) : 0.;
            const double r1 = in ? double(a.state[m][xbase[2] + k]) : 0., r2 = in ? double(a.state[m][xbase[3] + k]) : 0.;
            double Fx[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const bool pos = f ? ux1[j] : ux0[j];
                const double xu = f ? (pos ? q[j] : r1) : (pos ? l1 : q[j]);
                const double xd = f ? (pos ? r1 : q[j]) : (pos ? q[j] : l1);
                const double xuu = f ? (pos ? l1 : r2) : (pos ? l2 : r1);
                Fx[f] = (f ? Mx1[j] : Mx0[j]) * face::value<S>(f ? hx1[j] : hx0[j], f ? gx1[j % NG] : gx0[j % NG], f ? rx1[j % NG] : rx0[j % NG],
                                                                  true, xu, xd, xuu);
            }
            dFx[j] = Fx[1] - Fx[0];
        }
        level_above<NJ>(F, Fup);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 64 * j + lane;
            if (k >= nz) continue;
            if (k == nz - 1) Fup[j] = Mup[j] * q[j];                 // qf[nz] = q[nz-1]
            const double adv = -((Fup[j] - F[j]) / den[j]) + -(dFx[j] / denx[j]);
            const double div = q[j] * dM[j] + q[j] * dMx[j];
            if (a.adv[m]) a.adv[m][base + k] = T(adv);
            if (a.div[m]) a.div[m][base + k] = T(div);
            if (a.sum[m]) a.sum[m][base + k] = T(adv + div);
        }
    }
}

template <class T, int N, int S> void launch_slab(dim3 grid, dim3 block, hipStream_t st, const SlabArgs<T, N> &a)
{
    switch ((a.nz + 63) / 64) {
    case 1: hipLaunchKernelGGL((k_kid_advect_slab<T, 1, N, S>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_kid_advect_slab<T, 2, N, S>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_kid_advect_slab<T, 3, N, S>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((k_kid_advect_slab<T, 4, N, S>), grid, block, 0, st, a); break;
    }
}

template <class T, class F> void members(const F *f, T *(&out)[KID_NF], int nf)
{
    for (int m = 0; m < KID_NF; ++m) out[m] = nullptr;
    if (!f) return;
    T *const p[KID_NF] = {f->theta, f->qv, f->qc, f->qr, f->nr, f->qi, f->ni, f->qs, f->qg};
    for (int m = 0; m < nf; ++m) out[m] = p[m];
}

template <class T, class F>
int advect_slab_device(kidmp_ctx *ctx, const char *who, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx, const F *state,
                       const T *u, const T *w, int32_t shared_flow, const T *rho, const T *dz, const F *adv, const F *div, const F *sum,
                       T *courant, void *stream)
{
    const int nf = ctx && ctx->cfg.iiwarm ? KID_NWARM : KID_NF;      // the frozen members are not looked at in a warm context
    KidMembers<T, KID_NF> f{};
    members<T>(state, f.state, nf);
    members<T>(adv, f.adv, nf);
    members<T>(div, f.div, nf);
    members<T>(sum, f.sum, nf);
    return kid_advect_slab_members<T, KID_NF>(ctx, who, {nslab, nx, nz, dt, dx, shared_flow}, f, KID_NWARM,
                                              "theta, qv, qc, qr and nr of state are required", FIELD_NAMES, u, w, rho, dz, courant, stream);
}
}  // namespace

template <class T, int N>
int kidmp::kid_advect_slab_members(kidmp_ctx *ctx, const char *who, const KidSlabShape &g, const KidMembers<T, N> &f, int nreq,
                                   const char *required, const char *const *names, const T *u, const T *w, const T *rho, const T *dz,
                                   T *courant, void *stream)
{
    const std::string me(who);
    const int64_t nslab = g.nslab;
    const int32_t nx = g.nx, nz = g.nz;
    if (int rc = require_ready(ctx)) return rc;
    if (nslab < 0) return fail(ctx, KIDMP_EINVAL, me + ": nslab < 0");
    if (nx < 3) return fail(ctx, KIDMP_EINVAL, me + ": nx < 3 (the stencil i-2 .. i+2 must name distinct cells)");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, me + ": nz outside [2, KIDMP_MAX_NZ]");
    if (!(g.dt > 0.)) return fail(ctx, KIDMP_EINVAL, me + ": dt must be > 0");
    if (!(g.dx > 0.)) return fail(ctx, KIDMP_EINVAL, me + ": dx must be > 0");
    if (nslab > int64_t(0x7fffffff) / nx) return fail(ctx, KIDMP_EINVAL, me + ": more columns than one launch takes");
    if (nslab == 0) return KIDMP_OK;                                 // an empty batch has nothing to point at
    if (!u || !w || !rho || !dz) return fail(ctx, KIDMP_EINVAL, me + ": null argument (state, u, w, rho and dz are required)");
    SlabArgs<T, N> a{};
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
    const void *more[] = {u, w, rho, dz, courant};
    const char *what[] = {"u", "w", "rho", "dz", "courant"};
    for (int i = 0; i < 5; ++i)
        if (int rc = check_device_array(ctx, who, more[i], what[i])) return rc;
    a.u = u; a.w = w; a.rho = rho; a.dz = dz; a.courant = courant; a.dt = g.dt; a.dx = g.dx;
    a.nx = nx; a.nz = nz; a.shared_flow = g.shared_flow != 0;
    a.nstrip = uint32_t((nx + SLAB_WAVES - 1) / SLAB_WAVES);
    const dim3 grid((unsigned)(nslab * a.nstrip)), block(SLAB_THREADS);      // <= nslab*nx <= 0x7fffffff
    hipStream_t st = (hipStream_t)stream;
    if (ctx->advection == KIDMP_ADVECT_ULTIMATE) launch_slab<T, N, KIDMP_ADVECT_ULTIMATE>(grid, block, st, a);
    else                                         launch_slab<T, N, KIDMP_ADVECT_VANLEER>(grid, block, st, a);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}
template int kidmp::kid_advect_slab_members<double, KID_NA>(kidmp_ctx *, const char *, const KidSlabShape &, const KidMembers<double, KID_NA> &,
    int, const char *, const char *const *, const double *, const double *, const double *, const double *, double *, void *);
template int kidmp::kid_advect_slab_members<float, KID_NA>(kidmp_ctx *, const char *, const KidSlabShape &, const KidMembers<float, KID_NA> &,
    int, const char *, const char *const *, const float *, const float *, const float *, const float *, float *, void *);

extern "C" {
int kidmp_kid_advect_slab_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
                                 const kidmp_kid_fields *state, const double *u, const double *w, int32_t shared_flow, const double *rho,
                                 const double *dz, const kidmp_kid_fields *adv, const kidmp_kid_fields *div, const kidmp_kid_fields *sum,
                                 double *courant, void *stream)
{
    return advect_slab_device<double>(ctx, "kidmp_kid_advect_slab_device", nslab, nx, nz, dt, dx, state, u, w, shared_flow, rho, dz, adv, div, sum,
                                      courant, stream);
}
int kidmp32_kid_advect_slab_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
                                   const kidmp32_kid_fields *state, const float *u, const float *w, int32_t shared_flow, const float *rho,
                                   const float *dz, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div, const kidmp32_kid_fields *sum,
                                   float *courant, void *stream)
{
    return advect_slab_device<float>(ctx, "kidmp32_kid_advect_slab_device", nslab, nx, nz, dt, dx, state, u, w, shared_flow, rho, dz, adv, div, sum,
                                     courant, stream);
}
}  // extern "C"
