// kidmp_aerosol.hip -- the entries of include/kidmp_aerosol.h: nc, nwfa, nifa and the updraft through the adapter, both
// advection entries and the update, for an aerosol-aware context.  No kernel lives here: the gather and the back-out are
// the AERO instantiations of k_kid_gather / k_kid_backout (kidmp_adapter.hip), the advection and the update are the
// three-member instantiations of k_kid_advect, k_kid_advect_slab and k_kid_update (kidmp_kinematic.hip, kidmp_slab.hip), so
// the per-member arithmetic stays where it was.  This unit checks the arguments and unpacks the structs.
#include "kidmp_ctx.h"
#include "../../include/kidmp_aerosol.h"

using namespace kidmp;

namespace {
const char *const AER_NAMES[KID_NA] = {"nc", "nwfa", "nifa"};

template <class T, class A> void members(const A *a, T *(&out)[KID_NA])
{
    for (int m = 0; m < KID_NA; ++m) out[m] = nullptr;
    if (a) { out[0] = a->nc; out[1] = a->nwfa; out[2] = a->nifa; }
}

// gather_only: `state` and `aer` stand in for mphys and aer_mphys, which are not looked at
template <class T, class F, class A, class O>
int interface_aero(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, T dt, T p0, T r_on_cp, const F *state, const F *adv,
                   const F *div, const T *exner, const T *dz, const F *mphys, T *ppt, double *rates, int32_t *nstep, const O *out,
                   int32_t arith, const A *aer, const A *aer_adv, const A *aer_div, const A *aer_mphys, const T *w, int64_t w_col_stride,
                   const T *nwfa_src, void *work, size_t work_bytes, void *stream, bool gather_only = false)
{
    KidCall<T> c{};
    ColumnOutputs<T> o{};
    if (out) o = {out->dbz, out->re_qc, out->re_qi, out->re_qs};
    if (int rc = kid_check<T, F>(ctx, who, ncol, nz, double(dt), state, adv, div, exner, dz, gather_only ? state : mphys, ppt, o, arith, c))
        return rc;
    const std::string me(who);
    if (!ctx->cfg.is_aerosol_aware)
        return fail(ctx, KIDMP_EINVAL, me + ": the context is not aerosol-aware (kidmp_cfg.is_aerosol_aware); kidmp_kid_interface_device "
                                            "serves it with the default aerosols");
    // the all-binary32 column step of an aerosol-aware context hung on the MI355X the first time it was run (DESIGN.md
    // section 4.6e; no earlier test had stepped it): not offered here until its cause is found.  The reference's native
    // arithmetic (KIDMP_ARITH_P32N) is.
    if (std::is_same<T, float>::value && arith != KIDMP_ARITH_P32N && !gather_only)
        return fail(ctx, KIDMP_EINVAL, me + ": binary32 fields step in KIDMP_ARITH_P32N only with prognostic aerosols");
    if (w_col_stride != 0 && w_col_stride < int64_t(nz)) return fail(ctx, KIDMP_EINVAL, me + ": w_col_stride must be 0 or >= nz");
    if (ncol == 0) return KIDMP_OK;
    c.dt = dt; c.p0 = p0; c.r_on_cp = r_on_cp; c.rates = rates; c.nstep = nstep;
    c.aer.on = true;
    members<T>(aer, c.aer.state);
    members<T>(aer_adv, c.aer.adv);
    members<T>(aer_div, c.aer.div);
    members<T>(gather_only ? aer : aer_mphys, c.aer.mphys);
    for (int m = 0; m < KID_NA; ++m)
        if (!c.aer.state[m] || !c.aer.mphys[m])
            return fail(ctx, KIDMP_EINVAL, me + ": nc, nwfa and nifa of aer and aer_mphys are required");
    c.aer.w = w; c.aer.w_col_stride = w_col_stride; c.aer.nwfa_src = nwfa_src;
    return kid_device_call<T>(ctx, who, c, work, work_bytes, stream, gather_only);
}

template <class T, class A>
int advect_aero(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, double dt, const A *aer, const T *w, int64_t w_col_stride,
                const T *rho, const T *dz, const A *adv, const A *div, const A *sum, void *stream)
{
    KidMembers<T, KID_NA> f{};
    members<T>(aer, f.state);
    members<T>(adv, f.adv);
    members<T>(div, f.div);
    members<T>(sum, f.sum);
    return kid_advect_members<T, KID_NA>(ctx, who, ncol, nz, dt, f, 0, "", AER_NAMES, w, w_col_stride, rho, dz, nullptr, stream);
}

template <class T, class A>
int advect_slab_aero(kidmp_ctx *ctx, const char *who, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx, const A *aer, const T *u,
                     const T *w, int32_t shared_flow, const T *rho, const T *dz, const A *adv, const A *div, const A *sum, void *stream)
{
    KidMembers<T, KID_NA> f{};
    members<T>(aer, f.state);
    members<T>(adv, f.adv);
    members<T>(div, f.div);
    members<T>(sum, f.sum);
    return kid_advect_slab_members<T, KID_NA>(ctx, who, {nslab, nx, nz, dt, dx, shared_flow}, f, 0, "", AER_NAMES, u, w, rho, dz, nullptr,
                                              stream);
}

template <class T, class A>
int update_aero(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, T dt, const A *aer, const A *t1, const A *t2, const A *t3,
                int32_t clip, void *stream)
{
    KidUpdate<T, KID_NA> f{};
    members<T>(aer, f.state);
    const A *const t[3] = {t1, t2, t3};
    for (int i = 0; i < 3; ++i) {
        T *p[KID_NA];
        members<T>(t[i], p);
        for (int m = 0; m < KID_NA; ++m) f.t[i][m] = p[m];
    }
    return kid_update_members<T, KID_NA>(ctx, who, ncol, nz, dt, f, KID_NA, AER_NAMES, clip ? 7u : 0u, stream);
}
}  // namespace

extern "C" {
int kidmp_kid_interface_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                                    const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                                    const double *exner, const double *dz, const kidmp_kid_fields *mphys, double *ppt,
                                    double *rates, int32_t *nstep, const kidmp_outputs *out,
                                    const kidmp_kid_aerosols *aer, const kidmp_kid_aerosols *aer_adv, const kidmp_kid_aerosols *aer_div,
                                    const kidmp_kid_aerosols *aer_mphys, const double *w, int64_t w_col_stride, const double *nwfa_src,
                                    void *work, size_t work_bytes, void *stream)
{
    return interface_aero<double>(ctx, "kidmp_kid_interface_aero_device", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, ppt,
                                  rates, nstep, out, 0, aer, aer_adv, aer_div, aer_mphys, w, w_col_stride, nwfa_src, work, work_bytes, stream);
}
int kidmp32_kid_interface_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                                      const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                                      const float *exner, const float *dz, const kidmp32_kid_fields *mphys, float *ppt,
                                      double *rates, int32_t *nstep, const kidmp32_outputs *out, int32_t arith,
                                      const kidmp32_kid_aerosols *aer, const kidmp32_kid_aerosols *aer_adv, const kidmp32_kid_aerosols *aer_div,
                                      const kidmp32_kid_aerosols *aer_mphys, const float *w, int64_t w_col_stride, const float *nwfa_src,
                                      void *work, size_t work_bytes, void *stream)
{
    return interface_aero<float>(ctx, "kidmp32_kid_interface_aero_device", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, ppt,
                                 rates, nstep, out, arith, aer, aer_adv, aer_div, aer_mphys, w, w_col_stride, nwfa_src, work, work_bytes, stream);
}
int kidmp_kid_gather_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                                 const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                                 const double *exner, const double *dz, double *ppt,
                                 const kidmp_kid_aerosols *aer, const kidmp_kid_aerosols *aer_adv, const kidmp_kid_aerosols *aer_div,
                                 const double *w, int64_t w_col_stride, void *work, size_t work_bytes, void *stream)
{
    return interface_aero<double, kidmp_kid_fields, kidmp_kid_aerosols, kidmp_outputs>(
        ctx, "kidmp_kid_gather_aero_device", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, nullptr, ppt, nullptr, nullptr, nullptr, 0,
        aer, aer_adv, aer_div, nullptr, w, w_col_stride, nullptr, work, work_bytes, stream, true);
}
int kidmp32_kid_gather_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                                   const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                                   const float *exner, const float *dz, float *ppt,
                                   const kidmp32_kid_aerosols *aer, const kidmp32_kid_aerosols *aer_adv, const kidmp32_kid_aerosols *aer_div,
                                   const float *w, int64_t w_col_stride, void *work, size_t work_bytes, void *stream)
{
    return interface_aero<float, kidmp32_kid_fields, kidmp32_kid_aerosols, kidmp32_outputs>(
        ctx, "kidmp32_kid_gather_aero_device", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, nullptr, ppt, nullptr, nullptr, nullptr,
        KIDMP_ARITH_P32N, aer, aer_adv, aer_div, nullptr, w, w_col_stride, nullptr, work, work_bytes, stream, true);
}

int kidmp_kid_advect_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_aerosols *aer,
                                 const double *w, int64_t w_col_stride, const double *rho, const double *dz,
                                 const kidmp_kid_aerosols *adv, const kidmp_kid_aerosols *div, const kidmp_kid_aerosols *sum, void *stream)
{
    return advect_aero<double>(ctx, "kidmp_kid_advect_aero_device", ncol, nz, dt, aer, w, w_col_stride, rho, dz, adv, div, sum, stream);
}
int kidmp32_kid_advect_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp32_kid_aerosols *aer,
                                   const float *w, int64_t w_col_stride, const float *rho, const float *dz,
                                   const kidmp32_kid_aerosols *adv, const kidmp32_kid_aerosols *div, const kidmp32_kid_aerosols *sum,
                                   void *stream)
{
    return advect_aero<float>(ctx, "kidmp32_kid_advect_aero_device", ncol, nz, dt, aer, w, w_col_stride, rho, dz, adv, div, sum, stream);
}
int kidmp_kid_advect_slab_aero_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
                                      const kidmp_kid_aerosols *aer, const double *u, const double *w, int32_t shared_flow,
                                      const double *rho, const double *dz, const kidmp_kid_aerosols *adv, const kidmp_kid_aerosols *div,
                                      const kidmp_kid_aerosols *sum, void *stream)
{
    return advect_slab_aero<double>(ctx, "kidmp_kid_advect_slab_aero_device", nslab, nx, nz, dt, dx, aer, u, w, shared_flow, rho, dz, adv, div,
                                    sum, stream);
}
int kidmp32_kid_advect_slab_aero_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
                                        const kidmp32_kid_aerosols *aer, const float *u, const float *w, int32_t shared_flow,
                                        const float *rho, const float *dz, const kidmp32_kid_aerosols *adv, const kidmp32_kid_aerosols *div,
                                        const kidmp32_kid_aerosols *sum, void *stream)
{
    return advect_slab_aero<float>(ctx, "kidmp32_kid_advect_slab_aero_device", nslab, nx, nz, dt, dx, aer, u, w, shared_flow, rho, dz, adv, div,
                                   sum, stream);
}
int kidmp_kid_update_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_aerosols *aer,
                                 const kidmp_kid_aerosols *t1, const kidmp_kid_aerosols *t2, const kidmp_kid_aerosols *t3, int32_t clip,
                                 void *stream)
{
    return update_aero<double>(ctx, "kidmp_kid_update_aero_device", ncol, nz, dt, aer, t1, t2, t3, clip, stream);
}
int kidmp32_kid_update_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, const kidmp32_kid_aerosols *aer,
                                   const kidmp32_kid_aerosols *t1, const kidmp32_kid_aerosols *t2, const kidmp32_kid_aerosols *t3,
                                   int32_t clip, void *stream)
{
    return update_aero<float>(ctx, "kidmp32_kid_update_aero_device", ncol, nz, dt, aer, t1, t2, t3, clip, stream);
}
}  // extern "C"
