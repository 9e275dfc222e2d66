// kidmp_capi.hip -- the C ABI of include/kidmp.h over the gfx950 kernels.
// Host-side mirror of the reference's thompson_init / mp_thompson pair
// (M:374, M:1156) plus the batched form of the KiD adapter loop (W:54-246).
// This unit: the context's lifecycle, the getters and the device entries.
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <new>

#include "kidmp_ctx.h"
#include "thompson_host_init.h"

using namespace kidmp;
thread_local std::string kidmp::g_err;

namespace {
std::mutex g_slot_mu;
bool g_slot_used[MAX_CONST_SLOTS] = {};

int take_slot()
{
    std::lock_guard<std::mutex> g(g_slot_mu);
    for (int i = 0; i < MAX_CONST_SLOTS; ++i)
        if (!g_slot_used[i]) { g_slot_used[i] = true; return i; }
    return -1;
}
void give_slot(int i)
{
    std::lock_guard<std::mutex> g(g_slot_mu);
    if (i >= 0 && i < MAX_CONST_SLOTS) g_slot_used[i] = false;
}

template <class T>
int refl_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const T *t, const T *p, const T *qv, const T *qr, const T *nr,
                const T *qs, const T *qg, T *dbz, void *stream)
{
    const void *req[] = {t, p, qv, qr, nr, dbz};
    if (int rc = check_refl_args(ctx, ncol, nz, req, 6, qs, qg)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const char *names[] = {"t", "p", "qv", "qr", "nr", "qs", "qg", "dbz"};
    const void *ptrs[] = {t, p, qv, qr, nr, qs, qg, dbz};
    for (int i = 0; i < 8; ++i)
        if (int rc = check_device_array(ctx, "kidmp_reflectivity", ptrs[i], names[i])) return rc;
    HIPTRY(ctx, launch_reflectivity<T>(refl_consts(ctx->hc), ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, (hipStream_t)stream));
    return KIDMP_OK;
}
}  // namespace

template <class R>
int kidmp::step_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, R dt, R *const *io, const R *p, const R *w, const R *dz,
                       R *ppt, double *rates, int32_t *nstep, int32_t arith, void *stream, int64_t nc_first)
{
    // w1d only feeds activ_ncloud (is_aerosol_aware, M:2797): optional otherwise
    const void *ptrs[] = {io[0], io[1], io[2], io[3], io[4], io[5], io[6], io[7], io[8], io[9], io[10], io[11], p, dz, ppt};
    if (int rc = check_step_args(ctx, ncol, nz, double(dt), ptrs, 15)) return rc;
    if (ctx->cfg.is_aerosol_aware && !w) return fail(ctx, KIDMP_EINVAL, "kidmp: an aerosol-aware context needs the updraft profile w");
    if (std::is_same<R, float>::value && !valid_arith(arith)) return fail(ctx, KIDMP_EINVAL, BAD_ARITH);
    if (nc_first < 0) if (int rc = check_nc_count(ctx, "kidmp_batch_step", ncol)) return rc;
    GUARD(ctx);
    if (int rc = check_on_device(ctx, io[0], "qv")) return rc;
    if (int rc = check_on_device(ctx, ppt, "ppt")) return rc;
    if (ncol == 0) return KIDMP_OK;
    StepArgsT<R> a{};
    a.qv = io[0]; a.qc = io[1]; a.qi = io[2]; a.qr = io[3]; a.qs = io[4]; a.qg = io[5]; a.ni = io[6]; a.nr = io[7];
    a.nc = io[8]; a.nwfa = io[9]; a.nifa = io[10]; a.t = io[11]; a.p = p; a.dz = dz; a.w = w;
    a.ppt = ppt; a.rates = rates; a.nstep = nstep; a.ncol = ncol; a.nz = nz; a.dt = dt;
    a.cslot = ctx->cslot; a.tables = ctx->tables; a.iiwarm = ctx->cfg.iiwarm != 0; a.aero = ctx->cfg.is_aerosol_aware != 0;
    a.debug_stop = ctx->debug_stop;
    a.set_nc_col = ctx->d_nc_col ? ctx->d_nc_col + (nc_first > 0 ? nc_first : 0) : nullptr;
    if constexpr (std::is_same<R, double>::value) HIPTRY(ctx, p64::launch_column_step(a, (hipStream_t)stream));
    else if (arith == KIDMP_ARITH_P32N)           HIPTRY(ctx, p32n::launch_column_step(a, (hipStream_t)stream));
    else                                          HIPTRY(ctx, f32::launch_column_step(a, (hipStream_t)stream));
    return KIDMP_OK;
}
template int kidmp::step_device<double>(kidmp_ctx *, int64_t, int32_t, double, double *const *, const double *, const double *,
                                        const double *, double *, double *, int32_t *, int32_t, void *, int64_t);
template int kidmp::step_device<float>(kidmp_ctx *, int64_t, int32_t, float, float *const *, const float *, const float *,
                                       const float *, float *, double *, int32_t *, int32_t, void *, int64_t);

// ---- calc_refl10cm entries (M:4946-5244) ----
// arguments common to the four entries; qs/qg: both or neither, neither only in an iiwarm context (a warm run keeps them 0)
int kidmp::check_refl_args(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const void *const *req, int nreq, const void *qs, const void *qg)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, "kidmp_reflectivity: ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, "kidmp_reflectivity: nz outside [2, KIDMP_MAX_NZ]");
    for (int i = 0; i < nreq; ++i)
        if (!req[i]) return fail(ctx, KIDMP_EINVAL, "kidmp_reflectivity: null array argument");
    if ((qs == nullptr) != (qg == nullptr)) return fail(ctx, KIDMP_EINVAL, "kidmp_reflectivity: qs and qg must be given or left out together");
    if (!qs && !ctx->cfg.iiwarm) return fail(ctx, KIDMP_EINVAL, "kidmp_reflectivity: a mixed-phase context needs qs and qg");
    if (!refl_consts_supported(ctx->hc)) return fail(ctx, KIDMP_ESTATE, "kidmp_reflectivity: exponents differ from the kernel's");
    return KIDMP_OK;
}

extern "C" {
int kidmp_init(const kidmp_cfg *cfg, kidmp_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, KIDMP_EINVAL, "kidmp_init: null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, KIDMP_ENODEV, "kidmp_init: no HIP device visible (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, KIDMP_ENODEV, "kidmp_init: bad device ordinal");
    if (!(cfg->set_Nc > 0.)) return fail(nullptr, KIDMP_EINVAL, "kidmp_init: set_Nc must be > 0");
    kidmp_ctx *c = new (std::nothrow) kidmp_ctx;
    if (!c) return fail(nullptr, KIDMP_ENOMEM, "kidmp_init: out of host memory");
    c->cfg = *cfg;
#ifdef KIDMP_PROFILING
    if (const char *e = getenv("KIDMP_DEBUG_STOP")) c->debug_stop = atoi(e);   // libkidmp_prof.so only: truncates the step
#endif
    const auto t0 = std::chrono::steady_clock::now();
    auto bail = [&](int code, const std::string &why) { kidmp_finalize(c); g_err = why; return code; };
    DeviceGuard guard_(cfg->device);                 // the caller's current device is restored on every exit path
    if (guard_.err != hipSuccess) return bail(KIDMP_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && !strstr(prop.gcnArchName, "gfx950"))
        return bail(KIDMP_ENODEV, std::string("kidmp_init: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    host_init(cfg->iiwarm ? 1 : 0, cfg->l_sediment ? 1 : 0, cfg->set_Nc, c->hc, c->hb);
    if (!generated_consts_match(c->hc))
        return bail(KIDMP_ESTATE, "kidmp_init: thompson_consts_gen.h is stale (rebuild: make -C kid_amd/csrc clean all)");
    hipError_t e;
#define INITTRY(x) do { e = (x); if (e != hipSuccess) return bail(KIDMP_EHIP, std::string(#x ": ") + hipGetErrorString(e)); } while (0)
    INITTRY(hipStreamCreate(&c->stream));
    INITTRY(hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking));
    INITTRY(hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking));
    for (int b = 0; b < HOST_NBUF; ++b) {
        INITTRY(hipEventCreateWithFlags(&c->ev_up[b], hipEventDisableTiming));
        INITTRY(hipEventCreateWithFlags(&c->ev_step[b], hipEventDisableTiming));
        INITTRY(hipEventCreateWithFlags(&c->ev_down[b], hipEventDisableTiming));
    }
    // scratch of the diagnostics entries, sized for KIDMP_MAX_NZ once: no entry allocates after kidmp_init
    c->red_elems = size_t(RED_CHUNKS) * size_t(KIDMP_NRATES) * size_t(KIDMP_MAX_NZ);
    INITTRY(hipMalloc((void **)&c->d_red, c->red_elems * sizeof(double)));
    INITTRY(hipMalloc((void **)&c->d_sanity, SANITY_N * sizeof(unsigned long long)));
    INITTRY(hipMalloc((void **)&c->d_acc, ACC_N * sizeof(unsigned long long)));
    INITTRY(hipMalloc((void **)&c->d_consts, sizeof(Consts)));
    INITTRY(hipMalloc((void **)&c->d_bins, sizeof(Bins)));
    INITTRY(hipMemcpy(c->d_consts, &c->hc, sizeof(Consts), hipMemcpyHostToDevice));
    INITTRY(hipMemcpy(c->d_bins, &c->hb, sizeof(Bins), hipMemcpyHostToDevice));
    c->cslot = take_slot();
    if (c->cslot < 0) return bail(KIDMP_ESTATE, "kidmp_init: more than " + std::to_string(MAX_CONST_SLOTS) + " live contexts in this process");
    INITTRY(p64::upload_consts(c->cslot, c->hc));       // one constant-memory image per arithmetic variant
    INITTRY(p32n::upload_consts(c->cslot, c->hc));
    INITTRY(f32::upload_consts(c->cslot, c->hc));
    INITTRY(alloc_tables(c->tables));
    INITTRY(build_tables(c->d_consts, c->d_bins, c->hc.iiwarm, c->tables, c->stream));
#undef INITTRY
    c->init_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->ready = true;
    *out = c;
    return KIDMP_OK;
}

void kidmp_finalize(kidmp_ctx *c)
{
    if (!c) return;
    DeviceGuard guard_(c->cfg.device);
    free_tables(c->tables);
    for (void *p : {(void *)c->d_consts, (void *)c->d_bins, (void *)c->d_stage, (void *)c->d_red, (void *)c->d_sanity, (void *)c->d_acc, (void *)c->d_nc_col})
        if (p) (void)hipFree(p);
    for (hipStream_t s : {c->stream, c->s_h2d, c->s_d2h})
        if (s) (void)hipStreamDestroy(s);
    for (int b = 0; b < HOST_NBUF; ++b)
        for (hipEvent_t e : {c->ev_up[b], c->ev_step[b], c->ev_down[b]})
            if (e) (void)hipEventDestroy(e);
    give_slot(c->cslot);
    delete c;
}

const char *kidmp_last_error(const kidmp_ctx *c) { return c && !c->err.empty() ? c->err.c_str() : g_err.c_str(); }
double kidmp_init_seconds(const kidmp_ctx *c) { return c ? c->init_s : 0.; }
const char *kidmp_kernel_name(void) { return column_kernel_name(); }

int kidmp_batch_step_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                            double *qv, double *qc, double *qi, double *qr, double *qs, double *qg,
                            double *ni, double *nr, double *nc, double *nwfa, double *nifa, double *t,
                            const double *p, const double *w, const double *dz,
                            double *ppt, double *rates, int32_t *nstep, void *stream)
{
    double *const io[12] = {qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t};
    return step_device<double>(ctx, ncol, nz, dt, io, p, w, dz, ppt, rates, nstep, 0, stream);
}
// binary32 state: the reference as shipped (P32n) and the all-binary32 build
int kidmp32_batch_step_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                              float *qv, float *qc, float *qi, float *qr, float *qs, float *qg,
                              float *ni, float *nr, float *nc, float *nwfa, float *nifa, float *t,
                              const float *p, const float *w, const float *dz,
                              float *ppt, double *rates, int32_t *nstep, int32_t arith, void *stream)
{
    float *const io[12] = {qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t};
    return step_device<float>(ctx, ncol, nz, dt, io, p, w, dz, ppt, rates, nstep, arith, stream);
}

int kidmp_reflectivity_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p,
                              const double *qv, const double *qr, const double *nr, const double *qs, const double *qg,
                              double *dbz, void *stream)
{
    return refl_device<double>(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, stream);
}
int kidmp32_reflectivity_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p,
                                const float *qv, const float *qr, const float *nr, const float *qs, const float *qg,
                                float *dbz, void *stream)
{
    return refl_device<float>(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz, stream);
}

// ---- a droplet number per column (set_Nc, namelists M:22; Nt_c = set_Nc*1.e6, M:381) ----
int kidmp_set_column_nc(kidmp_ctx *ctx, int64_t ncol, const double *set_nc)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, "kidmp_set_column_nc: ncol < 0");
    if (ctx->cfg.is_aerosol_aware)
        return fail(ctx, KIDMP_EINVAL, "kidmp_set_column_nc: the context is aerosol-aware (the droplet number is prognostic there)");
    if (ncol > int64_t(0x7fffffff)) return fail(ctx, KIDMP_EINVAL, "kidmp_set_column_nc: more columns than one launch takes");
    GUARD(ctx);
    if (ncol == 0 || !set_nc) {                              // unbind
        if (ctx->d_nc_col) HIPTRY(ctx, hipFree(ctx->d_nc_col));   // (waits for the work that reads it)
        ctx->d_nc_col = nullptr;
        ctx->nc_count = 0;
        return KIDMP_OK;
    }
    if (int rc = check_on_device(ctx, set_nc, "set_nc")) return rc;
    std::vector<double> h;
    try { h.resize(size_t(ncol)); } catch (const std::exception &) { return fail(ctx, KIDMP_ENOMEM, "kidmp_set_column_nc: out of host memory"); }
    HIPTRY(ctx, hipMemcpy(h.data(), set_nc, size_t(ncol) * sizeof(double), hipMemcpyDefault));
    for (int64_t i = 0; i < ncol; ++i)                       // what kidmp_init demands of cfg->set_Nc, and finite
        if (!(h[size_t(i)] > 0.) || !(h[size_t(i)] <= 1.7976931348623157e308))
            return fail(ctx, KIDMP_EINVAL, "kidmp_set_column_nc: set_nc of column " + std::to_string(i) + " is not a finite number > 0");
    double *d = nullptr;
    HIPTRY(ctx, hipMalloc((void **)&d, size_t(ncol) * sizeof(double)));
    const hipError_t e = hipMemcpy(d, h.data(), size_t(ncol) * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hipfail(ctx, e, "hipMemcpy(set_nc)"); }
    if (ctx->d_nc_col) (void)hipFree(ctx->d_nc_col);
    ctx->d_nc_col = d;
    ctx->nc_count = ncol;
    return KIDMP_OK;
}
int64_t kidmp_column_nc_count(const kidmp_ctx *ctx) { return ctx && ctx->ready && ctx->d_nc_col ? ctx->nc_count : 0; }

const char *kidmp_kernel_fingerprint(kidmp_ctx *ctx)
{
    if (!ctx || !ctx->ready) return "";
    DeviceGuard guard_(ctx->cfg.device);
    ctx->fingerprint = p64::column_kernel_fingerprint(ctx->cfg.iiwarm != 0);
    return ctx->fingerprint.c_str();
}
const char *kidmp32_kernel_fingerprint(kidmp_ctx *ctx, int32_t arith)
{
    if (!ctx || !ctx->ready || !valid_arith(arith)) return "";
    DeviceGuard guard_(ctx->cfg.device);
    ctx->fingerprint = arith == KIDMP_ARITH_P32N ? p32n::column_kernel_fingerprint(ctx->cfg.iiwarm != 0)
                                                 : f32::column_kernel_fingerprint(ctx->cfg.iiwarm != 0);
    return ctx->fingerprint.c_str();
}

/* deprecated: device memory is no longer reserved per batch (launches own no per-batch memory since round 2); kept so that
 * hosts linked against earlier builds keep linking.  Checks its arguments and does nothing. */
int kidmp_reserve(kidmp_ctx *ctx, int64_t ncol, int32_t nz)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0 || nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, "kidmp_reserve: bad ncol / nz");
    return KIDMP_OK;
}
}  // extern "C"
