// kidmp_ctx.h -- internal to the units behind include/kidmp.h (not installed): the context, the error and device-guard
// helpers of every entry point, and what the units kidmp_{capi,diag,host,tables,multi,adapter,stats,summary,fall,doppler,kinematic,slab,
// spectra,dspectrum,aerosol,lidar,brightband,mie,radiometer,multichannel,polarimetric,scan,specproc,mathprobe}.hip offer one another.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/kidmp.h"
#include "thompson_column.h"
#include "thompson_reflectivity.h"
#include "thompson_tables.h"
#include "kidmp_stage_plan.h"

namespace kidmp {
constexpr int HOST_NBUF = 3;                         // staging sets of the host pipeline
constexpr int RED_CHUNKS = 128;                      // column chunks of kidmp_reduce_rates_device
constexpr int ACC_LIMBS = 6, ACC_N = 4 * ACC_LIMBS;  // k_ppt_exact: six 64-bit limbs per species
static_assert(ACC_N == KIDMP_PPT_LIMBS, "include/kidmp.h");
// k_sanity: maxima of qc, qr, nr, qs, qi, qg, ni, then the numbers of negative entries of those and of qv
constexpr int SANITY_MAX = 7, SANITY_NEG = 8, SANITY_N = SANITY_MAX + SANITY_NEG;
}

struct kidmp_ctx {
    kidmp_cfg cfg{};
    kidmp::Consts hc{};
    kidmp::Bins hb{};
    kidmp::Consts *d_consts = nullptr;
    kidmp::Bins *d_bins = nullptr;
    kidmp::Tables tables{};
    bool ready = false;
    double init_s = 0.;
    std::string err;
    // staging for the host-array entries: a ring of HOST_NBUF column chunks in HBM, one stream per direction and
    // one for the kernel, so that the upload of chunk i+1, the step of chunk i and the download of chunk i-1 overlap
    double *d_stage = nullptr;
    size_t stage_bytes = 0;
    hipStream_t stream = nullptr;                    // the context's compute stream
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_up[kidmp::HOST_NBUF] = {}, ev_step[kidmp::HOST_NBUF] = {}, ev_down[kidmp::HOST_NBUF] = {};
    int64_t host_chunk = 0;                          // columns per chunk; 0 = chosen per call (kidmp_set_host_chunk)
    int debug_stop = 0;
    int cslot = -1;
    // partial sums of kidmp_reduce_rates_device, accumulators of kidmp_sanity_device
    double *d_red = nullptr;
    size_t red_elems = 0;
    unsigned long long *d_sanity = nullptr;
    // exact (fixed-point) domain sums of the surface precipitation: KIDMP_PPT_LIMBS 64-bit accumulators
    unsigned long long *d_acc = nullptr;
    std::string fingerprint;
    // kidmp_set_column_nc: the bound per-column set_Nc (cm**-3, binary64) in HBM, owned by the context; null = unbound
    double *d_nc_col = nullptr;
    int64_t nc_count = 0;
    // kidmp_set_advection (include/kidmp_advection.h): the scheme an advection entry reads when it is called
    int32_t advection = 0;                           // KIDMP_ADVECT_VANLEER
};

namespace kidmp {
// ONE object for all units: kidmp_last_error(NULL) reads the failures that have no context (defined in kidmp_capi.hip)
extern thread_local std::string g_err;

template <class C> int fail(C *c, int code, const std::string &msg)   // C: kidmp_ctx or kidmp_multi
{
    if (c) c->err = msg;
    g_err = msg;
    return code;
}
inline int fail(std::nullptr_t, int code, const std::string &msg) { return fail((kidmp_ctx *)nullptr, code, msg); }
inline int hipfail(kidmp_ctx *c, hipError_t e, const char *what) { return fail(c, KIDMP_EHIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define HIPTRY(c, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hipfail((c), e_, #x); } while (0)

// `also`: what else the entry needs before anything is touched (a name, a directory); it fails with the same message
inline int require_ready(kidmp_ctx *c, const char *msg = "kidmp: context not initialised", bool also = true)
{ return c && c->ready && also ? KIDMP_OK : fail(c, KIDMP_ESTATE, msg); }
inline bool valid_arith(int32_t arith) { return arith == KIDMP_ARITH_P32N || arith == KIDMP_ARITH_F32; }
constexpr char BAD_ARITH[] = "kidmp32: arith must be KIDMP_ARITH_P32N or KIDMP_ARITH_F32";

// Every entry point that touches the device runs with the context's device current and puts the caller's
// device back on exit: the caller (torch, a Fortran host driving several GPUs) may have another one selected,
// and hipMalloc / kernel launches / the __constant__ slot all bind to the current device.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete; DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define GUARD(c) DeviceGuard guard_((c)->cfg.device); if (guard_.err != hipSuccess) return hipfail((c), guard_.err, "hipSetDevice")

// A device pointer handed to a device entry must live on the context's GPU: a buffer of another GPU would be
// reached through peer access at best and fault at worst.
inline int check_on_device(kidmp_ctx *c, const void *p, const char *what)
{
    if (!p) return KIDMP_OK;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return KIDMP_OK; }   // unregistered: let the launch decide
    if (at.type == hipMemoryTypeDevice && at.device != c->cfg.device)
        return fail(c, KIDMP_EINVAL, std::string("kidmp: ") + what + " lives on device " + std::to_string(at.device)
                                     + ", the context is bound to device " + std::to_string(c->cfg.device));
    return KIDMP_OK;
}

// Stricter: the entries of the column diagnostics refuse anything but device memory of the context's GPU (a pageable
// host array would otherwise reach the kernel and fault it).
inline int check_device_array(kidmp_ctx *c, const char *who, const void *p, const char *what)
{
    if (!p) return KIDMP_OK;
    hipPointerAttribute_t at;
    const bool known = hipPointerGetAttributes(&at, p) == hipSuccess;
    if (!known) (void)hipGetLastError();
    if (!known || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged))
        return fail(c, KIDMP_EINVAL, std::string(who) + ": " + what + " is not device memory");
    if (at.device != c->cfg.device)
        return fail(c, KIDMP_EINVAL, std::string(who) + ": " + what + " lives on device " + std::to_string(at.device)
                                     + ", the context is bound to device " + std::to_string(c->cfg.device));
    return KIDMP_OK;
}

inline int check_step_args(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const void *const *ptrs, int nptr)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, "kidmp: ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, "kidmp: nz outside [2, KIDMP_MAX_NZ]");
    if (!(dt > 0.)) return fail(ctx, KIDMP_EINVAL, "kidmp: dt must be > 0");
    for (int i = 0; i < nptr && ncol > 0; ++i)                 // an empty batch has nothing to point at
        if (!ptrs[i]) return fail(ctx, KIDMP_EINVAL, "kidmp: null array argument");
    return KIDMP_OK;
}

// While a per-column droplet number is bound (kidmp_set_column_nc) a batch must be exactly the bound columns.
inline int check_nc_count(kidmp_ctx *c, const char *who, int64_t ncol)
{
    if (!c || !c->d_nc_col || ncol == c->nc_count) return KIDMP_OK;
    return fail(c, KIDMP_EINVAL, std::string(who) + ": ncol = " + std::to_string(ncol) + ", but kidmp_set_column_nc bound " +
                                 std::to_string(c->nc_count) + " columns");
}
// the entries that take n elements and no nz: n must be whole columns of the binding; nz_col = 0 without a binding
inline int nc_levels_of(kidmp_ctx *c, const char *who, int64_t n, int64_t &nz_col)
{
    nz_col = 0;
    if (!c || !c->d_nc_col || n <= 0) return KIDMP_OK;
    if (n % c->nc_count != 0)
        return fail(c, KIDMP_EINVAL, std::string(who) + ": n = " + std::to_string(n) + " is not a multiple of the " +
                                     std::to_string(c->nc_count) + " columns kidmp_set_column_nc bound");
    nz_col = n / c->nc_count;
    return KIDMP_OK;
}

// kidmp_capi.hip: the one body of the step's device entries (R = double: p64; float: `arith` selects p32n or f32), which
// also steps every chunk of the host pipeline; io = qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t
template <class R>
int step_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, R dt, R *const *io, const R *p, const R *w, const R *dz,
                R *ppt, double *rates, int32_t *nstep, int32_t arith, void *stream, int64_t nc_first = -1);
// nc_first: with a per-column droplet number bound, -1 = the batch is the whole binding (ncol is checked against it);
// >= 0 = a chunk of the host pipeline (which made that check) whose first column is nc_first
int check_refl_args(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const void *const *req, int nreq, const void *qs, const void *qg);

// kidmp_diag.hip.  The two void ones only launch: the caller asks hipGetLastError().  v = qc, qr, nr, qs, qi, qg, ni, qv
// set_nc_col (null: Nt_c everywhere): per-column set_Nc in cm**-3, element i belonging to column (e0 + i) / nz_col
template <class T> void launch_default_aerosols(int64_t n, T Nt_c, const T *qv, const T *t, const T *p, T *nc, T *nwfa, T *nifa, hipStream_t s,
                                                const double *set_nc_col = nullptr, int64_t nz_col = 1, int64_t e0 = 0);
void launch_sanity(int64_t n, const double *const (&v)[SANITY_NEG], unsigned long long *acc, hipStream_t s);
template <class T> hipError_t launch_ppt_exact(int64_t ncol, const T *ppt, unsigned long long *acc, hipStream_t s);
// the column outputs (dbz, re_qc, re_qi, re_qs; preset form): the checks every entry shares, then ONE launch picked from
// what `out` asks for -- k_reflectivity, k_effective_radii or k_column_outputs
template <class T> int check_outputs_request(kidmp_ctx *ctx, const char *who, const ColumnOutputs<T> &out);   // `out` alone
template <class T>
int check_outputs_args(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const ColumnState<T> &in, const ColumnOutputs<T> &out);
template <class T>
hipError_t launch_outputs(kidmp_ctx *ctx, int64_t ncol, int nz, const ColumnState<T> &in, const ColumnOutputs<T> &out, hipStream_t s,
                          int64_t nc_first = 0);   // first column of the batch within a bound per-column droplet number
// calc_effectRad in its INOUT (keep) form on n elements, with the optional arrays of the lenient entries
template <class T>
int check_radii_args(kidmp_ctx *ctx, const char *who, int64_t n, const T *t, const T *p, const T *qv, const T *qc, const T *nc,
                     const T *qi, const T *ni, const T *qs, T *re_qc, T *re_qi, T *re_qs);
template <class T>
hipError_t launch_radii_keep(kidmp_ctx *ctx, int64_t n, const T *t, const T *p, const T *qv, const T *qc, const T *nc,
                             const T *qi, const T *ni, const T *qs, T *re_qc, T *re_qi, T *re_qs, hipStream_t s,
                             int64_t nz_col = 0, int64_t e0 = 0);   // nc_levels_of; e0: the first element's index in the binding

// kidmp_host.hip: the columns per chunk of a host-array entry, and the context's staging memory (it only grows)
int64_t pick_host_chunk(const kidmp_ctx *ctx, int64_t ncol);
int ensure_stage(kidmp_ctx *ctx, size_t need);
// kidmp_host.hip: the one body of the diagnostics' host-array entries (kidmp_stage_plan.h).  stage_open makes the plan's
// staging memory and hands every present array its slot (StageArray::dev); stage_run moves the chunks through it.
int stage_open(kidmp_ctx *ctx, const StagePlan &plan);
int stage_run(kidmp_ctx *ctx, const StagePlan &plan, const std::function<hipError_t(int64_t c0, int64_t n)> &enqueue);
// kidmp_host.hip.  What an entry may ask of the pipeline beyond the step: the exact precipitation sums and the sanity
// scan (left in ctx->d_acc / d_sanity), and the column outputs (host arrays) of every chunk's post-step state.
template <class T> struct PipelineExtras { bool exact_sums = false, scan_sanity = false; ColumnOutputs<T> out{}; };
template <class T>
int host_pipeline(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, T *const *io, const T *const *in, T *ppt,
                  double *rates, int32_t *nstep, int32_t arith, const PipelineExtras<T> &extra = {});

// kidmp_adapter.hip: the KiD adapter (W:28-310).  Members in the order of kidmp_kid_fields; WORK_OF[m] is the profile of
// the workspace (0..11 the order of mp_thompson's dummies, 12 p, 13 w, 14 dz) that member m is gathered into.
constexpr int KID_NF = 9, KID_NWARM = 5, KID_NWORK = 15;                 // theta, qv, qc, qr, nr | qi, ni, qs, qg
constexpr int KID_WORK_OF[KID_NF] = {11, 0, 1, 3, 7, 2, 6, 4, 5};
template <class T> struct KidFields { T *f[KID_NF]; };
// the aerosol-aware call of include/kidmp_aerosol.h: nc, nwfa, nifa are gathered into profiles KID_AER_WORK0 .. + 2 and
// backed out like the other moments, w goes to profile 13; on == false: the U2 defaults and w = 0
constexpr int KID_NA = 3, KID_AER_WORK0 = 8;
template <class T> struct KidAerosols {
    bool on;
    T *state[KID_NA], *adv[KID_NA], *div[KID_NA], *mphys[KID_NA];   // a null member of adv / div is a zero operand
    const T *w; int64_t w_col_stride;                // cell-centre updraft [ncol][nz] (stride 0: one profile), null: zeros
    const T *nwfa_src;                               // [ncol], null: no surface source (M:1001)
};
template <class T> struct KidCall {
    int64_t ncol; int32_t nz; T dt, p0, r_on_cp;
    KidFields<T> state, adv, div, mphys;             // a null member of adv / div is a zero operand
    const T *exner, *dz;
    T *ppt; double *rates; int32_t *nstep; ColumnOutputs<T> out;
    int32_t arith;
    KidAerosols<T> aer;
};
inline size_t kid_stride(int64_t ncol, int32_t nz, size_t elem)      // bytes from one workspace profile to the next; 0: bad arguments
{ return ncol < 0 || nz < 1 || nz > KIDMP_MAX_NZ ? 0 : (size_t(ncol) * size_t(nz) * elem + 255) / 256 * 256; }
// what the device and the host entries check alike, before anything is written; F = kidmp_kid_fields / kidmp32_kid_fields
template <class T, class F>
int kid_check(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, double dt, const F *state, const F *adv, const F *div,
              const T *exner, const T *dz, const F *mphys, T *ppt, const ColumnOutputs<T> &out, int32_t arith, KidCall<T> &call);
// gather (gather_only: that alone), step, outputs, back-out on `s`, nothing else: `c` holds device pointers; nc_first as for step_device
template <class T> int kid_enqueue(kidmp_ctx *ctx, const KidCall<T> &c, void *work, hipStream_t s, int64_t nc_first, bool gather_only = false);
// what a device entry does once kid_check has passed and `c` is filled: the workspace and device checks, then kid_enqueue
template <class T>
int kid_device_call(kidmp_ctx *ctx, const char *who, const KidCall<T> &c, void *work, size_t work_bytes, void *stream, bool gather_only);
// kidmp_host.hip
template <class T> int kid_host(kidmp_ctx *ctx, const KidCall<T> &host);

// kidmp_kinematic.hip / kidmp_slab.hip: the bodies of the advection and update entries for N members (N = KID_NF behind
// kidmp_kinematic.h and kidmp_slab.h, KID_NA behind kidmp_aerosol.h), one launch each.  The first `nreq` members of
// `state` are required (`required` is what the refusal says); `names` are the members' names in messages.
template <class T, int N> struct KidMembers { T *state[N], *adv[N], *div[N], *sum[N]; };
template <class T, int N>
int kid_advect_members(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, double dt, const KidMembers<T, N> &f, int nreq,
                       const char *required, const char *const *names, const T *w, int64_t w_col_stride, const T *rho, const T *dz,
                       T *courant, void *stream);
struct KidSlabShape { int64_t nslab; int32_t nx, nz; double dt, dx; int32_t shared_flow; };
template <class T, int N>
int kid_advect_slab_members(kidmp_ctx *ctx, const char *who, const KidSlabShape &g, const KidMembers<T, N> &f, int nreq,
                            const char *required, const char *const *names, const T *u, const T *w, const T *rho, const T *dz,
                            T *courant, void *stream);
// state <- state + ((t[0] + t[1]) + t[2])*dt; bit m of clip_mask: member m becomes max(X, +0.0); nloop <= N members are walked
template <class T, int N> struct KidUpdate { T *state[N]; const T *t[3][N]; };
template <class T, int N>
int kid_update_members(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, T dt, const KidUpdate<T, N> &f, int nloop,
                       const char *const *names, uint32_t clip_mask, void *stream);
}  // namespace kidmp
