// kidmp_multichannel.hip -- the entries of include/kidmp_multichannel.h: a set of existing radiometer or cloud-radar tables
// checked on the host (same context, same grids, the wavelength-independent rows equal bit for bit) and run in one launch
// of k_radiometer_multi or k_mie_radar_multi (thompson_reflectivity.hip), over device arrays or over host arrays in chunks
// through the context's staging memory.  No kernel of its own.
#include <cstddef>
#include <cstring>

#include "kidmp_channel_call.h"
#include "../../include/kidmp_multichannel.h"

using namespace kidmp;

static_assert(MC_MAX_CHANNELS == KIDMP_MAX_CHANNELS, "include/kidmp_multichannel.h");

namespace {
constexpr size_t STAGE_LIMIT = size_t(1) << 30;          // the host entries' staging: chunks are sized to stay below it

// the rows of a table that do not depend on the wavelength, by the table's kind
constexpr int RAD_SHARED[] = {2}, MIE_SHARED[] = {1, 3, 4};

// What makes nch tables one channel set.  The grids and the shared rows are compared on the host copies the tables hold.
template <class Tab, size_t NS>
int check_set(kidmp_ctx *ctx, const std::string &w, const Tab *const *tables, int32_t nch, const int (&shared)[NS])
{
    if (nch < 1 || nch > KIDMP_MAX_CHANNELS) return fail(ctx, KIDMP_EINVAL, w + ": nch outside [1, KIDMP_MAX_CHANNELS]");
    if (!tables) return fail(ctx, KIDMP_EINVAL, w + ": tables is NULL");
    for (int c = 0; c < nch; ++c)
        if (!tables[c] || tables[c]->ctx != ctx) return fail(ctx, KIDMP_EINVAL, w + ": a table is NULL or belongs to another context");
    const MieTableData &f = *tables[0];
    for (int c = 1; c < nch; ++c) {
        const MieTableData &t = *tables[c];
        for (int x = 0; x < MIE_NSPEC; ++x) {
            if (t.nb[x] != f.nb[x]) return fail(ctx, KIDMP_EINVAL, w + ": the tables' grids differ in nb");
            const size_t nb = size_t(f.nb[x]);
            const double *a = f.h_buf + f.off[x], *b = t.h_buf + t.off[x];
            if (std::memcmp(a, b, 2 * nb * sizeof(double)) != 0) return fail(ctx, KIDMP_EINVAL, w + ": the tables' grids differ in D or dD");
            for (int r : shared)
                if (std::memcmp(a + (2 + size_t(r)) * nb, b + (2 + size_t(r)) * nb, nb * sizeof(double)) != 0)
                    return fail(ctx, KIDMP_EINVAL, w + ": the tables' rows that do not depend on the wavelength differ (rho_w?)");
        }
    }
    return KIDMP_OK;
}

int check_ch_stride(kidmp_ctx *ctx, const std::string &w, int64_t ch_stride, int64_t col_stride, int64_t ncol, int32_t nz)
{
    const int64_t need = col_stride != 0 && ncol > 0 ? (ncol - 1) * col_stride + nz : nz;
    if (ch_stride != 0 && ch_stride < need) return fail(ctx, KIDMP_EINVAL, w + ": k_gas_ch_stride must be 0 or hold one channel's profiles");
    return KIDMP_OK;
}

// the table part of the kernel's arguments
template <class Args, class Tab> void set_tables(Args &args, const Tab *const *tables, int32_t nch)
{
    const MieTableData &f = *tables[0];
    for (int x = 0; x < MIE_NSPEC; ++x) {
        args.nb[x] = f.nb[x];
        args.D[x] = f.d_buf + f.off[x];
        args.dD[x] = args.D[x] + f.nb[x];
    }
    args.nch = nch;
    for (int c = 0; c < MC_MAX_CHANNELS; ++c) {
        const MieTableData &t = *tables[c < nch ? c : 0];
        for (int x = 0; x < MIE_NSPEC; ++x) args.rows[c][x] = t.d_buf + t.off[x] + 2 * size_t(t.nb[x]);
        args.kc[c] = t.kc;
        args.rho_w[c] = t.cfg.rho_w;
    }
}

// the strides of a call between the slabs of its channels
struct ChStrides { int64_t k_gas, prof, col; };

// ---- the radiometer ----
struct RadSet {
    const kidmp_radiometer_table *const *tables;
    int32_t nch;
    kidmp_radiometer_cfg r[KIDMP_MAX_CHANNELS];
};

template <class T>
int check_rad_multi(kidmp_ctx *ctx, const char *who, RadSet &set, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz, const RadCall<T> &a,
                    int64_t k_gas_ch_stride)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (int rc = check_set(ctx, w, set.tables, set.nch, RAD_SHARED)) return rc;
    for (int c = 0; c < set.nch; ++c) {
        set.r[c] = resolve(rcfg ? rcfg + c : nullptr);
        if (int rc = check_rad<T>(ctx, who, set.tables[c], set.r[c], ncol, nz, a)) return rc;
    }
    return check_ch_stride(ctx, w, k_gas_ch_stride, a.k_gas_col_stride, ncol, nz);
}

template <class T>
hipError_t enqueue_rad_multi(kidmp_ctx *ctx, const RadSet &set, int64_t ncol, int nz, const RadCall<T> &a, const ChStrides &cs, hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    const T *const *q = a.in;
    RadiometerMultiArgs<T> args{};
    args.t = q[0]; args.p = q[1]; args.qv = q[2]; args.qr = q[3]; args.nr = q[4]; args.qc = q[5];
    args.qs = warm ? nullptr : q[6];
    args.qg = warm ? nullptr : q[7];
    args.dz = a.dz; args.k_gas = a.k_gas; args.t_sfc = a.t_sfc;
    args.dz_col_stride = a.dz_col_stride; args.k_gas_col_stride = a.k_gas_col_stride;
    args.k_gas_ch_stride = cs.k_gas; args.prof_ch_stride = cs.prof; args.col_ch_stride = cs.col;
    for (int v = 0; v < RAD_NOUT; ++v) args.out[v] = a.out[v];
    args.tb_toa = a.col[0]; args.tb_ground = a.col[1]; args.tau_abs = a.col[2];
    set_tables(args, set.tables, set.nch);
    for (int c = 0; c < MC_MAX_CHANNELS; ++c) {
        const kidmp_radiometer_cfg &r = set.r[c < set.nch ? c : 0];
        args.mu[c] = r.mu; args.emissivity[c] = r.emissivity; args.t_cosmic[c] = r.t_cosmic;
    }
    return launch_radiometer_multi<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int rad_multi_device(kidmp_ctx *ctx, const char *who, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
                     int64_t ncol, int32_t nz, const RadCall<T> &a, int64_t k_gas_ch_stride, void *stream)
{
    RadSet set{tables, nch, {}};
    if (int rc = check_rad_multi<T>(ctx, who, set, rcfg, ncol, nz, a, k_gas_ch_stride)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NIN; ++v)
        if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    if (int rc = check_device_array(ctx, who, a.dz, "dz")) return rc;
    if (int rc = check_device_array(ctx, who, a.k_gas, "k_gas")) return rc;
    if (int rc = check_device_array(ctx, who, a.t_sfc, "t_sfc")) return rc;
    for (int v = 0; v < RAD_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], RAD_OUT_NAMES[v])) return rc;
    for (int v = 0; v < NCOL_OUT; ++v)
        if (int rc = check_device_array(ctx, who, a.col[v], RAD_COL_NAMES[v])) return rc;
    const ChStrides cs{k_gas_ch_stride, ncol * int64_t(nz), ncol};
    HIPTRY(ctx, enqueue_rad_multi<T>(ctx, set, ncol, nz, a, cs, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip over the arrays of kidmp_channel_call.h with nch slabs, the chunk narrowed to stay
// below STAGE_LIMIT.  Staged rows are packed; a channel's slab of a staged array is one 256-byte aligned piece of its slot.
template <class T> ChStrides staged_strides(const StagePlan &plan, int nz, const StageArray &k_gas)
{
    const int64_t prof = int64_t(stage_slab_bytes(plan.chunk, nz, sizeof(T)) / sizeof(T)), col = int64_t(stage_slab_bytes(plan.chunk, 1, sizeof(T)) / sizeof(T));
    return ChStrides{k_gas.host && k_gas.nslab > 1 ? prof : 0, prof, col};
}

template <class T>
int rad_multi_host(kidmp_ctx *ctx, const char *who, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
                   int64_t ncol, int32_t nz, const RadCall<T> &h, int64_t k_gas_ch_stride)
{
    RadSet set{tables, nch, {}};
    if (int rc = check_rad_multi<T>(ctx, who, set, rcfg, ncol, nz, h, k_gas_ch_stride)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    StageArray a[RAD_NARRAYS];
    rad_stage_list(ctx, a, ncol, nz, h, nch, k_gas_ch_stride);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol), STAGE_LIMIT);
    if (int rc = stage_open(ctx, plan)) return rc;
    const RadCall<T> d = rad_staged(a, nz, h);
    const ChStrides cs = staged_strides<T>(plan, nz, a[RAD_A_KGAS]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_rad_multi<T>(ctx, set, n, nz, d, cs, ctx->stream); });
}

// ---- the cloud radar ----
struct MieSet {
    const kidmp_mie_table *const *tables;
    int32_t nch;
};

template <class T>
int check_mie_multi(kidmp_ctx *ctx, const char *who, const MieSet &set, int64_t ncol, int32_t nz, const MieCall<T> &a, int64_t k_gas_ch_stride)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (int rc = check_set(ctx, w, set.tables, set.nch, MIE_SHARED)) return rc;
    if (int rc = check_mie<T>(ctx, who, set.tables[0], ncol, nz, a)) return rc;
    return check_ch_stride(ctx, w, k_gas_ch_stride, a.k_gas_col_stride, ncol, nz);
}

template <class T>
hipError_t enqueue_mie_multi(kidmp_ctx *ctx, const MieSet &set, int64_t ncol, int nz, const MieCall<T> &a, const ChStrides &cs, hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    const T *const *q = a.in;
    MieMultiArgs<T> args{};
    args.t = q[0]; args.p = q[1]; args.qv = q[2]; args.qr = q[3]; args.nr = q[4]; args.qc = q[5];
    args.qs = warm ? nullptr : q[6];
    args.qg = warm ? nullptr : q[7];
    args.dz = a.dz; args.w = a.w; args.k_gas = a.k_gas;
    args.dz_col_stride = a.dz_col_stride; args.k_gas_col_stride = a.k_gas_col_stride;
    args.k_gas_ch_stride = cs.k_gas; args.prof_ch_stride = cs.prof; args.col_ch_stride = cs.col;
    for (int v = 0; v < MIE_NOUT; ++v) args.out[v] = a.out[v];
    args.pia_total = a.pia_total;
    set_tables(args, set.tables, set.nch);
    return launch_mie_radar_multi<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int mie_multi_device(kidmp_ctx *ctx, const char *who, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz,
                     const MieCall<T> &a, int64_t k_gas_ch_stride, void *stream)
{
    const MieSet set{tables, nch};
    if (int rc = check_mie_multi<T>(ctx, who, set, ncol, nz, a, k_gas_ch_stride)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NIN; ++v)
        if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    if (int rc = check_device_array(ctx, who, a.dz, "dz")) return rc;
    if (int rc = check_device_array(ctx, who, a.w, "w")) return rc;
    if (int rc = check_device_array(ctx, who, a.k_gas, "k_gas")) return rc;
    for (int v = 0; v < MIE_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], MIE_OUT_NAMES[v])) return rc;
    if (int rc = check_device_array(ctx, who, a.pia_total, "pia_total")) return rc;
    const ChStrides cs{k_gas_ch_stride, ncol * int64_t(nz), ncol};
    HIPTRY(ctx, enqueue_mie_multi<T>(ctx, set, ncol, nz, a, cs, (hipStream_t)stream));
    return KIDMP_OK;
}

template <class T>
int mie_multi_host(kidmp_ctx *ctx, const char *who, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz,
                   const MieCall<T> &h, int64_t k_gas_ch_stride)
{
    const MieSet set{tables, nch};
    if (int rc = check_mie_multi<T>(ctx, who, set, ncol, nz, h, k_gas_ch_stride)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    StageArray a[MIE_NARRAYS];
    mie_stage_list(ctx, a, ncol, nz, h, nch, k_gas_ch_stride);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol), STAGE_LIMIT);
    if (int rc = stage_open(ctx, plan)) return rc;
    const MieCall<T> d = mie_staged(a, nz, h);
    const ChStrides cs = staged_strides<T>(plan, nz, a[MIE_A_KGAS]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_mie_multi<T>(ctx, set, n, nz, d, cs, ctx->stream); });
}
}  // namespace

extern "C" {
int32_t kidmp_multichannel_tile(int32_t which, int32_t nz)
{
    if (nz < 1 || nz > KIDMP_MAX_NZ) return 0;
    return multichannel_tile(which, nz);
}

#define RAD_STATE(T) const T *t, const T *p, const T *qv, const T *qc, const T *qr, const T *nr, const T *qs, const T *qg, const T *dz, \
                     int64_t dz_col_stride, const T *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const T *t_sfc
#define RAD_CALL(T) rad_call<T>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, k_gas, k_gas_col_stride, t_sfc, out)
int kidmp_radiometer_multi_device(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
                                  int64_t ncol, int32_t nz, RAD_STATE(double), const kidmp_radiometer_out *out, void *stream)
{ return rad_multi_device<double>(ctx, "kidmp_radiometer_multi_device", tables, nch, rcfg, ncol, nz, RAD_CALL(double), k_gas_ch_stride, stream); }
int kidmp32_radiometer_multi_device(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
                                    int64_t ncol, int32_t nz, RAD_STATE(float), const kidmp32_radiometer_out *out, void *stream)
{ return rad_multi_device<float>(ctx, "kidmp32_radiometer_multi_device", tables, nch, rcfg, ncol, nz, RAD_CALL(float), k_gas_ch_stride, stream); }
int kidmp_radiometer_multi_host(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
                                int64_t ncol, int32_t nz, RAD_STATE(double), const kidmp_radiometer_out *out)
{ return rad_multi_host<double>(ctx, "kidmp_radiometer_multi_host", tables, nch, rcfg, ncol, nz, RAD_CALL(double), k_gas_ch_stride); }
int kidmp32_radiometer_multi_host(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
                                  int64_t ncol, int32_t nz, RAD_STATE(float), const kidmp32_radiometer_out *out)
{ return rad_multi_host<float>(ctx, "kidmp32_radiometer_multi_host", tables, nch, rcfg, ncol, nz, RAD_CALL(float), k_gas_ch_stride); }
#undef RAD_STATE
#undef RAD_CALL

#define MIE_STATE(T) const T *t, const T *p, const T *qv, const T *qc, const T *qr, const T *nr, const T *qs, const T *qg, const T *dz, \
                     int64_t dz_col_stride, const T *w, const T *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride
#define MIE_CALL(T) mie_call<T>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, w, k_gas, k_gas_col_stride, out)
int kidmp_mie_radar_multi_device(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz, MIE_STATE(double),
                                 const kidmp_mie_out *out, void *stream)
{ return mie_multi_device<double>(ctx, "kidmp_mie_radar_multi_device", tables, nch, ncol, nz, MIE_CALL(double), k_gas_ch_stride, stream); }
int kidmp32_mie_radar_multi_device(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz, MIE_STATE(float),
                                   const kidmp32_mie_out *out, void *stream)
{ return mie_multi_device<float>(ctx, "kidmp32_mie_radar_multi_device", tables, nch, ncol, nz, MIE_CALL(float), k_gas_ch_stride, stream); }
int kidmp_mie_radar_multi_host(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz, MIE_STATE(double),
                               const kidmp_mie_out *out)
{ return mie_multi_host<double>(ctx, "kidmp_mie_radar_multi_host", tables, nch, ncol, nz, MIE_CALL(double), k_gas_ch_stride); }
int kidmp32_mie_radar_multi_host(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz, MIE_STATE(float),
                                 const kidmp32_mie_out *out)
{ return mie_multi_host<float>(ctx, "kidmp32_mie_radar_multi_host", tables, nch, ncol, nz, MIE_CALL(float), k_gas_ch_stride); }
#undef MIE_STATE
#undef MIE_CALL
}  // extern "C"
