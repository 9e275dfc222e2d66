// kidmp_radiometer.hip -- the entries of include/kidmp_radiometer.h: the sphere's four efficiencies and the per-bin rows on
// the host (kidmp_mie_sphere.h), the table object that carries them to the device (kidmp_mie_table.h), and the radiometer
// of device arrays in one launch of k_radiometer (thompson_reflectivity.hip) or of host arrays in chunks through the
// context's staging memory.  No kernel of its own.
#include <cmath>
#include <cstddef>

#include "kidmp_channel_call.h"

using namespace kidmp;

static_assert(sizeof(kidmp_radiometer_out) == (RAD_NOUT + 3) * sizeof(double *) && sizeof(kidmp32_radiometer_out) == (RAD_NOUT + 3) * sizeof(float *)
                  && RAD_NROWS == KIDMP_RADIOMETER_NROWS && RADIOMETER_ROWS == KIDMP_RADIOMETER_NROWS
                  && sizeof(kidmp_radiometer_cfg) == 3 * sizeof(double),
              "include/kidmp_radiometer.h");

namespace {
// one launch over device pointers; an iiwarm context reads no snow and no graupel
template <class T>
hipError_t enqueue_rad(kidmp_ctx *ctx, const kidmp_radiometer_table *tab, const kidmp_radiometer_cfg &r, int64_t ncol, int nz, const RadCall<T> &a,
                       hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    const T *const *q = a.in;
    RadiometerArgs<T> args{};
    args.t = q[0]; args.p = q[1]; args.qv = q[2]; args.qr = q[3]; args.nr = q[4]; args.qc = q[5];
    args.qs = warm ? nullptr : q[6];
    args.qg = warm ? nullptr : q[7];
    args.dz = a.dz; args.k_gas = a.k_gas; args.t_sfc = a.t_sfc;
    args.dz_col_stride = a.dz_col_stride; args.k_gas_col_stride = a.k_gas_col_stride;
    for (int v = 0; v < RAD_NOUT; ++v) args.out[v] = a.out[v];
    args.tb_toa = a.col[0]; args.tb_ground = a.col[1]; args.tau_abs = a.col[2];
    for (int x = 0; x < MIE_NSPEC; ++x) {
        const double *b = tab->d_buf + tab->off[x];
        args.nb[x] = tab->nb[x];
        args.D[x] = b;
        args.dD[x] = b + tab->nb[x];
        args.rows[x] = b + 2 * size_t(tab->nb[x]);
    }
    args.kc = tab->kc;
    args.rho_w = tab->cfg.rho_w;
    args.mu = r.mu; args.emissivity = r.emissivity; args.t_cosmic = r.t_cosmic;
    return launch_radiometer<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int rad_device(kidmp_ctx *ctx, const char *who, const kidmp_radiometer_table *tab, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
               const RadCall<T> &a, void *stream)
{
    const kidmp_radiometer_cfg r = resolve(rcfg);
    if (int rc = check_rad<T>(ctx, who, tab, r, ncol, nz, a)) return rc;
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
    HIPTRY(ctx, enqueue_rad<T>(ctx, tab, r, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: chunks of columns through the context's staging memory on its compute stream, one after the other
// (mie_host of kidmp_mie.hip).  A column's result does not depend on its batch, so any chunking gives the same bits.
// Only the inputs given go up and only what was asked for comes down.
template <class T>
int rad_host(kidmp_ctx *ctx, const char *who, const kidmp_radiometer_table *tab, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
             const RadCall<T> &h)
{
    const kidmp_radiometer_cfg r = resolve(rcfg);
    if (int rc = check_rad<T>(ctx, who, tab, r, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const bool warm = ctx->cfg.iiwarm != 0, with_dz = needs_dz(h);
    const int64_t CH = pick_host_chunk(ctx, ncol);
    const size_t b_prof = (size_t(CH) * size_t(nz) * sizeof(T) + 255) / 256 * 256, b_col = (size_t(CH) * sizeof(T) + 255) / 256 * 256;
    bool up[NIN];
    int slots = (with_dz ? 1 : 0) + (h.k_gas ? 1 : 0), cols = h.t_sfc ? 1 : 0;
    for (int v = 0; v < NIN; ++v) {
        up[v] = h.in[v] && !(warm && v >= 6);
        slots += up[v];
    }
    for (int v = 0; v < RAD_NOUT; ++v) slots += h.out[v] != nullptr;
    for (int v = 0; v < NCOL_OUT; ++v) cols += h.col[v] != nullptr;
    if (int rc = ensure_stage(ctx, size_t(slots) * b_prof + size_t(cols) * b_col)) return rc;
    char *next = reinterpret_cast<char *>(ctx->d_stage);
    auto slot = [&](bool wanted, size_t bytes) { T *p = wanted ? reinterpret_cast<T *>(next) : nullptr; if (wanted) next += bytes; return p; };
    RadCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = slot(up[v], b_prof);
    T *const d_dz = slot(with_dz, b_prof), *const d_kg = slot(h.k_gas != nullptr, b_prof);
    d.dz = d_dz; d.k_gas = d_kg;
    d.dz_col_stride = h.dz_col_stride ? nz : 0;           // staged rows are packed
    d.k_gas_col_stride = h.k_gas_col_stride ? nz : 0;
    for (int v = 0; v < RAD_NOUT; ++v) d.out[v] = slot(h.out[v] != nullptr, b_prof);
    T *const d_ts = slot(h.t_sfc != nullptr, b_col);
    d.t_sfc = d_ts;
    for (int v = 0; v < NCOL_OUT; ++v) d.col[v] = slot(h.col[v] != nullptr, b_col);
    hipError_t e = hipSuccess;
    const size_t row = size_t(nz) * sizeof(T);
    if (with_dz && !h.dz_col_stride) e = hipMemcpyAsync(d_dz, h.dz, row, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && h.k_gas && !h.k_gas_col_stride) e = hipMemcpyAsync(d_kg, h.k_gas, row, hipMemcpyHostToDevice, ctx->stream);
    for (int64_t c0 = 0; c0 < ncol && e == hipSuccess; c0 += CH) {
        const int64_t n = c0 + CH <= ncol ? CH : ncol - c0;
        const size_t off = size_t(c0) * size_t(nz), cnt = size_t(n) * size_t(nz);
        for (int v = 0; v < NIN && e == hipSuccess; ++v)
            if (up[v]) e = hipMemcpyAsync(const_cast<T *>(d.in[v]), h.in[v] + off, cnt * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && h.t_sfc) e = hipMemcpyAsync(d_ts, h.t_sfc + c0, size_t(n) * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && with_dz && h.dz_col_stride)
            e = hipMemcpy2DAsync(d_dz, row, h.dz + size_t(c0) * size_t(h.dz_col_stride), size_t(h.dz_col_stride) * sizeof(T), row, size_t(n),
                                 hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && h.k_gas && h.k_gas_col_stride)
            e = hipMemcpy2DAsync(d_kg, row, h.k_gas + size_t(c0) * size_t(h.k_gas_col_stride), size_t(h.k_gas_col_stride) * sizeof(T), row,
                                 size_t(n), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = enqueue_rad<T>(ctx, tab, r, n, nz, d, ctx->stream);
        for (int v = 0; v < RAD_NOUT && e == hipSuccess; ++v)
            if (h.out[v]) e = hipMemcpyAsync(h.out[v] + off, d.out[v], cnt * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
        for (int v = 0; v < NCOL_OUT && e == hipSuccess; ++v)
            if (h.col[v]) e = hipMemcpyAsync(h.col[v] + c0, d.col[v], size_t(n) * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);        // no copy may still be in flight towards the caller's arrays
    HIPTRY(ctx, e);
    HIPTRY(ctx, es);
    return KIDMP_OK;
}
}  // namespace

extern "C" {
void kidmp_radiometer_defaults(kidmp_radiometer_cfg *rcfg)
{
    if (!rcfg) return;
    *rcfg = kidmp_radiometer_cfg{1.0, 1.0, 2.725};
}

int kidmp_radiometer_sphere(double x, double m_re, double m_im, double *qext, double *qsca, double *qback, double *g)
{
    if (!qext || !qsca || !qback || !g) return fail(nullptr, KIDMP_EINVAL, "kidmp_radiometer_sphere: null argument");
    MieEff e;
    if (!mie_efficiencies(x, m_re, m_im, e))
        return fail(nullptr, KIDMP_EINVAL,
                    "kidmp_radiometer_sphere: x and Re(m) must be finite and above 0, Im(m) finite and not below 0, |m| x below 1e7");
    *qext = e.qext;
    *qsca = e.qsca;
    *qback = e.qback;
    *g = e.g;
    return KIDMP_OK;
}

int kidmp_radiometer_bins(const kidmp_mie_cfg *cfg, int32_t species, int32_t nb, const double *D, double *rows)
{
    const std::string w("kidmp_radiometer_bins");
    if (!cfg || !D || !rows) return fail(nullptr, KIDMP_EINVAL, w + ": null argument");
    if (const char *bad = mie_bad_cfg(*cfg)) return fail(nullptr, KIDMP_EINVAL, w + ": " + bad);
    if (species < 0 || species >= MIE_NSPEC) return fail(nullptr, KIDMP_EINVAL, w + ": unknown species");
    if (nb < 1) return fail(nullptr, KIDMP_EINVAL, w + ": nb < 1");
    std::vector<double> r(size_t(RADIOMETER_ROWS) * size_t(nb));
    if (!radiometer_bins(mie_model_cfg(*cfg), species, nb, D, r.data()))
        return fail(nullptr, KIDMP_EINVAL, w + ": a diameter is not finite or not above 0, or its sphere has more than 1e7 terms");
    std::memcpy(rows, r.data(), r.size() * sizeof(double));
    return KIDMP_OK;
}

int kidmp_radiometer_table_create(kidmp_ctx *ctx, const kidmp_mie_cfg *cfg, const kidmp_mie_grids *grids, kidmp_radiometer_table **table)
{
    const std::string w("kidmp_radiometer_table_create");
    if (table) *table = nullptr;
    if (int rc = require_ready(ctx)) return rc;
    if (!table) return fail(ctx, KIDMP_EINVAL, w + ": null argument");
    MieTableData d;
    if (int rc = mie_table_build(ctx, w, cfg, grids, RADIOMETER_ROWS, radiometer_bins, &d)) return rc;
    kidmp_radiometer_table *t = new kidmp_radiometer_table;
    static_cast<MieTableData &>(*t) = d;
    *table = t;
    return KIDMP_OK;
}

void kidmp_radiometer_table_destroy(kidmp_radiometer_table *table)
{
    if (!table) return;
    mie_table_free(table);
    delete table;
}

int kidmp_radiometer_table_get(const kidmp_radiometer_table *table, int32_t species, int32_t *nb, double *D, double *dD, double *rows,
                               kidmp_mie_cfg *cfg)
{
    const std::string w("kidmp_radiometer_table_get");
    if (!table) return fail(nullptr, KIDMP_EINVAL, w + ": null table");
    return mie_table_read(table, w, species, nb, D, dD, rows, cfg);
}

int kidmp_radiometer_device(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
                            const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
                            const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const double *k_gas,
                            int64_t k_gas_col_stride, const double *t_sfc, const kidmp_radiometer_out *out, void *stream)
{
    return rad_device<double>(ctx, "kidmp_radiometer_device", table, rcfg, ncol, nz,
                              rad_call<double>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, k_gas, k_gas_col_stride, t_sfc, out), stream);
}
int kidmp32_radiometer_device(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
                              const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
                              const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const float *k_gas,
                              int64_t k_gas_col_stride, const float *t_sfc, const kidmp32_radiometer_out *out, void *stream)
{
    return rad_device<float>(ctx, "kidmp32_radiometer_device", table, rcfg, ncol, nz,
                             rad_call<float>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, k_gas, k_gas_col_stride, t_sfc, out), stream);
}
int kidmp_radiometer_host(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
                          const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
                          const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const double *k_gas,
                          int64_t k_gas_col_stride, const double *t_sfc, const kidmp_radiometer_out *out)
{
    return rad_host<double>(ctx, "kidmp_radiometer_host", table, rcfg, ncol, nz,
                            rad_call<double>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, k_gas, k_gas_col_stride, t_sfc, out));
}
int kidmp32_radiometer_host(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
                            const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
                            const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const float *k_gas,
                            int64_t k_gas_col_stride, const float *t_sfc, const kidmp32_radiometer_out *out)
{
    return rad_host<float>(ctx, "kidmp32_radiometer_host", table, rcfg, ncol, nz,
                           rad_call<float>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, k_gas, k_gas_col_stride, t_sfc, out));
}
}  // extern "C"
