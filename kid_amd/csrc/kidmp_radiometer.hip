// kidmp_radiometer.hip -- the entries of include/kidmp_radiometer.h: the sphere's four efficiencies and the per-bin rows on
// the host (kidmp_mie_sphere.h), the table object that carries them to the device (kidmp_mie_table.h), and the radiometer
// of device arrays in one launch of k_radiometer (below) or of host arrays in chunks through the
// context's staging memory.  No kernel of its own.
#include <cmath>
#include <cstddef>

#include "kidmp_radiometer_channel.h"

namespace kidmp {

// The microwave radiometer (include/kidmp_radiometer.h): absorption and back-hemisphere scattering coefficients from
// k_mie_radar's load and a table of three rows per diameter bin (s_abs, s_bsc, mass), the two-stream layer of every level
// and the adding of the layers by two wave scans.  Null means: qc, qs, qg, k_gas -- zero; t_sfc -- the column's t at level
// 0; an output -- not wanted; dz -- not read when only k_abs and k_bsc are wanted.  out: k_abs, k_bsc, refl, trans, tb_up,
// tb_down [ncol][nz]; tb_toa, tb_ground, tau_abs [ncol].  One launch; lanes over levels, a loop over the bins.
template <class T> struct RadiometerArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *k_gas, *t_sfc;
    int64_t dz_col_stride, k_gas_col_stride;
    T *out[RAD_NOUT];
    T *tb_toa, *tb_ground, *tau_abs;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC], *rows[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    double kc, rho_w, mu, emissivity, t_cosmic;
};

// One wavefront per column: the radiometer of include/kidmp_radiometer.h.  The load is k_mie_radar's (load_channel_levels),
// lanes over levels.  Then species by species the three sums over the table's bins (radiometer_sums), which leave behind
// only k_abs and k_bsc; the rest is radiometer_tail.  No atomics, no scratch, nothing but the fastmath tables in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_radiometer(ReflConsts c, DopplerConsts dc, RadiometerArgs<T> a, int64_t ncol, int nz)
{
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    const RadChannel<T> ch{a.out, 0, a.tb_toa, a.tb_ground, a.tau_abs, a.k_gas ? a.k_gas + col * a.k_gas_col_stride : nullptr,
                           a.kc, a.rho_w, a.mu, a.emissivity, a.t_cosmic};

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);

    // ---- k_abs = (((abs_r + abs_s) + abs_g) + abs_c) + k_gas, k_bsc = (bsc_r + bsc_s) + bsc_g; levels past nz keep +0.0 ----
    double kabs[NJ], kbsc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) kabs[j] = kbsc[j] = 0.;
    {
        double A[1][NJ], S[1][NJ], M[NJ], rr[NJ];
        rain_mass<NJ>(a, base, lane, L, rr);
        const double *const rows_r[1] = {a.rows[0]}, *const rows_s[1] = {a.rows[1]}, *const rows_g[1] = {a.rows[2]};
        radiometer_sums<0, NJ, 1>(a.D[0], a.dD[0], a.nb[0], rows_r, 1, lane, L.lqr,
                                  [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); }, A, S, M);
        radiometer_species_finish<NJ>(L.lqr, rr, A[0], S[0], M, kabs, kbsc);
        radiometer_sums<1, NJ, 1>(a.D[1], a.dD[1], a.nb[1], rows_s, 1, lane, L.lqs,
                                  [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); }, A, S, M);
        radiometer_species_finish<NJ>(L.lqs, L.rs, A[0], S[0], M, kabs, kbsc);
        radiometer_sums<2, NJ, 1>(a.D[2], a.dD[2], a.nb[2], rows_g, 1, lane, L.lqg,
                                  [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); }, A, S, M);
        radiometer_species_finish<NJ>(L.lqg, L.rg, A[0], S[0], M, kabs, kbsc);
    }
    radiometer_tail<T, NJ>(a, ch, col, base, nz, lane, L, kabs, kbsc);
}

namespace {
template <class T>
hipError_t launch_radiometer(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const RadiometerArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // an empty batch is not looked at
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_radiometer<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, dc, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

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

// host arrays: stage_run of kidmp_host.hip.  Only the inputs the kernel reads go up and only what was asked for comes down.
template <class T>
int rad_host(kidmp_ctx *ctx, const char *who, const kidmp_radiometer_table *tab, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
             const RadCall<T> &h)
{
    const kidmp_radiometer_cfg r = resolve(rcfg);
    if (int rc = check_rad<T>(ctx, who, tab, r, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    StageArray a[RAD_NARRAYS];
    rad_stage_list(ctx, a, ncol, nz, h, 1, 0);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    const RadCall<T> d = rad_staged(a, nz, h);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_rad<T>(ctx, tab, r, n, nz, d, ctx->stream); });
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
