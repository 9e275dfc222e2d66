// kidmp_mie.hip -- the entries of include/kidmp_mie.h: the Lorenz-Mie sphere and the per-bin rows on the host
// (kidmp_mie_sphere.h), the table object that carries them to the device, and the cloud radar of device arrays in one
// launch of k_mie_radar (below) or of host arrays in chunks through the context's staging memory.
#include <cmath>
#include <cstddef>

#include "kidmp_mie_channel.h"

namespace kidmp {

// The cloud radar (include/kidmp_mie.h): Mie reflectivity, extinction, path-integrated attenuation and mean Doppler
// velocity from k_doppler_moments' load and a table of five rows per diameter bin.  Null means: qc, qs, qg, w, k_gas --
// zero; an output -- not wanted; dz -- not read when no path integral is wanted.  out in the order of kidmp_mie_out,
// pia_total [ncol].  D, dD: device arrays of nb[x] doubles by species rain, snow, graupel; rows[x]: [MIE_NROWS][nb[x]]
// (s_mie, s_ray, s_ext, mass, v0).  kc: (6 pi/lambda) Im(K(eps_w)); rho_w: the configuration's.  Cloud water enters through
// its mass alone, where qc > R1.  One launch; lanes over levels, a loop over the bins.
template <class T> struct MieArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *w, *k_gas;
    int64_t dz_col_stride, k_gas_col_stride;
    T *out[MIE_NOUT];
    T *pia_total;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC], *rows[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    double kc, rho_w;
};

// One wavefront per column: the cloud radar of include/kidmp_mie.h.  The load and the scan are k_doppler_moments'
// (load_channel_levels), lanes over levels.  Then species by species -- rain, snow, graupel -- the five sums over the
// table's bins (mie_sums), which leave behind only mie_x, the species' extinction and its share of the Doppler sums
// (mie_species_finish).  Cloud water (present where qc > R1) and the caller's gas extinction close ext; the path integrals
// are column_depths, the scans of k_lidar_profiles, and a request without them ends before (mie_tail).  No atomics, no
// scratch, nothing but the fastmath tables in LDS.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_mie_radar(ReflConsts c, DopplerConsts dc, MieArgs<T> a, int64_t ncol, int nz)
{
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    T *const *out = a.out;
    const MieChannel<T> ch{out, 0, a.pia_total, a.k_gas ? a.k_gas + col * a.k_gas_col_stride : nullptr, a.kc, a.rho_w};
    const MieWants want = mie_wants<T>(out, a.pia_total);
    const auto wants = [&](int x) __attribute__((always_inline)) { return want.all || out[MIE_DBZ_X + x] || out[MIE_MIE_X + x]; };

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);

    // what the species leave behind: ze_x' in ze_x, ext = (ext_r + ext_s) + ext_g, and the Doppler sums over the species
    // that are present with A above 0
    double ext[NJ], zw[NJ], zv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) ext[j] = zw[j] = zv[j] = 0.;
    double A[1][NJ], B[NJ], E[1][NJ], M[NJ], V[1][NJ];
    if (wants(0)) {
        double rr[NJ];
        rain_mass<NJ>(a, base, lane, L, rr);
        const double *const rows[1] = {a.rows[0]};
        mie_sums<0, NJ, 1>(a.D[0], a.dD[0], a.nb[0], rows, 1, lane, L.lqr,
                           [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); },
                           A, B, E, M, V);
        mie_species_finish<T, NJ>(L.lqr, rr, A[0], B, E[0], M, V[0], L.ze_r, ext, zw, zv, out[MIE_MIE_X + 0], out[MIE_DBZ_X + 0], base, nz, lane);
    }
    if (wants(1)) {
        const double *const rows[1] = {a.rows[1]};
        mie_sums<1, NJ, 1>(a.D[1], a.dD[1], a.nb[1], rows, 1, lane, L.lqs,
                           [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); },
                           A, B, E, M, V);
        mie_species_finish<T, NJ>(L.lqs, L.rs, A[0], B, E[0], M, V[0], L.ze_s, ext, zw, zv, out[MIE_MIE_X + 1], out[MIE_DBZ_X + 1], base, nz, lane);
    }
    if (wants(2)) {
        const double *const rows[1] = {a.rows[2]};
        mie_sums<2, NJ, 1>(a.D[2], a.dD[2], a.nb[2], rows, 1, lane, L.lqg,
                           [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); },
                           A, B, E, M, V);
        mie_species_finish<T, NJ>(L.lqg, L.rg, A[0], B, E[0], M, V[0], L.ze_g, ext, zw, zv, out[MIE_MIE_X + 2], out[MIE_DBZ_X + 2], base, nz, lane);
    }
    if (!want.all) return;                                           // wave-uniform: one species' own profiles alone
    mie_tail<T, NJ>(a, ch, want, col, base, nz, lane, L, L.ze_r, L.ze_s, L.ze_g, ext, zw, zv);
}

namespace {
template <class T>
hipError_t launch_mie_radar(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const MieArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // an empty batch is not looked at
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_mie_radar<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, dc, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

using namespace kidmp;

static_assert(sizeof(kidmp_mie_out) == (MIE_NOUT + 1) * sizeof(double *) && sizeof(kidmp32_mie_out) == (MIE_NOUT + 1) * sizeof(float *)
                  && MIE_NSPEC == KIDMP_MIE_NSPECIES && MIE_MAX_BINS == KIDMP_MIE_MAX_BINS && MIE_NROWS == KIDMP_MIE_NROWS
                  && MIE_ROWS == KIDMP_MIE_NROWS && nbins <= KIDMP_MIE_MAX_BINS && sizeof(kidmp_mie_cfg) == 8 * sizeof(double)
                  && MIE_RAIN == KIDMP_MIE_R && MIE_SNOW == KIDMP_MIE_S && MIE_GRAUPEL == KIDMP_MIE_G,
              "include/kidmp_mie.h");

namespace {
// one launch over device pointers; an iiwarm context reads no snow and no graupel
template <class T>
hipError_t enqueue_mie(kidmp_ctx *ctx, const kidmp_mie_table *tab, int64_t ncol, int nz, const MieCall<T> &a, hipStream_t s)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    const T *const *q = a.in;
    MieArgs<T> args{};
    args.t = q[0]; args.p = q[1]; args.qv = q[2]; args.qr = q[3]; args.nr = q[4]; args.qc = q[5];
    args.qs = warm ? nullptr : q[6];
    args.qg = warm ? nullptr : q[7];
    args.dz = a.dz; args.w = a.w; args.k_gas = a.k_gas;
    args.dz_col_stride = a.dz_col_stride; args.k_gas_col_stride = a.k_gas_col_stride;
    for (int v = 0; v < MIE_NOUT; ++v) args.out[v] = a.out[v];
    args.pia_total = a.pia_total;
    for (int x = 0; x < MIE_NSPEC; ++x) {
        const double *b = tab->d_buf + tab->off[x];
        args.nb[x] = tab->nb[x];
        args.D[x] = b;
        args.dD[x] = b + tab->nb[x];
        args.rows[x] = b + 2 * size_t(tab->nb[x]);
    }
    args.kc = tab->kc;
    args.rho_w = tab->cfg.rho_w;
    return launch_mie_radar<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int mie_device(kidmp_ctx *ctx, const char *who, const kidmp_mie_table *tab, int64_t ncol, int32_t nz, const MieCall<T> &a, void *stream)
{
    if (int rc = check_mie<T>(ctx, who, tab, ncol, nz, a)) return rc;
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
    HIPTRY(ctx, enqueue_mie<T>(ctx, tab, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip.  Only the inputs the kernel reads go up and only what was asked for comes down.
template <class T>
int mie_host(kidmp_ctx *ctx, const char *who, const kidmp_mie_table *tab, int64_t ncol, int32_t nz, const MieCall<T> &h)
{
    if (int rc = check_mie<T>(ctx, who, tab, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    StageArray a[MIE_NARRAYS];
    mie_stage_list(ctx, a, ncol, nz, h, 1, 0);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    const MieCall<T> d = mie_staged(a, nz, h);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_mie<T>(ctx, tab, n, nz, d, ctx->stream); });
}
}  // namespace

extern "C" {
void kidmp_mie_defaults(kidmp_mie_cfg *cfg)
{
    if (!cfg) return;
    const double k = std::sqrt(0.176);
    *cfg = kidmp_mie_cfg{0.10, 79.5, 24.9, (1. + 2. * k) / (1. - k), 0., 1000., 900., 0.93};
}

int kidmp_mie_sphere(double x, double m_re, double m_im, double *qext, double *qback)
{
    if (!qext || !qback) return fail(nullptr, KIDMP_EINVAL, "kidmp_mie_sphere: null argument");
    double qe, qb;
    if (!mie_sphere(x, m_re, m_im, qe, qb))
        return fail(nullptr, KIDMP_EINVAL, "kidmp_mie_sphere: x and Re(m) must be finite and above 0, Im(m) finite and not below 0, |m| x below 1e7");
    *qext = qe;
    *qback = qb;
    return KIDMP_OK;
}

int kidmp_mie_bins(const kidmp_mie_cfg *cfg, int32_t species, int32_t nb, const double *D, double *rows)
{
    const std::string w("kidmp_mie_bins");
    if (!cfg || !D || !rows) return fail(nullptr, KIDMP_EINVAL, w + ": null argument");
    if (const char *bad = mie_bad_cfg(*cfg)) return fail(nullptr, KIDMP_EINVAL, w + ": " + bad);
    if (species < 0 || species >= MIE_NSPEC) return fail(nullptr, KIDMP_EINVAL, w + ": unknown species");
    if (nb < 1) return fail(nullptr, KIDMP_EINVAL, w + ": nb < 1");
    std::vector<double> r(size_t(MIE_ROWS) * size_t(nb));
    if (!mie_bins(mie_model_cfg(*cfg), species, nb, D, r.data()))
        return fail(nullptr, KIDMP_EINVAL, w + ": a diameter is not finite or not above 0, or its sphere has more than 1e7 terms");
    std::memcpy(rows, r.data(), r.size() * sizeof(double));
    return KIDMP_OK;
}

int kidmp_mie_table_create(kidmp_ctx *ctx, const kidmp_mie_cfg *cfg, const kidmp_mie_grids *grids, kidmp_mie_table **table)
{
    const std::string w("kidmp_mie_table_create");
    if (table) *table = nullptr;
    if (int rc = require_ready(ctx)) return rc;
    if (!table) return fail(ctx, KIDMP_EINVAL, w + ": null argument");
    MieTableData d;
    if (int rc = mie_table_build(ctx, w, cfg, grids, MIE_ROWS, mie_bins, &d)) return rc;
    kidmp_mie_table *t = new kidmp_mie_table;
    static_cast<MieTableData &>(*t) = d;
    *table = t;
    return KIDMP_OK;
}

void kidmp_mie_table_destroy(kidmp_mie_table *table)
{
    if (!table) return;
    mie_table_free(table);
    delete table;
}

int kidmp_mie_table_get(const kidmp_mie_table *table, int32_t species, int32_t *nb, double *D, double *dD, double *rows, kidmp_mie_cfg *cfg)
{
    const std::string w("kidmp_mie_table_get");
    if (!table) return fail(nullptr, KIDMP_EINVAL, w + ": null table");
    return mie_table_read(table, w, species, nb, D, dD, rows, cfg);
}

int kidmp_mie_radar_device(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz, const double *t, const double *p,
                           const double *qv, const double *qc, const double *qr, const double *nr, const double *qs, const double *qg,
                           const double *dz, int64_t dz_col_stride, const double *w, const double *k_gas, int64_t k_gas_col_stride,
                           const kidmp_mie_out *out, void *stream)
{
    return mie_device<double>(ctx, "kidmp_mie_radar_device", table, ncol, nz,
                              mie_call<double>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, w, k_gas, k_gas_col_stride, out), stream);
}
int kidmp32_mie_radar_device(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz, const float *t, const float *p,
                             const float *qv, const float *qc, const float *qr, const float *nr, const float *qs, const float *qg,
                             const float *dz, int64_t dz_col_stride, const float *w, const float *k_gas, int64_t k_gas_col_stride,
                             const kidmp32_mie_out *out, void *stream)
{
    return mie_device<float>(ctx, "kidmp32_mie_radar_device", table, ncol, nz,
                             mie_call<float>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, w, k_gas, k_gas_col_stride, out), stream);
}
int kidmp_mie_radar_host(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz, const double *t, const double *p,
                         const double *qv, const double *qc, const double *qr, const double *nr, const double *qs, const double *qg,
                         const double *dz, int64_t dz_col_stride, const double *w, const double *k_gas, int64_t k_gas_col_stride,
                         const kidmp_mie_out *out)
{
    return mie_host<double>(ctx, "kidmp_mie_radar_host", table, ncol, nz,
                            mie_call<double>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, w, k_gas, k_gas_col_stride, out));
}
int kidmp32_mie_radar_host(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz, const float *t, const float *p,
                           const float *qv, const float *qc, const float *qr, const float *nr, const float *qs, const float *qg,
                           const float *dz, int64_t dz_col_stride, const float *w, const float *k_gas, int64_t k_gas_col_stride,
                           const kidmp32_mie_out *out)
{
    return mie_host<float>(ctx, "kidmp32_mie_radar_host", table, ncol, nz,
                           mie_call<float>(t, p, qv, qc, qr, nr, qs, qg, dz, dz_col_stride, w, k_gas, k_gas_col_stride, out));
}
}  // extern "C"
