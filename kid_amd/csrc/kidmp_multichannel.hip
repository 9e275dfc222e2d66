// kidmp_multichannel.hip -- the entries of include/kidmp_multichannel.h: a set of existing radiometer or cloud-radar tables
// checked on the host (same context, same grids, the wavelength-independent rows equal bit for bit) and run in one launch
// of k_radiometer_multi or k_mie_radar_multi (below), over device arrays or over host arrays in chunks
// through the context's staging memory.  No kernel of its own.
#include <cstddef>
#include <cstring>

#include "kidmp_mie_channel.h"
#include "kidmp_radiometer_channel.h"
#include "../../include/kidmp_multichannel.h"

namespace kidmp {

// Several channels of the radiometer or of the cloud radar in one launch (include/kidmp_multichannel.h): the load and the
// densities of the bin loop are formed once and shared by the channels, which are taken in tiles of
// multichannel_tile(which, nz) inside the launch.  The state, dz, w and t_sfc are the single-channel kernels'; everything
// else is per channel c < nch: rows[c][x] the species' rows of the channel's table (all tables on the grids D, dD, nb, the
// rows that do not depend on the wavelength equal bit for bit), kc, rho_w and the radiometer's closure, k_gas at
// k_gas + c*k_gas_ch_stride, and the slab of every output: a profile at out + c*prof_ch_stride, a per-column one at
// + c*col_ch_stride.  Slab c holds the bits the single-channel kernel writes with channel c's table.
constexpr int MC_MAX_CHANNELS = 16;
template <class T> struct RadiometerMultiArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *k_gas, *t_sfc;
    int64_t dz_col_stride, k_gas_col_stride, k_gas_ch_stride, prof_ch_stride, col_ch_stride;
    T *out[RAD_NOUT];
    T *tb_toa, *tb_ground, *tau_abs;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    int32_t nch;
    const double *rows[MC_MAX_CHANNELS][MIE_NSPEC];
    double kc[MC_MAX_CHANNELS], rho_w[MC_MAX_CHANNELS], mu[MC_MAX_CHANNELS], emissivity[MC_MAX_CHANNELS], t_cosmic[MC_MAX_CHANNELS];
};
template <class T> struct MieMultiArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *w, *k_gas;
    int64_t dz_col_stride, k_gas_col_stride, k_gas_ch_stride, prof_ch_stride, col_ch_stride;
    T *out[MIE_NOUT];
    T *pia_total;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    int32_t nch;
    const double *rows[MC_MAX_CHANNELS][MIE_NSPEC];
    double kc[MC_MAX_CHANNELS], rho_w[MC_MAX_CHANNELS];
};

// One wavefront per column: nch channels of the cloud radar (include/kidmp_multichannel.h).  The load is formed once; the
// channels are taken in tiles of CT, and per tile and species one walk over the bins forms every density once and folds
// it into the sums of the tile's channels (mie_sums).  What stays alive per channel across the species is ze_r', ze_s',
// ze_g', ext and the two Doppler sums; mie_species_finish and mie_tail then run per channel as in k_mie_radar, so slab c
// of every output holds k_mie_radar's bits for channel c's table.  No atomics, no scratch.
template <class T, int NJ, int CT>
__global__ void __launch_bounds__(REFL_THREADS)
k_mie_radar_multi(ReflConsts c, DopplerConsts dc, MieMultiArgs<T> a, int64_t ncol, int nz)
{
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    const MieWants want = mie_wants<T>(a.out, a.pia_total);
    const auto wants = [&](int x) __attribute__((always_inline)) { return want.all || a.out[MIE_DBZ_X + x] || a.out[MIE_MIE_X + x]; };

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);
    double rr[NJ];
    rain_mass<NJ>(a, base, lane, L, rr);

    for (int c0 = 0; c0 < a.nch; c0 += CT) {
        const int used = a.nch - c0 < CT ? a.nch - c0 : CT;
        double ze_r[CT][NJ], ze_s[CT][NJ], ze_g[CT][NJ], ext[CT][NJ], zw[CT][NJ], zv[CT][NJ];
#pragma unroll
        for (int cc = 0; cc < CT; ++cc)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                ze_r[cc][j] = L.ze_r[j]; ze_s[cc][j] = L.ze_s[j]; ze_g[cc][j] = L.ze_g[j];
                ext[cc][j] = zw[cc][j] = zv[cc][j] = 0.;
            }
        double A[CT][NJ], B[NJ], E[CT][NJ], M[NJ], V[CT][NJ];
        const auto rows_of = [&](int x, const double *(&rows)[CT]) __attribute__((always_inline)) {
#pragma unroll
            for (int cc = 0; cc < CT; ++cc) rows[cc] = a.rows[c0 + (cc < used ? cc : 0)][x];
        };
        const auto finish = [&](int x, const bool (&has)[NJ], const double (&rq)[NJ], double (&ze)[CT][NJ]) __attribute__((always_inline)) {
#pragma unroll
            for (int cc = 0; cc < CT; ++cc) {
                if (cc >= used) continue;                            // wave-uniform
                const int64_t slab = int64_t(c0 + cc) * a.prof_ch_stride;
                T *const om = a.out[MIE_MIE_X + x], *const od = a.out[MIE_DBZ_X + x];
                mie_species_finish<T, NJ>(has, rq, A[cc], B, E[cc], M, V[cc], ze[cc], ext[cc], zw[cc], zv[cc], om ? om + slab : nullptr,
                                          od ? od + slab : nullptr, base, nz, lane);
            }
        };
        const double *rows[CT];
        if (wants(0)) {
            rows_of(0, rows);
            mie_sums<0, NJ, CT>(a.D[0], a.dD[0], a.nb[0], rows, used, lane, L.lqr,
                                [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); },
                                A, B, E, M, V);
            finish(0, L.lqr, rr, ze_r);
        }
        if (wants(1)) {
            rows_of(1, rows);
            mie_sums<1, NJ, CT>(a.D[1], a.dD[1], a.nb[1], rows, used, lane, L.lqs,
                                [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); },
                                A, B, E, M, V);
            finish(1, L.lqs, L.rs, ze_s);
        }
        if (wants(2)) {
            rows_of(2, rows);
            mie_sums<2, NJ, CT>(a.D[2], a.dD[2], a.nb[2], rows, used, lane, L.lqg,
                                [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); },
                                A, B, E, M, V);
            finish(2, L.lqg, L.rg, ze_g);
        }
        if (!want.all) continue;                                     // wave-uniform: one species' own profiles alone
        // the tail once in the code, channel after channel: the channel's registers are picked by wave-uniform selects
#pragma unroll 1
        for (int cc = 0; cc < used; ++cc) {
            double zr[NJ], zs[NJ], zg[NJ], ex[NJ], w1[NJ], v1[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                zr[j] = ze_r[0][j]; zs[j] = ze_s[0][j]; zg[j] = ze_g[0][j]; ex[j] = ext[0][j]; w1[j] = zw[0][j]; v1[j] = zv[0][j];
#pragma unroll
                for (int u = 1; u < CT; ++u)
                    if (u == cc) { zr[j] = ze_r[u][j]; zs[j] = ze_s[u][j]; zg[j] = ze_g[u][j]; ex[j] = ext[u][j]; w1[j] = zw[u][j]; v1[j] = zv[u][j]; }
            }
            const int ci = c0 + cc;
            const MieChannel<T> ch{a.out, int64_t(ci) * a.prof_ch_stride, a.pia_total ? a.pia_total + int64_t(ci) * a.col_ch_stride : nullptr,
                                   a.k_gas ? a.k_gas + int64_t(ci) * a.k_gas_ch_stride + col * a.k_gas_col_stride : nullptr, a.kc[ci], a.rho_w[ci]};
            mie_tail<T, NJ>(a, ch, want, col, base, nz, lane, L, zr, zs, zg, ex, w1, v1);
        }
    }
}

// One wavefront per column: nch channels of the radiometer (include/kidmp_multichannel.h).  The load is formed once; the
// channels are taken in tiles of CT, and per tile and species one walk over the bins forms every density once and folds
// it into the sums of the tile's channels (radiometer_sums).  What stays alive per channel across the species is k_abs and
// k_bsc; radiometer_tail then runs per channel as in k_radiometer, so slab c of every output holds k_radiometer's bits
// for channel c's table, closure and k_gas.  No atomics, no scratch.
template <class T, int NJ, int CT>
__global__ void __launch_bounds__(REFL_THREADS)
k_radiometer_multi(ReflConsts c, DopplerConsts dc, RadiometerMultiArgs<T> a, int64_t ncol, int nz)
{
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);

    ChannelLevels<NJ> L;
    load_channel_levels<NJ>(c, dc, a, base, nz, lane, L);
    double rr[NJ];
    rain_mass<NJ>(a, base, lane, L, rr);

    for (int c0 = 0; c0 < a.nch; c0 += CT) {
        const int used = a.nch - c0 < CT ? a.nch - c0 : CT;
        double kabs[CT][NJ], kbsc[CT][NJ];
#pragma unroll
        for (int cc = 0; cc < CT; ++cc)
#pragma unroll
            for (int j = 0; j < NJ; ++j) kabs[cc][j] = kbsc[cc][j] = 0.;
        {
            double A[CT][NJ], S[CT][NJ], M[NJ];
            const double *rows[CT];
            const auto rows_of = [&](int x) __attribute__((always_inline)) {
#pragma unroll
                for (int cc = 0; cc < CT; ++cc) rows[cc] = a.rows[c0 + (cc < used ? cc : 0)][x];
            };
            const auto finish = [&](const bool (&has)[NJ], const double (&rq)[NJ]) __attribute__((always_inline)) {
#pragma unroll
                for (int cc = 0; cc < CT; ++cc)
                    if (cc < used) radiometer_species_finish<NJ>(has, rq, A[cc], S[cc], M, kabs[cc], kbsc[cc]);
            };
            rows_of(0);
            radiometer_sums<0, NJ, CT>(a.D[0], a.dD[0], a.nb[0], rows, used, lane, L.lqr,
                                       [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_r[j], L.lamr[j], D, dD); }, A, S, M);
            finish(L.lqr, rr);
            rows_of(1);
            radiometer_sums<1, NJ, CT>(a.D[1], a.dD[1], a.nb[1], rows, used, lane, L.lqs,
                                       [&](int j, double D, double dD, double Dmu) __attribute__((always_inline)) { return lvl::snow_bin(L.ss[j], D, Dmu, dD); }, A, S, M);
            finish(L.lqs, L.rs);
            rows_of(2);
            radiometer_sums<2, NJ, CT>(a.D[2], a.dD[2], a.nb[2], rows, used, lane, L.lqg,
                                       [&](int j, double D, double dD, double) __attribute__((always_inline)) { return lvl::exp_bin(L.N0_g[j], L.lamg[j], D, dD); }, A, S, M);
            finish(L.lqg, L.rg);
        }
        // the tail once in the code, channel after channel: the channel's registers are picked by wave-uniform selects
#pragma unroll 1
        for (int cc = 0; cc < used; ++cc) {
            double ka[NJ], kb[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                ka[j] = kabs[0][j]; kb[j] = kbsc[0][j];
#pragma unroll
                for (int u = 1; u < CT; ++u)
                    if (u == cc) { ka[j] = kabs[u][j]; kb[j] = kbsc[u][j]; }
            }
            const int ci = c0 + cc;
            const int64_t cslab = int64_t(ci) * a.col_ch_stride;
            const RadChannel<T> ch{a.out, int64_t(ci) * a.prof_ch_stride, a.tb_toa ? a.tb_toa + cslab : nullptr,
                                   a.tb_ground ? a.tb_ground + cslab : nullptr, a.tau_abs ? a.tau_abs + cslab : nullptr,
                                   a.k_gas ? a.k_gas + int64_t(ci) * a.k_gas_ch_stride + col * a.k_gas_col_stride : nullptr,
                                   a.kc[ci], a.rho_w[ci], a.mu[ci], a.emissivity[ci], a.t_cosmic[ci]};
            radiometer_tail<T, NJ>(a, ch, col, base, nz, lane, L, ka, kb);
        }
    }
}

namespace {

// The channels one pass carries, by the number of level groups.  Every channel place of a tile costs about half a
// single-channel launch whether a channel fills it or not, and registers beyond 256 cost the second wave per SIMD, so the
// tile is not the widest that fits: at two level groups 4 (radiometer) and 3 (radar) were the fastest of the candidates
// measured, the other counts follow the compiler's report.  No instantiation has scratch; the
// radar's NJ = 3 takes 2 because 3 needs 64 AGPRs, NJ = 4 takes 3 because 2 is the one candidate the compiler spilled.
constexpr int rad_tile(int) { return 4; }
constexpr int mie_tile(int nj) { return nj == 3 ? 2 : 3; }
int multichannel_tile(int which, int nz)
{
    const int nj = (nz + 63) / 64;
    if (nj < 1 || nj > 4 || (which != 0 && which != 1)) return 0;
    return which == 0 ? rad_tile(nj) : mie_tile(nj);
}

template <class T>
hipError_t launch_radiometer_multi(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const RadiometerMultiArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // an empty batch is not looked at
    if (a.nch < 1 || a.nch > MC_MAX_CHANNELS) return hipErrorInvalidValue;
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_radiometer_multi<T, NJ, rad_tile(NJ)>), column_grid(ncol), dim3(REFL_THREADS), 0, s,
                           c, dc, a, ncol, nz);
    });
}
template <class T>
hipError_t launch_mie_radar_multi(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const MieMultiArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // an empty batch is not looked at
    if (a.nch < 1 || a.nch > MC_MAX_CHANNELS) return hipErrorInvalidValue;
    for (int x = 0; x < MIE_NSPEC; ++x)
        if (a.nb[x] < 1 || a.nb[x] > MIE_MAX_BINS) return hipErrorInvalidValue;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_mie_radar_multi<T, NJ, mie_tile(NJ)>), column_grid(ncol), dim3(REFL_THREADS), 0, s,
                           c, dc, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

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
