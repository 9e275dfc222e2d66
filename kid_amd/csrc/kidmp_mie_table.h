// kidmp_mie_table.h -- what the table objects of include/kidmp_mie.h and include/kidmp_radiometer.h share: the check of a
// kidmp_mie_cfg, the choice of the grids, and one device buffer that holds per species D[nb], dD[nb], rows[nrows][nb].
#pragma once

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kidmp_ctx.h"
#include "kidmp_mie_sphere.h"
#include "../../include/kidmp_mie.h"

namespace kidmp {
constexpr int MIE_NSPEC = 3, MIE_MAX_BINS = 256;           // rain, snow, graupel; the bins a species' table may have

struct MieTableData {
    kidmp_ctx *ctx;
    int device;
    kidmp_mie_cfg cfg;
    int32_t nb[MIE_NSPEC];
    size_t off[MIE_NSPEC];                                // the species' first double in the buffer
    double *d_buf;
    double kc;
    int nrows;
    double *h_buf;                                        // the host's copy of d_buf: what a channel set compares
};

}  // namespace kidmp

// the handles of include/kidmp_mie.h and include/kidmp_radiometer.h: one device buffer, per species D[nb], dD[nb], rows[nrows][nb]
struct kidmp_mie_table : kidmp::MieTableData {};
struct kidmp_radiometer_table : kidmp::MieTableData {};

namespace kidmp {

inline const double *mie_bins_D(const Bins &b, int x) { return x == 0 ? b.Dr : x == 1 ? b.Ds : b.Dg; }
inline const double *mie_bins_dD(const Bins &b, int x) { return x == 0 ? b.dtr : x == 1 ? b.dts : b.dtg; }

// nullptr where the configuration is good, else what is wrong with it
inline const char *mie_bad_cfg(const kidmp_mie_cfg &g)
{
    const double members[] = {g.wavelength, g.eps_w_re, g.eps_w_im, g.eps_i_re, g.eps_i_im, g.rho_w, g.rho_i, g.kw2};
    for (double m : members)
        if (!std::isfinite(m)) return "a member of the configuration is not finite";
    if (!(g.wavelength > 0.) || !(g.rho_w > 0.) || !(g.rho_i > 0.) || !(g.kw2 > 0.)) return "wavelength, rho_w, rho_i and kw2 must be above 0";
    if (g.eps_w_im < 0. || g.eps_i_im < 0.) return "Im(eps) must not be below 0";
    if ((g.eps_w_im == 0. && !(g.eps_w_re > 0.)) || (g.eps_i_im == 0. && !(g.eps_i_re > 0.))) return "a real permittivity must be above 0";
    return nullptr;
}
inline MieCfg mie_model_cfg(const kidmp_mie_cfg &g) { return MieCfg{g.wavelength, {g.eps_w_re, g.eps_w_im}, {g.eps_i_re, g.eps_i_im}, g.rho_w, g.rho_i, g.kw2}; }

// Builds the rows on the host with bins(cfg, species, nb, D, rows) and uploads them; *out is written on success alone.
template <class BinsFn>
int mie_table_build(kidmp_ctx *ctx, const std::string &w, const kidmp_mie_cfg *cfg, const kidmp_mie_grids *grids, int nrows, BinsFn &&bins,
                    MieTableData *out)
{
    kidmp_mie_cfg g;
    if (cfg) g = *cfg;
    else kidmp_mie_defaults(&g);
    if (const char *bad = mie_bad_cfg(g)) return fail(ctx, KIDMP_EINVAL, w + ": " + bad);
    int32_t nb[MIE_NSPEC];
    size_t off[MIE_NSPEC], total = 0;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC];
    for (int x = 0; x < MIE_NSPEC; ++x) {
        nb[x] = nbins;
        D[x] = mie_bins_D(ctx->hb, x);
        dD[x] = mie_bins_dD(ctx->hb, x);
        if (grids && (grids->D[x] || grids->dD[x])) {
            if (!grids->D[x] || !grids->dD[x]) return fail(ctx, KIDMP_EINVAL, w + ": a grid needs both D and dD");
            if (grids->nb[x] < 1 || grids->nb[x] > KIDMP_MIE_MAX_BINS) return fail(ctx, KIDMP_EINVAL, w + ": nb outside [1, KIDMP_MIE_MAX_BINS]");
            nb[x] = grids->nb[x]; D[x] = grids->D[x]; dD[x] = grids->dD[x];
            for (int b = 0; b < nb[x]; ++b)
                if (!std::isfinite(dD[x][b])) return fail(ctx, KIDMP_EINVAL, w + ": a dD is not finite");
        }
        off[x] = total;
        total += size_t(2 + nrows) * size_t(nb[x]);
    }
    std::vector<double> buf(total);
    const MieCfg mc = mie_model_cfg(g);
    for (int x = 0; x < MIE_NSPEC; ++x) {
        double *b = buf.data() + off[x];
        std::memcpy(b, D[x], size_t(nb[x]) * sizeof(double));
        std::memcpy(b + nb[x], dD[x], size_t(nb[x]) * sizeof(double));
        if (!bins(mc, x, nb[x], D[x], b + 2 * size_t(nb[x])))
            return fail(ctx, KIDMP_EINVAL, w + ": a diameter is not finite or not above 0, or its sphere has more than 1e7 terms");
    }
    GUARD(ctx);
    double *d_buf = nullptr;
    HIPTRY(ctx, hipMalloc(reinterpret_cast<void **>(&d_buf), total * sizeof(double)));
    const hipError_t e = hipMemcpy(d_buf, buf.data(), total * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_buf); return hipfail(ctx, e, "hipMemcpy of the table"); }
    double *h_buf = new double[total];
    std::memcpy(h_buf, buf.data(), total * sizeof(double));
    *out = MieTableData{ctx, ctx->cfg.device, g, {nb[0], nb[1], nb[2]}, {off[0], off[1], off[2]}, d_buf, mie_cloud_absorption(mc), nrows, h_buf};
    return KIDMP_OK;
}

inline void mie_table_free(MieTableData *t)
{
    DeviceGuard guard(t->device);
    if (t->d_buf) (void)hipFree(t->d_buf);
    delete[] t->h_buf;
}

inline int mie_table_read(const MieTableData *table, const std::string &w, int32_t species, int32_t *nb, double *D, double *dD, double *rows,
                          kidmp_mie_cfg *cfg)
{
    kidmp_ctx *ctx = table->ctx;
    if (species < 0 || species >= MIE_NSPEC) return fail(ctx, KIDMP_EINVAL, w + ": unknown species");
    const size_t n = size_t(table->nb[species]);
    if (nb) *nb = table->nb[species];
    if (cfg) *cfg = table->cfg;
    DeviceGuard guard(table->device);
    if (guard.err != hipSuccess) return hipfail(ctx, guard.err, "hipSetDevice");
    const double *b = table->d_buf + table->off[species];
    if (D) HIPTRY(ctx, hipMemcpy(D, b, n * sizeof(double), hipMemcpyDeviceToHost));
    if (dD) HIPTRY(ctx, hipMemcpy(dD, b + n, n * sizeof(double), hipMemcpyDeviceToHost));
    if (rows) HIPTRY(ctx, hipMemcpy(rows, b + 2 * n, size_t(table->nrows) * n * sizeof(double), hipMemcpyDeviceToHost));
    return KIDMP_OK;
}

}  // namespace kidmp
