// kidmp_channel_call.h -- what the entries of include/kidmp_mie.h, include/kidmp_radiometer.h and
// include/kidmp_multichannel.h share: the arguments of a call gathered into one struct, and what the device and the host
// entries check alike before anything is touched.
#pragma once

#include <cmath>
#include <string>

#include "kidmp_column.h"
#include "kidmp_mie_table.h"
#include "../../include/kidmp_radiometer.h"

namespace kidmp {
constexpr int NIN = 8, NREQ = 5;                          // t, p, qv, qr, nr | qc, qs, qg
inline constexpr const char *IN_NAMES[NIN] = {"t", "p", "qv", "qr", "nr", "qc", "qs", "qg"};

// ---- the cloud radar ----
// out in the order of kidmp_mie_out; a table has MIE_NROWS rows per diameter bin
constexpr int MIE_NOUT = 13, MIE_NROWS = 5;
constexpr int MIE_DBZ = 0, MIE_DBZ_UP = 1, MIE_DBZ_DOWN = 2, MIE_DBZ_X = 3, MIE_MIE_X = 6, MIE_EXT = 9, MIE_PIA_UP = 10, MIE_PIA_DOWN = 11, MIE_VD = 12;
inline constexpr const char *MIE_OUT_NAMES[MIE_NOUT] = {"dbz", "dbz_up", "dbz_down", "dbz_r", "dbz_s", "dbz_g", "mie_r", "mie_s", "mie_g", "ext",
                                         "pia_up", "pia_down", "vd"};

template <class T> struct MieCall {
    const T *in[NIN];
    const T *dz, *w, *k_gas;
    int64_t dz_col_stride, k_gas_col_stride;
    T *out[MIE_NOUT];
    T *pia_total;
};
template <class T, class O>
MieCall<T> mie_call(const T *t, const T *p, const T *qv, const T *qc, const T *qr, const T *nr, const T *qs, const T *qg, const T *dz,
                    int64_t dz_col_stride, const T *w, const T *k_gas, int64_t k_gas_col_stride, const O *out)
{
    MieCall<T> c{{t, p, qv, qr, nr, qc, qs, qg}, dz, w, k_gas, dz_col_stride, k_gas_col_stride, {}, nullptr};
    if (out) {
        T *const o[MIE_NOUT] = {out->dbz, out->dbz_up, out->dbz_down, out->dbz_r, out->dbz_s, out->dbz_g, out->mie_r, out->mie_s, out->mie_g,
                                out->ext, out->pia_up, out->pia_down, out->vd};
        for (int v = 0; v < MIE_NOUT; ++v) c.out[v] = o[v];
        c.pia_total = out->pia_total;
    }
    return c;
}
template <class T> bool needs_path(const MieCall<T> &a)
{ return a.out[MIE_DBZ_UP] || a.out[MIE_DBZ_DOWN] || a.out[MIE_PIA_UP] || a.out[MIE_PIA_DOWN] || a.pia_total; }

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_mie(kidmp_ctx *ctx, const char *who, const kidmp_mie_table *tab, int64_t ncol, int32_t nz, const MieCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (!tab || tab->ctx != ctx) return fail(ctx, KIDMP_EINVAL, w + ": the table is NULL or belongs to another context");
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (a.dz_col_stride != 0 && a.dz_col_stride < nz) return fail(ctx, KIDMP_EINVAL, w + ": dz_col_stride must be 0 or >= nz");
    if (a.k_gas_col_stride != 0 && a.k_gas_col_stride < nz) return fail(ctx, KIDMP_EINVAL, w + ": k_gas_col_stride must be 0 or >= nz");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = a.pia_total != nullptr;
    for (int v = 0; v < MIE_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: out is NULL or every member is");
    for (int v = 0; v < NREQ; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (needs_path(a) && !a.dz) return fail(ctx, KIDMP_EINVAL, w + ": path integrals need dz");
    if (!doppler_consts_supported(ctx->hc) || !spectra_consts_supported(ctx->hc))
        return fail(ctx, KIDMP_ESTATE, w + ": exponents differ from the kernel's");
    return KIDMP_OK;
}

// The arrays of a host entry (kidmp_stage_plan.h), of one channel (nch = 1, k_gas_ch_stride = 0) or of a set: every output
// has nch slabs, k_gas one per channel where the channels have profiles of their own.  Only what the kernel reads goes up.
constexpr int MIE_A_DZ = NIN, MIE_A_W = NIN + 1, MIE_A_KGAS = NIN + 2, MIE_A_OUT = NIN + 3, MIE_A_PIA = MIE_A_OUT + MIE_NOUT,
              MIE_NARRAYS = MIE_A_PIA + 1;
template <class T>
void mie_stage_list(const kidmp_ctx *ctx, StageArray (&a)[MIE_NARRAYS], int64_t ncol, int32_t nz, const MieCall<T> &h, int32_t nch,
                    int64_t k_gas_ch_stride)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    for (int v = 0; v < NIN; ++v) a[v] = stage_array(warm && v >= 6 ? nullptr : h.in[v], nz, STAGE_UP);
    a[MIE_A_DZ] = stage_rows(needs_path(h) ? h.dz : nullptr, nz, h.dz_col_stride);
    a[MIE_A_W] = stage_array(h.w, nz, STAGE_UP);
    a[MIE_A_KGAS] = stage_slabs(stage_rows(h.k_gas, nz, h.k_gas_col_stride), k_gas_ch_stride ? nch : 1, k_gas_ch_stride);
    for (int v = 0; v < MIE_NOUT; ++v) a[MIE_A_OUT + v] = stage_slabs(stage_array(h.out[v], nz, STAGE_DOWN), nch, ncol * nz);
    a[MIE_A_PIA] = stage_slabs(stage_array(h.pia_total, 1, STAGE_DOWN), nch, ncol);
}
// the call over the slots, once stage_open has made them
template <class T> MieCall<T> mie_staged(const StageArray (&a)[MIE_NARRAYS], int32_t nz, const MieCall<T> &h)
{
    MieCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[v]);
    d.dz = staged<T>(a[MIE_A_DZ]); d.w = staged<T>(a[MIE_A_W]); d.k_gas = staged<T>(a[MIE_A_KGAS]);
    d.dz_col_stride = h.dz_col_stride ? nz : 0;           // staged rows are packed
    d.k_gas_col_stride = h.k_gas_col_stride ? nz : 0;
    for (int v = 0; v < MIE_NOUT; ++v) d.out[v] = staged<T>(a[MIE_A_OUT + v]);
    d.pia_total = staged<T>(a[MIE_A_PIA]);
    return d;
}

// ---- the radiometer ----
constexpr int RAD_NOUT = 6, RAD_NROWS = 3;
constexpr int RAD_K_ABS = 0, RAD_K_BSC = 1, RAD_REFL = 2, RAD_TRANS = 3, RAD_TB_UP = 4, RAD_TB_DOWN = 5;
constexpr int NCOL_OUT = 3;                              // tb_toa, tb_ground, tau_abs
inline constexpr const char *RAD_OUT_NAMES[RAD_NOUT] = {"k_abs", "k_bsc", "refl", "trans", "tb_up", "tb_down"};
inline constexpr const char *RAD_COL_NAMES[NCOL_OUT] = {"tb_toa", "tb_ground", "tau_abs"};

template <class T> struct RadCall {
    const T *in[NIN];
    const T *dz, *k_gas, *t_sfc;
    int64_t dz_col_stride, k_gas_col_stride;
    T *out[RAD_NOUT];
    T *col[NCOL_OUT];
};
template <class T, class O>
RadCall<T> rad_call(const T *t, const T *p, const T *qv, const T *qc, const T *qr, const T *nr, const T *qs, const T *qg, const T *dz,
                    int64_t dz_col_stride, const T *k_gas, int64_t k_gas_col_stride, const T *t_sfc, const O *out)
{
    RadCall<T> c{{t, p, qv, qr, nr, qc, qs, qg}, dz, k_gas, t_sfc, dz_col_stride, k_gas_col_stride, {}, {}};
    if (out) {
        T *const o[RAD_NOUT] = {out->k_abs, out->k_bsc, out->refl, out->trans, out->tb_up, out->tb_down};
        for (int v = 0; v < RAD_NOUT; ++v) c.out[v] = o[v];
        c.col[0] = out->tb_toa; c.col[1] = out->tb_ground; c.col[2] = out->tau_abs;
    }
    return c;
}
template <class T> bool needs_dz(const RadCall<T> &a)
{
    bool any = a.col[0] || a.col[1] || a.col[2];
    for (int v = RAD_REFL; v < RAD_NOUT; ++v) any = any || a.out[v];
    return any;
}

inline kidmp_radiometer_cfg resolve(const kidmp_radiometer_cfg *rcfg)
{
    kidmp_radiometer_cfg r;
    if (rcfg) r = *rcfg;
    else kidmp_radiometer_defaults(&r);
    return r;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_rad(kidmp_ctx *ctx, const char *who, const kidmp_radiometer_table *tab, const kidmp_radiometer_cfg &r, int64_t ncol, int32_t nz,
              const RadCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (!tab || tab->ctx != ctx) return fail(ctx, KIDMP_EINVAL, w + ": the table is NULL or belongs to another context");
    if (!(r.mu > 0. && r.mu <= 1.)) return fail(ctx, KIDMP_EINVAL, w + ": mu outside (0, 1]");
    if (!(r.emissivity >= 0. && r.emissivity <= 1.)) return fail(ctx, KIDMP_EINVAL, w + ": emissivity outside [0, 1]");
    if (!(std::isfinite(r.t_cosmic) && r.t_cosmic >= 0.)) return fail(ctx, KIDMP_EINVAL, w + ": t_cosmic must be finite and not below 0");
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (a.dz_col_stride != 0 && a.dz_col_stride < nz) return fail(ctx, KIDMP_EINVAL, w + ": dz_col_stride must be 0 or >= nz");
    if (a.k_gas_col_stride != 0 && a.k_gas_col_stride < nz) return fail(ctx, KIDMP_EINVAL, w + ": k_gas_col_stride must be 0 or >= nz");
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = false;
    for (int v = 0; v < RAD_NOUT; ++v) any = any || a.out[v];
    for (int v = 0; v < NCOL_OUT; ++v) any = any || a.col[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: out is NULL or every member is");
    for (int v = 0; v < NREQ; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (needs_dz(a) && !a.dz) return fail(ctx, KIDMP_EINVAL, w + ": everything but k_abs and k_bsc needs dz");
    if (!doppler_consts_supported(ctx->hc) || !spectra_consts_supported(ctx->hc))
        return fail(ctx, KIDMP_ESTATE, w + ": exponents differ from the kernel's");
    return KIDMP_OK;
}

// the arrays of a host entry, as mie_stage_list
constexpr int RAD_A_DZ = NIN, RAD_A_KGAS = NIN + 1, RAD_A_OUT = NIN + 2, RAD_A_TSFC = RAD_A_OUT + RAD_NOUT, RAD_A_COL = RAD_A_TSFC + 1,
              RAD_NARRAYS = RAD_A_COL + NCOL_OUT;
template <class T>
void rad_stage_list(const kidmp_ctx *ctx, StageArray (&a)[RAD_NARRAYS], int64_t ncol, int32_t nz, const RadCall<T> &h, int32_t nch,
                    int64_t k_gas_ch_stride)
{
    const bool warm = ctx->cfg.iiwarm != 0;
    for (int v = 0; v < NIN; ++v) a[v] = stage_array(warm && v >= 6 ? nullptr : h.in[v], nz, STAGE_UP);
    a[RAD_A_DZ] = stage_rows(needs_dz(h) ? h.dz : nullptr, nz, h.dz_col_stride);
    a[RAD_A_KGAS] = stage_slabs(stage_rows(h.k_gas, nz, h.k_gas_col_stride), k_gas_ch_stride ? nch : 1, k_gas_ch_stride);
    for (int v = 0; v < RAD_NOUT; ++v) a[RAD_A_OUT + v] = stage_slabs(stage_array(h.out[v], nz, STAGE_DOWN), nch, ncol * nz);
    a[RAD_A_TSFC] = stage_array(h.t_sfc, 1, STAGE_UP);
    for (int v = 0; v < NCOL_OUT; ++v) a[RAD_A_COL + v] = stage_slabs(stage_array(h.col[v], 1, STAGE_DOWN), nch, ncol);
}
template <class T> RadCall<T> rad_staged(const StageArray (&a)[RAD_NARRAYS], int32_t nz, const RadCall<T> &h)
{
    RadCall<T> d{};
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[v]);
    d.dz = staged<T>(a[RAD_A_DZ]); d.k_gas = staged<T>(a[RAD_A_KGAS]); d.t_sfc = staged<T>(a[RAD_A_TSFC]);
    d.dz_col_stride = h.dz_col_stride ? nz : 0;           // staged rows are packed
    d.k_gas_col_stride = h.k_gas_col_stride ? nz : 0;
    for (int v = 0; v < RAD_NOUT; ++v) d.out[v] = staged<T>(a[RAD_A_OUT + v]);
    for (int v = 0; v < NCOL_OUT; ++v) d.col[v] = staged<T>(a[RAD_A_COL + v]);
    return d;
}

}  // namespace kidmp
