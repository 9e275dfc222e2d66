/*
 * kidmp_multichannel.h -- several channels of the radiometer (kidmp_radiometer.h) or of the cloud radar (kidmp_mie.h) in
 * one launch.
 *
 * A microwave imager has nine to thirteen channels and a dual-frequency radar two; the expensive part of either operator,
 * the densities n = N_x(D_b)*dD_b of every level, species and bin, does not depend on the wavelength.  A channel set is 1
 * to KIDMP_MAX_CHANNELS existing tables of one context, all on the same diameter grids, passed as an array of handles; no
 * new table object.  One launch forms the load, the running minimum and the densities once and folds each bin into the
 * sums of every channel; what follows the sums runs per channel exactly as in the single-channel kernel.  The channels are
 * taken kidmp_multichannel_tile() at a time inside the launch; each further tile forms the densities again and nothing
 * else.
 *
 * The contract: slab c of every output holds the bits that kidmp[32]_radiometer_device / kidmp[32]_mie_radar_device writes
 * for the same state with tables[c], rcfg[c] and channel c's k_gas.  Those bits do not depend on nch, on the channel's
 * position in the list, on which other tables are in it, on the tile, on the batch or on the requested outputs.  The same
 * table may appear twice.  (The library is built without contraction; per channel and bin the operations are the
 * single-channel kernel's in their order, the accumulators start at +0.0 per species, the bins are walked ascending.  The
 * rows that do not depend on the wavelength -- mass; s_ray, mass, v0 -- are read from one table of the set and must be
 * equal bit for bit across it.)
 *
 * Shapes.  tables is [nch].  rcfg is NULL (the defaults for every channel) or [nch].  k_gas is NULL (zero) or per channel:
 * channel c starts at k_gas + c*k_gas_ch_stride, a stride of 0 is one profile (set) for all channels; inside a channel
 * k_gas_col_stride is the single-channel entries' (0: one profile [nz] for all columns, else >= nz).  A
 * k_gas_ch_stride other than 0 must hold one channel's profiles: >= nz with a column stride of 0, else
 * >= (ncol-1)*k_gas_col_stride + nz.  t_sfc, dz and w are shared by the channels.  out is the single-channel struct; each
 * member is NULL or an array with a leading channel dimension: profiles [nch][ncol][nz]; tb_toa, tb_ground, tau_abs,
 * pia_total [nch][ncol].
 *
 * Everything else is as the single-channel entries document it: the NULL rules for qc, qs, qg and dz, an iiwarm context
 * without snow and graupel, a request for k_abs, k_bsc alone without layer and scan, a radar request without path outputs
 * without scan, a request for one species' own radar profiles walking that species alone.  Device entries never allocate,
 * never synchronise and enqueue exactly one launch on `stream`; host entries run chunks of columns through the context's
 * staging memory (the chunk of kidmp_set_host_chunk or the default, narrowed where nch slabs of it would pass 1 GiB) and
 * equal the device entry bit for bit for any chunk.
 *
 * KIDMP_EINVAL, nothing written: nch outside [1, KIDMP_MAX_CHANNELS]; tables NULL or one of its entries NULL; a table of
 * another context; tables whose grids differ in any nb, D or dD bit of a species, or whose wavelength-independent rows
 * differ in a bit (tables built with different rho_w); a k_gas_ch_stride that is neither 0 nor large enough; a bad member
 * of any rcfg[c]; everything the single-channel entries refuse.  KIDMP_ESTATE as there.  ncol == 0 returns KIDMP_OK.
 *
 * Not modelled: a dual-wavelength ratio (it is dbz[i] - dbz[j] on the result), channels of the polarimetric radar, the
 * lidar or the bright band, radar and radiometer channels mixed in one launch.
 */
#ifndef KIDMP_MULTICHANNEL_H
#define KIDMP_MULTICHANNEL_H

#include "kidmp_radiometer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_MAX_CHANNELS 16

/* How many channels one pass of the kernel carries at nz levels; which: 0 the radiometer, 1 the radar.  A pure host
 * function that needs no context; 0 for an unknown `which` or nz outside [1, KIDMP_MAX_NZ]. */
int32_t kidmp_multichannel_tile(int32_t which, int32_t nz);

int kidmp_radiometer_multi_device(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
        int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride,
        const double *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const double *t_sfc, const kidmp_radiometer_out *out, void *stream);
int kidmp32_radiometer_multi_device(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
        int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride,
        const float *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const float *t_sfc, const kidmp32_radiometer_out *out, void *stream);
int kidmp_radiometer_multi_host(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
        int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride,
        const double *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const double *t_sfc, const kidmp_radiometer_out *out);
int kidmp32_radiometer_multi_host(kidmp_ctx *ctx, const kidmp_radiometer_table *const *tables, int32_t nch, const kidmp_radiometer_cfg *rcfg,
        int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride,
        const float *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const float *t_sfc, const kidmp32_radiometer_out *out);

int kidmp_mie_radar_multi_device(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const double *w,
        const double *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const kidmp_mie_out *out, void *stream);
int kidmp32_mie_radar_multi_device(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const float *w,
        const float *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const kidmp32_mie_out *out, void *stream);
int kidmp_mie_radar_multi_host(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const double *w,
        const double *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const kidmp_mie_out *out);
int kidmp32_mie_radar_multi_host(kidmp_ctx *ctx, const kidmp_mie_table *const *tables, int32_t nch, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const float *w,
        const float *k_gas, int64_t k_gas_col_stride, int64_t k_gas_ch_stride, const kidmp32_mie_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_MULTICHANNEL_H */
