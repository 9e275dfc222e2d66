/*
 * kidmp_summary.h -- per-column summaries on the device: water paths, cloud optical depth, echo and cloud heights.
 *
 * One number per column per step is what KiD reports as time series and what the reference's adapter saves as its own
 * per-column scalars (W:155-192, W:248-303).  kidmp_column_summary_device forms KIDMP_SUMMARY_N = 16 doubles per column
 * from one read of the column's profiles, without a download and without writing a profile: the per-level reflectivity
 * and cloud-water radius are those of kidmp_reflectivity_device and kidmp_effective_radii_device, bit for bit, and stay
 * in registers.  Conventions as in kidmp.h (return codes, device binding, [ncol][nz] arrays with k fastest, k = 0 the
 * lowest level).
 *
 * With rho_k = 0.622 p / (R T (qv' + 0.622)), qv' = max(1e-10, qv) (the density of the column step and of
 * calc_refl10cm, M:1389-1391 and M:4995-4997), summary[col][slot] is
 *
 *    0 WVP           sum_k (rho_k qv'_k) dz_k                                                        kg m-2
 *    1 CWP           sum_k (rho_k qc_k) dz_k      values as stored, no threshold
 *    2 RWP           the same for qr
 *    3 IWP           the same for qi
 *    4 SWP           the same for qs
 *    5 GWP           the same for qg
 *    6 TAU_C         liquid cloud optical depth: the sum over the levels where calc_effectRad forms re_qc (not cycled
 *                    at M:4874) of (1.5 cw_k) / (1000.0 re_qc_k), cw_k the CWP term; re_qc_k as the library forms it
 *                    (its density with the unclamped qv, M:4860; Nt_c of the context or the bound per-column value)
 *    7 DBZ_MAX       max_k dBZ_k (composite reflectivity)
 *    8 Z_DBZ_MAX     mid-height of the lowest level that attains slot 7                              m
 *    9 Z_ECHO_TOP    top-face height of the highest level with dBZ_k >= dbz_echo
 *   10 DBZ_SFC       dBZ of level 0
 *   11 Z_CLOUD_BASE  bottom-face height of the lowest level with qc_k + qi_k > q_cloud
 *   12 Z_CLOUD_TOP   top-face height of the highest such level
 *   13 N_CLOUD       the number of such levels, as a double (0.0 when there is none)
 *   14 Z_FREEZE      mid-height of the lowest level with T_k < t_freeze
 *   15 reserved      +0.0
 *
 * Heights: the bottom face of level k is zb(k) = sum_{k' < k} dz_k' (0 for k = 0), its top face sum_{k' <= k} dz_k',
 * its middle zb(k) + 0.5 dz_k.  dz must be positive: stated, not checked.  A slot whose level does not exist holds a
 * quiet NaN (kidmp_level_stats_device leaves it out of the moments and counts it in its NaN slot).  Species the context
 * may omit (qi, qs, qg in an iiwarm context) count as exact zeros: their paths are +0.0.  Inputs are assumed finite; a
 * NaN input is memory-safe and gives unspecified values.
 *
 * Order of the sums: every sum and the maximum run in a fixed order that is a pure function of nz, so a column gives
 * the same bits alone, at any position in any batch and on a repeated call.
 */
#ifndef KIDMP_SUMMARY_H
#define KIDMP_SUMMARY_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_SUMMARY_N 16
enum { KIDMP_SUM_WVP = 0, KIDMP_SUM_CWP, KIDMP_SUM_RWP, KIDMP_SUM_IWP, KIDMP_SUM_SWP, KIDMP_SUM_GWP,
       KIDMP_SUM_TAU_C, KIDMP_SUM_DBZ_MAX, KIDMP_SUM_Z_DBZ_MAX, KIDMP_SUM_Z_ECHO_TOP, KIDMP_SUM_DBZ_SFC,
       KIDMP_SUM_Z_CLOUD_BASE, KIDMP_SUM_Z_CLOUD_TOP, KIDMP_SUM_N_CLOUD, KIDMP_SUM_Z_FREEZE };

/* The thresholds of slots 9 and 11-14.  A NULL cfg means { 18.0, 1.0e-5, 273.15 }: conventions of this library (an
 * 18 dBZ echo top, 0.01 g/kg of cloud condensate, 0 C); the reference has none. */
typedef struct kidmp_summary_cfg { double dbz_echo, q_cloud, t_freeze; } kidmp_summary_cfg;

/* summary[ncol][KIDMP_SUMMARY_N], binary64 in all four entries.  The kidmp32_ forms take binary32 inputs, widen every
 * value on load, run the same code and round nothing.
 *   dz, dz_col_stride   element (col, k) = dz[col*dz_col_stride + k]; 0 = one profile of nz values shared by all columns
 *                       (KiD's own dz), otherwise >= nz (the step's [ncol][nz] array and profile 14 of the KiD
 *                       workspace: nz)
 *   nc                  may be NULL unless the context is aerosol-aware
 *   qi; qs with qg      may be NULL in an iiwarm context, required in a mixed-phase one
 * A per-column droplet number bound with kidmp_set_column_nc is honoured in slot 6; ncol must then be the bound count.
 * The device entries never allocate, never synchronise and enqueue one launch on `stream`: they can be captured into a
 * hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on its
 * compute stream, then synchronise; their results equal the device entry's bit for bit for any chunking
 * (kidmp_set_host_chunk).
 * KIDMP_EINVAL, nothing written: a required NULL, nz outside [2, KIDMP_MAX_NZ], ncol < 0, dz_col_stride neither 0 nor
 * >= nz, a threshold that is not finite, a pointer that is not memory of the context's device (device entries), ncol
 * other than the bound count.  A NULL context returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_column_summary_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *nc,
        const double *qi, const double *qr, const double *nr, const double *qs, const double *qg,
        const double *dz, int64_t dz_col_stride, const kidmp_summary_cfg *cfg,
        double *summary, void *stream);
int kidmp32_column_summary_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *nc,
        const float *qi, const float *qr, const float *nr, const float *qs, const float *qg,
        const float *dz, int64_t dz_col_stride, const kidmp_summary_cfg *cfg,
        double *summary, void *stream);
int kidmp_column_summary_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *nc,
        const double *qi, const double *qr, const double *nr, const double *qs, const double *qg,
        const double *dz, int64_t dz_col_stride, const kidmp_summary_cfg *cfg,
        double *summary);
int kidmp32_column_summary_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *nc,
        const float *qi, const float *qr, const float *nr, const float *qs, const float *qg,
        const float *dz, int64_t dz_col_stride, const kidmp_summary_cfg *cfg,
        double *summary);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_SUMMARY_H */
