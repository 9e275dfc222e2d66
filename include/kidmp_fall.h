/*
 * kidmp_fall.h -- block-O fall speeds and precipitation-flux profiles on the device.
 *
 * How fast each species falls and how much precipitation crosses each level is what every KiD comparison plots, and
 * what the reference means to save as 'total_ppt_level' (W:305-307; the assignments are commented out, M:3394-3398 and
 * W:189-191).  kidmp_fall_speeds_device forms block O (M:3206-3354) of a state in one launch, as a diagnostic in the
 * way kidmp_reflectivity_device is one.  Conventions as in kidmp.h (return codes, device binding, [ncol][nz] arrays
 * with k fastest, k = 0 the lowest level).  In binary64, in the reference's order of operations:
 *
 *   load      rho from qv' = max(1e-10, qv) (M:1389-1391); rain, ice, snow and graupel as mp_thompson loads them
 *             (M:1420-1492), with the number limiting of ice (M:1424-1438) and rain (M:1451-1467); an absent species
 *             (q <= R1) has r = R1 and n = R2.  qc is not read.  The input arrays are never written.
 *   moments   snow's smob and smoc of block D (M:1545-1628); graupel's slope of block E (M:1633-1654), with the running
 *             minimum of the intercept from the top down.
 *   speeds    rhof = sqrt(RHO_NOT/rho); rain vt_r, vt_nr (M:3221-3237); ice vt_i, vt_ni (M:3256-3269); snow vt_s with
 *             the above-freezing form that reads the rain speed of the level (M:3288-3308); graupel vt_g with
 *             MAX(vtg, vtrk) above T_0 (M:3325-3334).  A level whose species fails its `> R1` test takes the value of
 *             the level above, bit for bit; the value above the top level is 0.
 *   fluxes    flux_x(k) = vt_x(k) * r_x(k) (M:3368 and its siblings; R1 where the species is absent), kg m-2 s-1;
 *             flux_total = ((flux_r + flux_i) + flux_s) + flux_g.
 *   nstep     per species MAX_k INT(dt/(dz_k/v_k) + 1.) over the levels with v_k > 1.E-3 (rain: v = MAX(vt_r, vt_nr));
 *             a count of 0 is reported as 1, as NINT(1./onstep) gives it; capped at 10 000.  [ncol][4] int32 in the
 *             order of the step's own nstep: rain, ice, snow, graupel.
 *
 * vts_boost is the one input block O takes from the rate sweep: an optional profile [ncol][nz].  NULL means the value
 * of a level without riming: 1.0 where T < T_0 (M:2027), 1.5 elsewhere (M:1751).  A caller who knows the riming ratio
 * passes MIN(1.5, 1.1 + (r_frac-2.)*.016) (M:2228) itself.  The result is what the step's sedimentation would use on a
 * state that blocks G-N leave alone.  It is NOT a replay of a particular step, whose speeds are formed from the
 * provisional tau+1 state.
 *
 * An iiwarm context: qi, ni, qs, qg (and vts_boost) are not read and may be NULL; the frozen speeds and fluxes are
 * exact +0.0 (M:3346-3352) and their output pointers may be NULL; flux_total = flux_r; the frozen nstep entries are 1.
 * A per-column droplet number bound with kidmp_set_column_nc is neither read nor checked.  A column gives the same bits
 * alone, at any position in any batch and on a repeated call.  Inputs are assumed finite and dz positive; a NaN input
 * is memory-safe and gives unspecified values.
 */
#ifndef KIDMP_FALL_H
#define KIDMP_FALL_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Each member is [ncol][nz] or NULL (not wanted: it costs no store).  At least one member or nstep must be asked for.
 * kidmp32_fall_out: binary64 inside, one rounding on store. */
typedef struct kidmp_fall_out { double *vt_r, *vt_nr, *vt_i, *vt_ni, *vt_s, *vt_g, *flux_r, *flux_i, *flux_s, *flux_g, *flux_total; } kidmp_fall_out;
typedef struct kidmp32_fall_out { float *vt_r, *vt_nr, *vt_i, *vt_ni, *vt_s, *vt_g, *flux_r, *flux_i, *flux_s, *flux_g, *flux_total; } kidmp32_fall_out;

/*   dz, dz_col_stride, dt   read only when nstep != NULL.  Element (col, k) = dz[col*dz_col_stride + k]; 0 = one profile
 *                           of nz values shared by all columns, otherwise >= nz; dt > 0
 *   out                     may be NULL when nstep is asked for
 * The device entries never allocate, never synchronise and enqueue one launch on `stream`: they can be captured into a
 * hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on its
 * compute stream, then synchronise; only the requested profiles cross PCIe, and the results equal the device entry's
 * bit for bit for any chunking (kidmp_set_host_chunk).
 * KIDMP_EINVAL, nothing written: a required NULL (t, p, qv, qr, nr), nz outside [2, KIDMP_MAX_NZ], ncol < 0, nothing
 * requested at all, a frozen input (qi, ni, qs, qg) missing in a mixed-phase context, nstep requested with dz NULL,
 * dt <= 0 or a dz_col_stride that is neither 0 nor >= nz, a pointer that is not memory of the context's device (device
 * entries).  A NULL context returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_fall_speeds_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qi, const double *ni, const double *qs, const double *qg, const double *vts_boost,
        const double *dz, int64_t dz_col_stride, double dt,
        const kidmp_fall_out *out, int32_t *nstep, void *stream);
int kidmp32_fall_speeds_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qi, const float *ni, const float *qs, const float *qg, const float *vts_boost,
        const float *dz, int64_t dz_col_stride, double dt,
        const kidmp32_fall_out *out, int32_t *nstep, void *stream);
int kidmp_fall_speeds_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qi, const double *ni, const double *qs, const double *qg, const double *vts_boost,
        const double *dz, int64_t dz_col_stride, double dt,
        const kidmp_fall_out *out, int32_t *nstep);
int kidmp32_fall_speeds_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qi, const float *ni, const float *qs, const float *qg, const float *vts_boost,
        const float *dz, int64_t dz_col_stride, double dt,
        const kidmp32_fall_out *out, int32_t *nstep);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_FALL_H */
