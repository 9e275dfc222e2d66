/*
 * kidmp_scan.h -- range-height (RHI) radar scans of an x-z slab: slant beams that cross columns, range gates that are
 * not model levels, attenuation along the beam, beam broadening in elevation and the radial velocity.
 *
 * Every other radar operator of the library points straight up: level k of column c is range gate k.  This one is a
 * geometric operator over [ncol][nz] fields that any of them may have made (kidmp_reflectivity_device,
 * kidmp_doppler_moments_device, kidmp_bright_band_device, kidmp_mie_radar_device, kidmp_polarimetric_device): it samples
 * them at the gate centres of a table of rays in one launch of kidmp::k_scan and returns the sampled cell indices, with
 * which a caller pulls any further field onto the same gates.  THE DEFINITIONS BELOW ARE THE PROJECT'S OWN (nothing in the
 * reference this library was written against corresponds to them): parity with a radar simulator is unpinned.
 * Conventions as in kidmp.h, kidmp_slab.h and kidmp_mie.h (return codes, device binding, [ncol][nz] fields with k fastest
 * and k = 0 the lowest level, ncol = nslab*nx and column s*nx + i cell i of slab s).
 *
 * INPUTS, device memory, never written:
 *   dbz    [ncol][nz]  required: a reflectivity in dBZ
 *   ext    [ncol][nz]  optional: one-way extinction in 1/m (kidmp_mie_out.ext); NULL = no attenuation
 *   vd     [ncol][nz]  optional: mean Doppler velocity of a vertical beam, positive downward, w already applied
 *                      (kidmp_doppler_out.vd, kidmp_mie_out.vd); NULL = 0
 *   u      [ncol][nz], or [nx][nz] with shared_flow != 0: the x velocity at the LEFT face of each cell, exactly the u of
 *                      kidmp_kid_advect_slab_device; NULL = 0
 *   zf     [nz+1] binary64: the level faces in m, ascending (stated, not checked)
 *   rays   [nray*nsub][6] binary64, one row per sub-ray: {slab, x0, z0, ce, se, wgt} -- the slab index as a whole number,
 *          the radar's position in m, cosine and sine of the elevation as the caller formed them (the kernel evaluates no
 *          trigonometric function) and the beam weight.  Output ray r is the weighted mean over its nsub consecutive rows.
 *   dx is a scalar.  zf and rays are binary64 in both entries.
 *
 * In binary64, every operation rounded once, no contraction, IEEE division:
 *
 *   geometry  per sub-ray and gate g = 0 .. ngate-1 (kid_amd/csrc/kidmp_scan_geom.h):
 *               r = r0 + (double(g) + 0.5)*dr;   s = r*ce;   x = x0 + s;   h = (z0 + r*se) + (s*s)*half_inv_ae
 *               xi = floor(x/dx);  periodic != 0: i = xi mod nx as whole numbers, in [0, nx); otherwise the sample is
 *               outside unless 0 <= xi < nx
 *               k = (the number of faces zf[0 .. nz] that are <= h) - 1; outside unless zf[0] <= h < zf[nz]
 *             Outside as well: a non-finite x or h; |xi| >= 2**52; a slab that is no whole number in [0, nslab); a wgt
 *             that is not finite or not above 0.  A gate centre exactly on a face belongs to the level above it, one
 *             exactly on x = i*dx to cell i.  half_inv_ae = 1/(2 a_e), a_e the effective earth radius; 0 = a flat earth.
 *   values    per inside sample at cell (i, k) of its slab:
 *               d = dbz;   a = ext*dr (+0.0 at an outside sample or with ext NULL)
 *               uc = 0.5*(u[i,k] + u[(i+1) mod nx, k]);   v = uc*ce - vd*se   (positive away from the radar)
 *             The elevation of the projection is the launch elevation: curvature raises the beam but does not tilt it.
 *   path      tau[g] = (sum over g' < g of a[g']) + 0.5*a[g];   p = (20/ln 10)*tau  (two-way, dB);   e = d - p
 *             The exclusive sum is the scan of kidmp_mie.h's tau_up with gates in place of levels: a Kogge-Stone scan
 *             over each group of 64 gates, the groups chained through a carry, the order fixed by g alone.
 *   beam      nsub == 1, a pass-through without a transcendental: dbz = d, pia = p, dbz_att = e, vr = v.
 *             nsub > 1, over the inside samples j of the gate, ascending, sums starting at +0.0:
 *               z_j = wgt_j*E((ln 10/10)*d_j);   z'_j = wgt_j*E((ln 10/10)*e_j);   W = sum wgt_j
 *               dbz = (10/ln 10)*L((sum z_j)/W);   dbz_att = (10/ln 10)*L((sum z'_j)/W);   pia = dbz - dbz_att
 *               vr = (sum z'_j*v_j)/(sum z'_j), +0.0 where sum z'_j is not above 0
 *             E(t) is fastmath.h's exp of min(t, 700) for t above -700 and +0.0 otherwise; L(q) is fastmath.h's ln for q
 *             not below the smallest normal number and -inf otherwise.
 *             A gate with no inside sample stores `missing` in dbz, dbz_att, pia and vr.
 *   outputs   dbz, dbz_att, pia, vr, height [nray][ngate] and cell [nray][ngate] (int32).  height is h of the centre
 *             sub-ray (row nsub/2) at every gate, always written, NaN where that row's slab or wgt is refused; cell is
 *             col*nz + k of the centre sub-ray's sample, -1 where it is outside.  The kidmp32_ entry takes binary32 fields,
 *             widens on load, computes as above and rounds once on store (`missing` too).
 *
 * The bits of a ray do not depend on the batch, on its position in the table, on a repeated call or on which outputs were
 * requested.  Any content of rays and zf is memory-safe: every gather index is formed from a sample already judged
 * inside.  A NaN field value is memory-safe and gives unspecified values in that gate and, through ext, in those behind it.
 *
 * Not modelled: beam broadening in azimuth (a slab has no y), refraction other than the effective earth radius, range
 * weighting inside a gate, ground clutter and beam blockage, multiple scattering.
 *
 * There are no host-array entries and no Fortran binding, for the reasons of kidmp_slab.h: the fields of a slab run live
 * on the card, and the diagnostics' column-chunked stager cannot split columns that one beam crosses.
 */
#ifndef KIDMP_SCAN_H
#define KIDMP_SCAN_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_SCAN_MAX_GATES 1024
#define KIDMP_SCAN_MAX_SUB 9

/* r0 >= 0 and dr > 0 in m: gate g is centred at r0 + (g + 0.5)*dr.  1 <= ngate <= KIDMP_SCAN_MAX_GATES,
 * 1 <= nsub <= KIDMP_SCAN_MAX_SUB.  half_inv_ae finite.  periodic != 0 wraps x into the slab.  missing may be any bit
 * pattern, a NaN included. */
typedef struct kidmp_scan_cfg {
    double r0, dr;
    int32_t ngate, nsub;
    double half_inv_ae;
    int32_t periodic;
    double missing;
} kidmp_scan_cfg;

/* Each member is [nray][ngate] or NULL (not wanted: no store).  At least one must be asked for. */
typedef struct kidmp_scan_out { double *dbz, *dbz_att, *pia, *vr, *height; int32_t *cell; } kidmp_scan_out;
typedef struct kidmp32_scan_out { float *dbz, *dbz_att, *pia, *vr, *height; int32_t *cell; } kidmp32_scan_out;

/* The entries never allocate, never synchronise and enqueue exactly one launch on `stream`: they can be captured into a
 * hipGraph and called between the steps of a device-resident run.  Outputs must not overlap inputs or one another (stated,
 * not checked).
 * KIDMP_EINVAL, nothing written: nx < 1; nz outside [2, KIDMP_MAX_NZ]; nslab < 0 or nslab*nx > 0x7fffffff; cell wanted
 * with nslab*nx*nz > 0x7fffffff; nray outside [0, 0x7fffffff]; ngate or nsub out of range; dx or dr not above 0 or
 * not finite; r0 below 0 or not finite; a non-finite half_inv_ae; a NULL among dbz, zf, rays, cfg, out; every member of
 * out NULL; vr wanted with both vd and u NULL; a pointer that is not memory of the context's device.  A NULL context
 * returns KIDMP_ESTATE; nray == 0 or nslab == 0 returns KIDMP_OK. */
int kidmp_scan_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dx,
        const double *dbz, const double *ext, const double *vd, const double *u, int32_t shared_flow,
        const double *zf, const double *rays, int64_t nray, const kidmp_scan_cfg *cfg, const kidmp_scan_out *out, void *stream);
int kidmp32_scan_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dx,
        const float *dbz, const float *ext, const float *vd, const float *u, int32_t shared_flow,
        const double *zf, const double *rays, int64_t nray, const kidmp_scan_cfg *cfg, const kidmp32_scan_out *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_SCAN_H */
