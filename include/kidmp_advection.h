/*
 * kidmp_advection.h -- the advection scheme of the KiD path, a setting of the context.
 *
 * The eight advection entries -- kidmp[32]_kid_advect_device (kidmp_kinematic.h), kidmp[32]_kid_advect_slab_device
 * (kidmp_slab.h), kidmp[32]_kid_advect_aero_device and kidmp[32]_kid_advect_slab_aero_device (kidmp_aerosol.h) -- read
 * the setting when they are called; nothing else does.  A new context is KIDMP_ADVECT_VANLEER, the scheme those headers
 * write out, and its results are bit for bit what they were before this header existed.  Conventions as in kidmp.h.
 *
 * KIDMP_ADVECT_ULTIMATE is Leonard's ULTIMATE QUICKEST (B. P. Leonard, "The ULTIMATE conservative difference scheme
 * applied to unsteady one-dimensional advection", Comput. Methods Appl. Mech. Engrg. 88 (1991) 17-74): the universal
 * limiter applied to the QUICKEST face value, one-dimensional, applied unsplit in x and z on a slab like the van Leer
 * scheme.  KiD documents its advection as ULTIMATE, but KiD's routine is not part of the reference this library was
 * written against: THIS IS THE PUBLISHED ALGORITHM, NOT A PORT OF KiD'S CODE, and parity with a KiD build is not pinned.
 *
 * It is fixed to the operation like the van Leer scheme: binary64, every operation rounded once (no contraction, IEEE
 * division).  M, c, den, the upwind side, (u, d, uu), the boundary faces, F, adv, div, sum and courant are EXACTLY those of
 * kidmp_kinematic.h; only qf of an interior face changes.  Per face and column, shared by all members:
 *
 *   hc = 0.5*(1.0 - c);   g = (1.0 - c*c)/6.0;   rc = 1.0/c                   (c == +0.0 gives +inf)
 *
 * and per member:
 *
 *   dq = q[d] - q[u];   b = q[u] - q[uu];   bd = b*dq
 *   if not (uu inside [0,nz) and bd > 0):
 *       qf = q[u]                                                             (first-order upwind)
 *   else:
 *       curv = dq - b
 *       qq   = (q[u] + hc*dq) - g*curv                                        (QUICKEST, uniform-grid weights)
 *       ref  = q[uu] + b*rc                                                   (b != 0 here: +-inf at c == 0, never NaN)
 *       dq > 0:  t = qq > q[u] ? qq : q[u];   h = ref < q[d] ? ref : q[d];   qf = t < h ? t : h
 *       else:    t = qq < q[u] ? qq : q[u];   h = ref > q[d] ? ref : q[d];   qf = t > h ? t : h
 *
 * The selects are comparisons, not fmin / fmax, so signed zeros are fixed.  In the x part of a slab the same holds with
 * cx, 1.0/cx and indices mod nx; every cell has a second upwind neighbour there, so there is no `inside` test.
 *
 * The face value uses the uniform-grid weights on any dz, as the van Leer form does: THIRD ORDER IS CLAIMED ON UNIFORM
 * GRIDS ONLY.  Under one-signed uniform flow at a Courant number <= 1 a face value lies between its upwind and downwind
 * cells and the updated cell stays within the range of its three-cell upwind neighbourhood (a few ulp of the field's
 * maximum aside); faces with w == 0 or c > 1 give finite values.  There is no multidimensional (transverse) term.
 */
#ifndef KIDMP_ADVECTION_H
#define KIDMP_ADVECTION_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_ADVECT_VANLEER  0     /* flux-form upwind with a van Leer limiter (kidmp_kinematic.h, kidmp_slab.h) */
#define KIDMP_ADVECT_ULTIMATE 1     /* ULTIMATE QUICKEST, above */

/* Selects the scheme of every later advection call on `ctx`; calls already enqueued keep the scheme they were enqueued
 * with.  KIDMP_EINVAL for any other value, with nothing changed; KIDMP_ESTATE for a NULL context. */
int kidmp_set_advection(kidmp_ctx *ctx, int32_t scheme);
/* The current scheme, or KIDMP_ESTATE for a NULL context. */
int kidmp_advection(const kidmp_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_ADVECTION_H */
