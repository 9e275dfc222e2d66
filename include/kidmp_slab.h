/*
 * kidmp_slab.h -- the kinematic half of a 2-D (x-z) KiD case on the device: prescribed-(u, w) advection of KiD's nine
 * fields on a batch of independent slabs that are periodic in x, in the adv / div form the adapter consumes.
 *
 * With kidmp_kid_advect_slab_device, kidmp_kid_interface_device and kidmp_kid_update_device (kidmp_kinematic.h) a whole
 * x-z case runs without a host round trip and can be captured in a graph.  Conventions as in kidmp.h and
 * kidmp_kinematic.h (return codes, device binding, k fastest, k = 0 the lowest level, the nine members of
 * kidmp_kid_fields / kidmp32_kid_fields).
 *
 * LAYOUT.  ncol = nslab*nx columns, every field [ncol][nz]; column s*nx + i is cell i of slab s.  u holds the x-face
 * velocities, nz per column: u[col][k] is at the LEFT face of cell i, between cells (i-1) mod nx and i.  w holds nz+1
 * face values per column as in kidmp_kid_advect_device.  With shared_flow != 0, u is [nx][nz] and w is [nx][nz+1] and
 * every slab uses them; with shared_flow == 0 they are [ncol][nz] and [ncol][nz+1].  rho and dz are one profile of nz
 * values each, dx is a scalar.
 *
 * THE SCHEME IS THE PROJECT'S OWN, as in kidmp_kinematic.h (KiD's ULTIMATE is not part of the reference this library was
 * written against): the 1-D entry's flux-form upwind scheme with a van Leer limiter, applied unsplit in both directions.
 * It is the scheme of a new context; kidmp_advection.h offers ULTIMATE QUICKEST as a second one, which changes qf in z and x.
 * Binary64, every operation rounded once (no contraction, IEEE division), in this order:
 *
 *   z part:  advz[i,k], divz[i,k] and the face Courant numbers cz[i,f] (f = 0 .. nz) are EXACTLY adv[k], div[k] and c of
 *            kidmp_kid_advect_device for column i with w[i,:] -- the same operations in the same order.
 *   x part, all x indices mod nx:
 *     Mx[i,k] = rho[k]*u[i,k]
 *     face i:  u[i,k] >= 0 ? (U,D,UU) = (i-1, i, i-2) : (U,D,UU) = (i, i-1, i+1)
 *         cx[i,k] = (|u[i,k]|*dt)/dx
 *         dq = q[D,k] - q[U,k];   b = q[U,k] - q[UU,k];   bd = b*dq
 *         s  = bd > 0 ? (2.0*bd)/(b + dq) : 0.0
 *         qf = q[U,k] + (0.5*(1.0 - cx[i,k]))*s
 *     Fx[i,k]   = Mx[i,k]*qf;   denx[k] = rho[k]*dx
 *     advx[i,k] = -((Fx[i+1,k] - Fx[i,k])/denx[k])
 *     divx[i,k] = q[i,k]*((Mx[i+1,k] - Mx[i,k])/denx[k])
 *   adv = advz + advx;   div = divz + divx;   sum = adv + div
 *   courant[col] = MAX_k ( max(cz[i,k], cz[i,k+1]) + max(cx[i,k], cx[i+1,k]) )
 *
 * adv is the flux-form tendency: over a slab, SUM_{i,k} rho[k]*dz[k]*adv telescopes in x and leaves the z boundary
 * fluxes.  adv + div is the advective form and leaves a constant field constant.  courant is the unsplit stability
 * number of the column's cells (one rounding in the add); for uniform one-signed flow q + dt*adv stays non-negative
 * while cx(2 - cx) + cz(2 - cz) <= 1.  The entry does not enforce this, it reports courant.
 * With u == +0.0 everywhere and non-negative fields every output equals, as a number, that of kidmp_kid_advect_device on
 * the same state; a zero may differ in sign (divz + 0.0 turns -0.0 into +0.0).
 *
 * The kidmp32_* entry takes binary32 arrays (u, w, rho, dz and courant too), widens on load, computes as above and rounds
 * once on store.  A slab gives the same bits alone, at any position of a batch and on a repeated call; rolling a slab's
 * cells in x rolls its outputs.  Inputs are assumed finite and rho, dz positive; a NaN input is memory-safe and gives
 * unspecified values.
 *
 * There are no host-array entries and no Fortran binding, for the reasons of kidmp_kinematic.h: a Fortran KiD build owns
 * its advection, and a host caller that ships fields across PCIe gains nothing from advecting them on the card.
 */
#ifndef KIDMP_SLAB_H
#define KIDMP_SLAB_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*   state                   IN, never written.  A NULL member is not advected and its outputs are not written; theta, qv,
 *                           qc, qr and nr are required.  In an iiwarm context qi, ni, qs and qg of every struct are
 *                           ignored throughout, as in the adapter.
 *   u, w, shared_flow       see LAYOUT
 *   adv, div, sum           optional outputs: a whole struct or any member may be NULL and then costs no store
 *   courant                 optional [ncol]
 * The entry never allocates, never synchronises and enqueues exactly one launch on `stream`: it can be captured into a
 * hipGraph.  Outputs must not overlap inputs or one another (stated, not checked).
 * KIDMP_EINVAL, nothing written: nx < 3 (the five-point stencil must name distinct cells); nz outside [2, KIDMP_MAX_NZ];
 * nslab < 0; nslab*nx > 0x7fffffff; dt <= 0 or dx <= 0; state, u, w, rho, dz or a required member NULL; nothing requested
 * (no output member of a present field and no courant); a pointer that is not memory of the context's device.  A NULL
 * context returns KIDMP_ESTATE; nslab == 0 returns KIDMP_OK. */
int kidmp_kid_advect_slab_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
        const kidmp_kid_fields *state, const double *u, const double *w, int32_t shared_flow, const double *rho, const double *dz,
        const kidmp_kid_fields *adv, const kidmp_kid_fields *div, const kidmp_kid_fields *sum, double *courant, void *stream);
int kidmp32_kid_advect_slab_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
        const kidmp32_kid_fields *state, const float *u, const float *w, int32_t shared_flow, const float *rho, const float *dz,
        const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div, const kidmp32_kid_fields *sum, float *courant, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_SLAB_H */
