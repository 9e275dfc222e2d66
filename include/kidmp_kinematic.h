/*
 * kidmp_kinematic.h -- the kinematic half of a 1-D KiD case on the device: prescribed-w vertical advection of KiD's nine
 * fields in the adv / div form the adapter consumes, and the state update that closes the time loop.
 *
 * With kidmp_kid_advect_device, kidmp_kid_interface_device and kidmp_kid_update_device a whole 1-D case (w(z,t) in, final
 * state, precipitation and any per-step diagnostic out) runs without a host round trip and can be captured in a graph.
 * Conventions as in kidmp.h (return codes, device binding, [ncol][nz] arrays with k fastest, k = 0 the lowest level);
 * the nine members are those of kidmp_kid_fields / kidmp32_kid_fields.
 *
 * THE SCHEME IS THE PROJECT'S OWN.  The KiD driver's advection code (ULTIMATE) is not part of the reference this library
 * was written against, so nothing here is a port and nothing is bit-compatible with a KiD build: it is a flux-form
 * upwind scheme with a van Leer limiter, fixed to the operation so that a restatement in any IEEE binary64 arithmetic
 * gives the same bits.  It is the scheme of a new context; kidmp_advection.h offers ULTIMATE QUICKEST as a second one, which
 * changes qf of an interior face and nothing else.  Binary64, every operation rounded once (no contraction, IEEE division),
 * in this order:
 *
 *   rf[0] = rho[0];  rf[nz] = rho[nz-1];  rf[f] = 0.5*(rho[f-1] + rho[f])      (0 < f < nz)
 *   M[f]  = rf[f]*w[f]
 *   interior face f:  w[f] >= 0 ? (u,d,uu) = (f-1, f, f-2) : (u,d,uu) = (f, f-1, f+1)
 *       c  = (|w[f]|*dt)/dz[u]
 *       dq = q[d] - q[u];   b = q[u] - q[uu];   bd = b*dq
 *       s  = (uu inside [0,nz) and bd > 0) ? (2.0*bd)/(b + dq) : 0.0          (van Leer, harmonic form: no ratio, no NaN)
 *       qf[f] = q[u] + (0.5*(1.0 - c))*s
 *   boundary faces:  qf[0] = q[0];  qf[nz] = q[nz-1]                          (zero gradient; w[0] = 0 closes the bottom)
 *   F[f]   = M[f]*qf[f];   den[k] = rho[k]*dz[k]
 *   adv[k] = -((F[k+1] - F[k])/den[k])
 *   div[k] = q[k]*((M[k+1] - M[k])/den[k])
 *   sum[k] = adv[k] + div[k]
 *   courant[col] = MAX over all nz+1 faces of c     (the boundary faces use dz[0] and dz[nz-1])
 *
 * adv is the flux-form tendency: SUM_k den[k]*adv[k] telescopes to F[0] - F[nz].  adv + div is the advective-form
 * tendency and leaves a constant field constant.  The adapter's gather forms (adv + div) first, so passing `sum` as the
 * adapter's adv with div = NULL gives the gather the same bits as passing adv and div -- with one exception: where the
 * sum is -0.0 the gather's (sum + 0) is +0.0.  Monotonicity and positivity hold for courant <= 1 with one-signed flow;
 * the entry does not enforce this, it reports courant.
 *
 * The kidmp32_* entries take binary32 arrays (w, rho and dz too), widen on load, compute as above and round once on
 * store, like the other diagnostics.  A column gives the same bits alone, at any position in any batch and on a
 * repeated call.  Inputs are assumed finite and rho, dz positive; a NaN input is memory-safe and gives unspecified values.
 *
 * There are no host-array entries and no Fortran binding: a Fortran KiD build owns its advection, and a host caller that
 * ships fields across PCIe gains nothing from advecting them on the card.
 */
#ifndef KIDMP_KINEMATIC_H
#define KIDMP_KINEMATIC_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*   state                   IN, never written.  A NULL member is not advected and its outputs are not written; theta, qv,
 *                           qc, qr and nr are required.  In an iiwarm context qi, ni, qs and qg of every struct are
 *                           ignored throughout, as in the adapter.
 *   w, w_col_stride         face velocities in m/s, nz+1 per column: face f is the lower face of cell f, face nz the model
 *                           top.  Element (col, f) = w[col*w_col_stride + f]; 0 = one profile shared by all columns,
 *                           otherwise >= nz+1
 *   rho, dz                 one profile of nz values each (in KiD both depend on z only)
 *   adv, div, sum           optional outputs: a whole struct or any member may be NULL and then costs no store
 *   courant                 optional [ncol]
 * The entry never allocates, never synchronises and enqueues exactly one launch on `stream`: it can be captured into a
 * hipGraph.  Outputs must not overlap inputs or one another (stated, not checked).
 * KIDMP_EINVAL, nothing written: state, w, rho, dz or a required member NULL; nz outside [2, KIDMP_MAX_NZ]; ncol < 0;
 * dt <= 0; a w_col_stride that is neither 0 nor >= nz+1; nothing requested (no output member of a present field and no
 * courant); a pointer that is not memory of the context's device.  A NULL context returns KIDMP_ESTATE; ncol == 0
 * returns KIDMP_OK. */
int kidmp_kid_advect_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_fields *state,
        const double *w, int64_t w_col_stride, const double *rho, const double *dz,
        const kidmp_kid_fields *adv, const kidmp_kid_fields *div, const kidmp_kid_fields *sum, double *courant, void *stream);
int kidmp32_kid_advect_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp32_kid_fields *state,
        const float *w, int64_t w_col_stride, const float *rho, const float *dz,
        const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div, const kidmp32_kid_fields *sum, float *courant, void *stream);

/* state is INOUT: X = X + ((t1 + t2) + t3)*dt, every operation rounded in the arrays' own format (the entry pairs with
 * the adapter, whose arithmetic is in that format).  A NULL struct or member of t1, t2, t3 is a literal +0.0 operand that
 * is never read, as in the adapter's gather.  With clip != 0 every member except theta then becomes X < 0 ? +0.0 : X.  A
 * NULL member of state is skipped; in an iiwarm context qi, ni, qs and qg are ignored.
 * One launch on `stream`, no allocation, no synchronisation.  The tendencies must not overlap state.
 * KIDMP_EINVAL, nothing written: state NULL or without any member; nz outside [2, KIDMP_MAX_NZ]; ncol < 0; dt <= 0; a
 * pointer that is not memory of the context's device.  A NULL context returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_kid_update_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_fields *state,
        const kidmp_kid_fields *t1, const kidmp_kid_fields *t2, const kidmp_kid_fields *t3, int32_t clip, void *stream);
int kidmp32_kid_update_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, const kidmp32_kid_fields *state,
        const kidmp32_kid_fields *t1, const kidmp32_kid_fields *t2, const kidmp32_kid_fields *t3, int32_t clip, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_KINEMATIC_H */
