/*
 * kidmp_aerosol.h -- prognostic aerosols in the KiD path: the droplet number nc and the two aerosol numbers nwfa (water
 * friendly, CCN) and nifa (ice friendly, IN) carried through the adapter, both advection entries and the update, on the
 * device, for a context made with kidmp_cfg.is_aerosol_aware.
 *
 * kidmp_kid_interface_device (kidmp.h) fills nc, nwfa and nifa with the non-aerosol defaults of M:958-964 on every call
 * and hands the step w = 0; in an aerosol-aware context it still does, so activation cannot deplete CCN from one step to
 * the next.  The entries below take the three fields as state, as the reference's 3-D driver documents it (copy in and
 * out, M:950-956 and M:1003-1007; a surface source into the lowest level, M:1001).  Conventions as in kidmp.h,
 * kidmp_kinematic.h and kidmp_slab.h: return codes, device binding, arrays [ncol][nz] with k fastest and k = 0 the lowest
 * level, a NULL context returns KIDMP_ESTATE, ncol == 0 returns KIDMP_OK, KIDMP_EINVAL leaves everything unwritten.  No
 * entry allocates or synchronises; each enqueues its launches on `stream` alone, as one linear chain, and can be captured
 * into a hipGraph.  Every pointer must be memory of the context's device.
 *
 * The kidmp32_* twins take binary32 arrays; the interface twin also takes `arith` like kidmp32_kid_interface_device.
 *
 * TWO FACTS ABOUT THIS BRANCH.  tnccn_act is 1.0 everywhere in the reference this library follows (M:752-762), so the
 * activated fraction is 1 and the updraft changes activ_ncloud's result by rounding only.  And the reference has no
 * recorded output with is_aerosol_aware set (KiD never sets it): parity of this branch is unpinned, as for the
 * aerosol-aware column step itself.
 *
 * There are no host-array entries and no Fortran binding.  The reference adapter never carries aerosols: W:36 declares
 * nc1d, nwfa1d, nifa1d and w1d and leaves them unset, so a Fortran KiD build has nothing to pass; and the reasons of
 * kidmp_kinematic.h hold as well (a Fortran KiD build owns its advection, and a host caller that ships fields across
 * PCIe gains nothing from moving them on the card).
 */
#ifndef KIDMP_AEROSOL_H
#define KIDMP_AEROSOL_H

#include "kidmp.h"
#include "kidmp_kinematic.h"
#include "kidmp_slab.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kidmp_kid_aerosols   { double *nc, *nwfa, *nifa; } kidmp_kid_aerosols;   /* each [ncol][nz], per kg */
typedef struct kidmp32_kid_aerosols { float  *nc, *nwfa, *nifa; } kidmp32_kid_aerosols;

/* The adapter with prognostic aerosols: the arguments of kidmp_kid_interface_device, then
 *   aer          IN: nc, nwfa, nifa, all three required
 *   aer_adv, aer_div   IN, optional: a NULL struct or member is a zero operand, as for adv and div
 *   aer_mphys    OUT: the three microphysics tendencies, all three required
 *   w, w_col_stride    the cell-centre updraft in m/s: w[col*w_col_stride + k].  w_col_stride == 0: one profile of nz values
 *                shared by all columns; otherwise >= nz.  NULL: zeros.  It becomes workspace profile 13, where mp_thompson
 *                reads w1d (M:2797)
 *   nwfa_src     optional [ncol], per kg per second: the surface source of M:1001
 * Gather: A1 = A + (dA_adv + dA_div)*dt for A = nc, nwfa, nifa, every operation rounded once in the arrays' format, the
 * expression of the other moments (W:60-93), into workspace profiles 8, 9 and 10; the other twelve profiles and ppt are
 * bit for bit those of kidmp_kid_gather_device.  The workspace is that of kidmp_kid_workspace_bytes / _offset.  Then the
 * column step and the column outputs as in kidmp_kid_interface_device.  Then, with nwfa_src,
 * nwfa1[col][0] = nwfa1[col][0] + nwfa_src[col]*dt, stored back into profile 9.  Back-out:
 * dA_mphys = (A1 - A)/dt - (dA_adv + dA_div) for the three members, with the nine tendencies of the other entry.  In a
 * context that is iiwarm as well the frozen members of state, adv, div and mphys are ignored, as in the adapter.
 * KIDMP_EINVAL, nothing written: everything kidmp_kid_interface_device refuses; a context that is not aerosol-aware;
 * aer, aer_mphys or one of their members NULL; w_col_stride in [1, nz-1] or negative; in the kidmp32_ twin, an arith other
 * than KIDMP_ARITH_P32N (the all-binary32 column step is not offered with prognostic aerosols: DESIGN.md section 4.6e). */
int kidmp_kid_interface_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
        const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
        const double *exner, const double *dz, const kidmp_kid_fields *mphys, double *ppt,
        double *rates, int32_t *nstep, const kidmp_outputs *out,
        const kidmp_kid_aerosols *aer, const kidmp_kid_aerosols *aer_adv, const kidmp_kid_aerosols *aer_div,
        const kidmp_kid_aerosols *aer_mphys, const double *w, int64_t w_col_stride, const double *nwfa_src,
        void *work, size_t work_bytes, void *stream);
int kidmp32_kid_interface_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
        const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
        const float *exner, const float *dz, const kidmp32_kid_fields *mphys, float *ppt,
        double *rates, int32_t *nstep, const kidmp32_outputs *out, int32_t arith,
        const kidmp32_kid_aerosols *aer, const kidmp32_kid_aerosols *aer_adv, const kidmp32_kid_aerosols *aer_div,
        const kidmp32_kid_aerosols *aer_mphys, const float *w, int64_t w_col_stride, const float *nwfa_src,
        void *work, size_t work_bytes, void *stream);

/* The gather alone, the counterpart of kidmp_kid_gather_device: the workspace holds the step's inputs, ppt is zeroed. */
int kidmp_kid_gather_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
        const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
        const double *exner, const double *dz, double *ppt,
        const kidmp_kid_aerosols *aer, const kidmp_kid_aerosols *aer_adv, const kidmp_kid_aerosols *aer_div,
        const double *w, int64_t w_col_stride, void *work, size_t work_bytes, void *stream);
int kidmp32_kid_gather_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
        const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
        const float *exner, const float *dz, float *ppt,
        const kidmp32_kid_aerosols *aer, const kidmp32_kid_aerosols *aer_adv, const kidmp32_kid_aerosols *aer_div,
        const float *w, int64_t w_col_stride, void *work, size_t work_bytes, void *stream);

/* Vertical advection of the aerosols: for each present member of `aer` exactly the operations of kidmp_kid_advect_device in
 * the same order, so a field gives the same bits here and in a slot of the nine-field entry.  w holds the nz+1 FACE
 * velocities of that entry (w_col_stride 0 or >= nz+1).  A NULL member of aer is not advected and its outputs are not
 * written; a NULL struct or member of adv, div, sum costs no store.  There is no courant output: the nine-field call
 * reports it.  One launch.  KIDMP_EINVAL: what kidmp_kid_advect_device refuses; aer NULL; nothing requested. */
int kidmp_kid_advect_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_aerosols *aer,
        const double *w, int64_t w_col_stride, const double *rho, const double *dz,
        const kidmp_kid_aerosols *adv, const kidmp_kid_aerosols *div, const kidmp_kid_aerosols *sum, void *stream);
int kidmp32_kid_advect_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp32_kid_aerosols *aer,
        const float *w, int64_t w_col_stride, const float *rho, const float *dz,
        const kidmp32_kid_aerosols *adv, const kidmp32_kid_aerosols *div, const kidmp32_kid_aerosols *sum, void *stream);

/* The same for kidmp_kid_advect_slab_device: periodic in x, nx >= 3, layout and shared_flow as in kidmp_slab.h. */
int kidmp_kid_advect_slab_aero_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
        const kidmp_kid_aerosols *aer, const double *u, const double *w, int32_t shared_flow, const double *rho, const double *dz,
        const kidmp_kid_aerosols *adv, const kidmp_kid_aerosols *div, const kidmp_kid_aerosols *sum, void *stream);
int kidmp32_kid_advect_slab_aero_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dt, double dx,
        const kidmp32_kid_aerosols *aer, const float *u, const float *w, int32_t shared_flow, const float *rho, const float *dz,
        const kidmp32_kid_aerosols *adv, const kidmp32_kid_aerosols *div, const kidmp32_kid_aerosols *sum, void *stream);

/* A = A + ((t1 + t2) + t3)*dt in the arrays' format for the present members of aer; a NULL tendency struct or member is
 * a zero operand.  With clip != 0 the result is A < 0 ? +0.0 : A for all three members.  One launch. */
int kidmp_kid_update_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, const kidmp_kid_aerosols *aer,
        const kidmp_kid_aerosols *t1, const kidmp_kid_aerosols *t2, const kidmp_kid_aerosols *t3, int32_t clip, void *stream);
int kidmp32_kid_update_aero_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, const kidmp32_kid_aerosols *aer,
        const kidmp32_kid_aerosols *t1, const kidmp32_kid_aerosols *t2, const kidmp32_kid_aerosols *t3, int32_t clip, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_AEROSOL_H */
