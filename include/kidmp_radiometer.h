/*
 * kidmp_radiometer.h -- a passive microwave radiometer: two-stream brightness temperatures at a chosen wavelength, looking
 * up from the ground or down from orbit.
 *
 * The third instrument beside the radar (kidmp_mie.h) and the lidar (kidmp_lidar.h).  Each species' particles are the
 * Lorenz-Mie spheres of kidmp_mie.h; a table of three numbers per diameter bin is built once on the host
 * (kidmp_radiometer_table_create) and one launch of kidmp::k_radiometer folds it into the scheme's size distributions,
 * forms a two-stream layer per level and adds the layers with two wave scans.  The particle models and every definition
 * below are the project's own convention: the reference has no such diagnostic, and parity with an instrument simulator
 * is unpinned.  Conventions as in kidmp.h and kidmp_mie.h (return codes, device binding, [ncol][nz] arrays with k fastest,
 * k = 0 the lowest level).  In binary64, every operation rounded once, no contraction:
 *
 *   sphere    the series of kidmp_mie.h (kid_amd/csrc/kidmp_mie_sphere.h; Q_ext and Q_back are kidmp_mie_sphere's bit for
 *             bit), which also yields
 *               Q_sca   = (2/x**2) sum_{n=1..nstop} (2n+1) (|a_n|**2 + |b_n|**2)
 *               g Q_sca = (4/x**2) [ sum_{n=1..nstop-1} (n(n+2)/(n+1)) Re(a_n conj(a_{n+1}) + b_n conj(b_{n+1}))
 *                                    + sum_{n=1..nstop} ((2n+1)/(n(n+1))) Re(a_n conj(b_n)) ]
 *             and g = (g Q_sca)/Q_sca, +0.0 where Q_sca is not above 0.
 *   rows      per species and bin (D, dD), with the particle models of kidmp_mie.h, in this order:
 *               0 s_abs   max(Q_ext - Q_sca, 0) * (pi D**2/4), m**2; +0.0 where the particle's index is real (Q_ext - Q_sca is
 *                         then rounding residue of either sign)
 *               1 s_bsc   max(0.5*(Q_sca - g Q_sca), 0) * (pi D**2/4), m**2: the cross-section scattered into the backward
 *                         hemisphere (g Q_sca as the series gives it, not g times Q_sca)
 *               2 mass    kg
 *   load      that of kidmp_mie_radar_device through the same functions; densities n = N_x(D_b)*dD_b as there.
 *   sums      per level and present species, over the bins ascending into accumulators that start at +0.0:
 *             A = sum n*s_abs, S = sum n*s_bsc, M = sum n*mass.
 *   carriers  abs_x = (rho*q_x)*A/M and bsc_x = (rho*q_x)*S/M in 1/m, +0.0 where the species is absent or M is not above
 *             0; abs_c is kidmp_mie.h's ext_c (Rayleigh absorption of cloud water where qc > R1); k_gas is the caller's
 *             absorption profile in 1/m.
 *               k_abs = (((abs_r + abs_s) + abs_g) + abs_c) + k_gas
 *               k_bsc = (bsc_r + bsc_s) + bsc_g
 *   layer     the hemispheric-constant two-stream of Meador & Weaver (1980) with the stream cosine mu as a parameter, the
 *             layer isothermal at t[k], in Rayleigh-Jeans brightness temperatures (linear in T).  With ta = k_abs*dz,
 *             b = k_bsc*dz, x = sqrt(ta*(ta + 2*b)), y = x/mu:
 *               ta <= 0 and b <= 0:  R = 0, T = 1, a = 0
 *               ta <= 0 <  b:        c = b/mu, R = c/(1 + c), T = 1/(1 + c), a = 0       (conservative scattering)
 *               otherwise:           S = (ta + b) + x, G = b/S, H = (ta + x)/S, e = exp(-y), f = y*g(y) with the g of
 *                                    kidmp_lidar.h (1 - e without cancellation), p = H + G*f, q = 1 + G*e,
 *                                    R = (G*f*(1 + e))/(p*q), T = (H*(1 + G)*e)/(p*q), a = (H*f)/q
 *             The layer's state is (Rt, Rb, T, Eu, Ed) = (R, R, T, a*t[k], a*t[k]).  With b = 0 this is Schwarzschild's
 *             layer, T = exp(-ta/mu), a = 1 - T.  (kid_amd/csrc/kidmp_radiometer_layer.h)
 *   adding    combine(lower A, upper B):  d = 1 - Rt_A*Rb_B;  T = (T_A*T_B)/d;  Rb = Rb_A + ((T_A*T_A)*Rb_B)/d;
 *             Rt = Rt_B + ((T_B*T_B)*Rt_A)/d;  Eu = Eu_B + (T_B*(Eu_A + Rt_A*Ed_B))/d;  Ed = Ed_A + (T_A*(Ed_B + Rb_B*Eu_A))/d.
 *             (0, 0, 1, 0, 0) is the identity, the state of a level past nz.  The stack below a level is a Kogge-Stone
 *             scan over the lanes of a wavefront with combine in place of a sum, the lower operand first, the groups of
 *             64 levels chained upwards through a carry state; the stack above it is the mirror image from the top.  The
 *             order of every operation is a pure function of the level and of ceil(nz/64).
 *   closure   with P the stack below a face, S the stack above it, rs = 1 - emissivity, ts the surface temperature and
 *             tc the cosmic background:
 *               Rt* = Rt_P + ((T_P*T_P)*rs)/(1 - rs*Rb_P);  Eu* = Eu_P + (T_P*(emissivity*ts + rs*Ed_P))/(1 - rs*Rb_P);
 *               Dn = Ed_S + T_S*tc
 *             tb_up[k], at the upper face of level k (P = levels 0..k, S = levels k+1..nz-1) = (Eu* + Rt**Dn)/(1 - Rt**Rb_S);
 *             tb_down[k], at the lower face of level k (P = levels 0..k-1, S = levels k..nz-1) = (Dn + Rb_S*Eu*)/(1 - Rt**Rb_S).
 *   outputs   k_abs, k_bsc, refl (R), trans (T), tb_up, tb_down [ncol][nz]; tb_toa [ncol], the bits of tb_up[nz-1]: what a
 *             satellite sees; tb_ground [ncol], the bits of tb_down[0]: what a ground radiometer sees; tau_abs [ncol] =
 *             sum_k k_abs*dz.  Binary64 inside, the kidmp32_ entries round once on store.  A NULL costs no store; a
 *             request for k_abs, k_bsc alone runs no layer and no scan, one without a brightness temperature no scan.
 *             The bits of a column do not depend on the batch, on its position, on a repeated call or on which outputs
 *             were requested.
 *
 * Not modelled: the Planck function, polarisation and view angles beyond mu, cloud ice, melting particles,
 * temperature-dependent permittivities and any gas absorption model (the caller passes k_gas).  Several channels in one
 * launch: kidmp_multichannel.h.
 */
#ifndef KIDMP_RADIOMETER_H
#define KIDMP_RADIOMETER_H

#include "kidmp_mie.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_RADIOMETER_NROWS 3

/* kidmp_radiometer_defaults writes mu = 1.0, emissivity = 1.0, t_cosmic = 2.725 K. */
typedef struct kidmp_radiometer_cfg {
    double mu;
    double emissivity;
    double t_cosmic;
} kidmp_radiometer_cfg;
void kidmp_radiometer_defaults(kidmp_radiometer_cfg *rcfg);

/* Each member is an array of the shape stated above or NULL (not wanted: no store).  At least one must be asked for. */
typedef struct kidmp_radiometer_out { double *k_abs, *k_bsc, *refl, *trans, *tb_up, *tb_down; double *tb_toa, *tb_ground, *tau_abs; } kidmp_radiometer_out;
typedef struct kidmp32_radiometer_out { float *k_abs, *k_bsc, *refl, *trans, *tb_up, *tb_down; float *tb_toa, *tb_ground, *tau_abs; } kidmp32_radiometer_out;

typedef struct kidmp_radiometer_table kidmp_radiometer_table;

/* Host entries that need no context and no device; refusals as kidmp_mie_sphere and kidmp_mie_bins (kw2 of cfg is not
 * read but must be valid).  rows is [KIDMP_RADIOMETER_NROWS][nb]. */
int kidmp_radiometer_sphere(double x, double m_re, double m_im, double *qext, double *qsca, double *qback, double *g);
int kidmp_radiometer_bins(const kidmp_mie_cfg *cfg, int32_t species, int32_t nb, const double *D, double *rows);

/* The table, as kidmp_mie_table_*: the three rows of the three species on the scheme's own 100 bins or the caller's (up to
 * KIDMP_MIE_MAX_BINS), built on the host and uploaded to the context's device; bound to its context; destroy it before
 * that context's kidmp_finalize. */
int kidmp_radiometer_table_create(kidmp_ctx *ctx, const kidmp_mie_cfg *cfg, const kidmp_mie_grids *grids, kidmp_radiometer_table **table);
void kidmp_radiometer_table_destroy(kidmp_radiometer_table *table);
int kidmp_radiometer_table_get(const kidmp_radiometer_table *table, int32_t species, int32_t *nb, double *D, double *dD, double *rows, kidmp_mie_cfg *cfg);

/* The step entries.  Device entries never allocate, never synchronise and enqueue exactly one launch on `stream`; host
 * entries run chunks of columns through the context's staging memory and equal the device entry bit for bit.  rcfg NULL =
 * the defaults.  t_sfc is [ncol], NULL = the column's t at level 0.  qc, qs, qg and k_gas may be NULL (zero); dz may be
 * NULL only when nothing but k_abs and k_bsc is wanted.  dz and k_gas take a column stride as in kidmp_mie_radar_device.
 * Refusals and return codes as kidmp_mie_radar_device, and KIDMP_EINVAL for mu outside (0, 1], emissivity outside [0, 1]
 * or t_cosmic not finite or below 0. */
int kidmp_radiometer_device(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride,
        const double *k_gas, int64_t k_gas_col_stride, const double *t_sfc, const kidmp_radiometer_out *out, void *stream);
int kidmp32_radiometer_device(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride,
        const float *k_gas, int64_t k_gas_col_stride, const float *t_sfc, const kidmp32_radiometer_out *out, void *stream);
int kidmp_radiometer_host(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride,
        const double *k_gas, int64_t k_gas_col_stride, const double *t_sfc, const kidmp_radiometer_out *out);
int kidmp32_radiometer_host(kidmp_ctx *ctx, const kidmp_radiometer_table *table, const kidmp_radiometer_cfg *rcfg, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride,
        const float *k_gas, int64_t k_gas_col_stride, const float *t_sfc, const kidmp32_radiometer_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_RADIOMETER_H */
