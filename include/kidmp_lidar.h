/*
 * kidmp_lidar.h -- a lidar / ceilometer forward operator on the device: extinction and attenuated backscatter.
 *
 * The radar diagnostics (kidmp_reflectivity_device, kidmp_doppler.h, kidmp_dspectrum.h) leave cloud droplets and cloud ice
 * out by definition.  The instrument beside every cloud radar, a ceilometer or lidar, sees exactly these: the liquid
 * cloud base, thin ice cloud, and the height at which the beam is spent.  kidmp_lidar_profiles_device forms, in one
 * launch of kidmp::k_lidar_profiles, the geometric-optics extinction of all five species from the scheme's own size
 * distributions in closed form, carries the optical depth along the column from the ground and from space, and gives the
 * layer-mean attenuated backscatter, the scattering ratio and eight numbers per column.  Conventions as in kidmp.h and
 * kidmp_summary.h (return codes, device binding, [ncol][nz] arrays with k fastest, k = 0 the lowest level; dz with
 * dz_col_stride; the bottom face of level k is zb(k) = sum_{k' < k} dz_k').
 *
 * The reference holds nothing like this.  The definitions below are this library's own; they are pinned by a numpy
 * restatement (tests/lidar_ref.py), and parity with any instrument simulator is NOT pinned.  In binary64:
 *
 *   load      exactly that of kidmp_size_spectra_device (kidmp_spectra.h): rho from qv' = max(1e-10, qv); the five species
 *             as that header states them, with the number limiting of ice and rain, block D's smob, block E's graupel
 *             intercept with its running minimum from the top down, and cloud water with Nt_c of the context, of
 *             kidmp_set_column_nc, or the aerosol-aware nc.  An absent species has exact +0.0 in everything of its own.
 *             An iiwarm context: qi, ni, qs and qg are not read and may be NULL; the frozen outputs are exact +0.0.
 *   ext_x     extinction per species in m-1, with Q_ext = 2 and the cross-section (pi/4) D**2 for all five (for snow a
 *             convention: calc_effectRad makes the same choice with its M3/M2 radius):
 *               ext_x = pi*n0_x/(lam_x*lam_x*lam_x)                      x in {i, r, g}: mu = 0, Gamma(3) = 2
 *               ext_c = (pi/2)*nc*((nu_c+1)(nu_c+2))/(lamc*lamc)         nc the loaded number
 *               ext_s = (pi/2)*smob                                      bm_s = 2: smob is the second moment
 *   totals    ext = (((ext_c + ext_i) + ext_r) + ext_s) + ext_g; bsc the same sum of ext_x / S_x (m-1 sr-1), S_x the
 *             lidar ratio of species x
 *   molecules bsc_mol = c_mol*(p/(k_B*T)), k_B = 1.380649e-23; ext_mol = (8 pi/3)*bsc_mol
 *   depth     dtau = (eta*ext + ext_mol)*dz and dtau_mol = ext_mol*dz; eta, the multiple-scattering factor, scales the
 *             particles only.  The instrument on the ground sits at the bottom face of level 0, the one in space above
 *             the top face of level nz-1:  tau_up(k) = sum_{k' < k} dtau(k'),  tau_dn(k) = sum_{k' > k} dtau(k'), and
 *             taum_up, taum_dn likewise of dtau_mol.
 *   att       layer-mean attenuated backscatter  att_up = (bsc + bsc_mol)*E(2*tau_up)*g(2*dtau), att_dn with tau_dn.
 *             E(x) = EXP(-x) with the 700 rule of kidmp_spectra.h: exact +0.0 past 700.  g(x) = (1 - EXP(-x))/x is the
 *             mean of EXP(-x') over the layer, formed without cancellation (within 3 ulp for every x >= 0, subnormal
 *             x included; g(0) = 1).  Molecules alone: attm_up = bsc_mol*E(2*taum_up)*g(2*dtau_mol), attm_dn likewise.
 *   sr        scattering ratio  sr_up = att_up/attm_up, sr_dn = att_dn/attm_dn.  Where attm is +0.0 (past the 700 rule)
 *             the ratio is what IEEE division gives.
 *   summary   summary[col][slot], binary64 in every entry; a quiet NaN where the level does not exist (kidmp_summary.h):
 *               0 TAU_PART    sum_k ext*dz
 *               1 TAU_MOL     sum_k ext_mol*dz
 *               2 Z_BASE_UP   bottom face of the lowest level with att_up >= beta_detect
 *               3 Z_LOST_UP   top face of the lowest level with E(2*(tau_up + dtau)) < trans_lost
 *               4 Z_TOP_DN    top face of the highest level with att_dn >= beta_detect
 *               5 Z_LOST_DN   bottom face of the highest level with E(2*(tau_dn + dtau)) < trans_lost
 *               6 N_UP        the number of levels with att_up >= beta_detect, as a double
 *               7 N_DN        the same for att_dn
 *
 * Order of the sums: the two prefix sums, the two suffix sums (reversed scans from the top, so that tau_dn is exact +0.0 at
 * the top level and nothing cancels) and the two totals run in an order that is a pure function of nz.  A column gives
 * the same bits alone, at any position in any batch and on a repeated call.  dz must be positive: stated, not checked.
 * Inputs are assumed finite and physical; a NaN input is memory-safe and gives unspecified values.
 *
 * Not modelled: Mie efficiencies and any wavelength dependence of the particles, depolarisation, off-zenith beams,
 * overlap and noise, aerosol backscatter, entries over several devices.
 */
#ifndef KIDMP_LIDAR_H
#define KIDMP_LIDAR_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_LIDAR_SUMMARY_N 8
enum { KIDMP_LIDAR_TAU_PART = 0, KIDMP_LIDAR_TAU_MOL, KIDMP_LIDAR_Z_BASE_UP, KIDMP_LIDAR_Z_LOST_UP, KIDMP_LIDAR_Z_TOP_DN,
       KIDMP_LIDAR_Z_LOST_DN, KIDMP_LIDAR_N_UP, KIDMP_LIDAR_N_DN };

/* s_ratio: the lidar ratios S_x in sr, in the order c, i, r, s, g; eta: multiple-scattering factor; c_mol: molecular
 * backscatter cross-section in m2 sr-1; beta_detect in m-1 sr-1; trans_lost: a two-way transmission.  A NULL cfg means
 * { {18.8, 25, 18.8, 25, 25}, 0.7, 6.2446e-32, 2e-5, 2.5e-3 }: conventions of this library, none of them checked against
 * a source (6.2446e-32 is a 532-nm figure).
 * KIDMP_EINVAL: a member that is not finite, a ratio <= 0, eta outside (0, 1], c_mol < 0, c_mol == 0 with sr_* wanted. */
typedef struct kidmp_lidar_cfg { double s_ratio[5]; double eta, c_mol, beta_detect, trans_lost; } kidmp_lidar_cfg;

/* Each member is [ncol][nz] or NULL (not wanted: it costs no store).  When nothing beyond ext_*, ext, bsc and bsc_mol is
 * asked for (and no summary), the kernel runs no scan and no exponential, and dz is not read and may be NULL.
 * kidmp32_lidar_out: binary64 inside, one rounding on store. */
typedef struct kidmp_lidar_out { double *ext_c, *ext_i, *ext_r, *ext_s, *ext_g, *ext, *bsc, *bsc_mol, *tau_up, *tau_dn, *att_up, *att_dn, *sr_up, *sr_dn; } kidmp_lidar_out;
typedef struct kidmp32_lidar_out { float *ext_c, *ext_i, *ext_r, *ext_s, *ext_g, *ext, *bsc, *bsc_mol, *tau_up, *tau_dn, *att_up, *att_dn, *sr_up, *sr_dn; } kidmp32_lidar_out;

/*   out, summary   either may be NULL; at least one member of out or the summary must be asked for.  summary is
 *                  [ncol][KIDMP_LIDAR_SUMMARY_N], binary64 in all four entries
 *   dz, dz_col_stride   as in kidmp_column_summary_device: 0 = one profile of nz values for all columns, otherwise >= nz
 * The device entries never allocate, never synchronise and enqueue one launch on `stream`: they can be captured into a
 * hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on its
 * compute stream, then synchronise; only what was asked for comes down, and the results equal the device entry's bit
 * for bit for any chunking (kidmp_set_host_chunk).
 * KIDMP_EINVAL, nothing written: a required NULL (t, p, qv, qc, qr, nr; dz when a depth, an attenuated profile, a ratio or
 * the summary is wanted), nz outside [2, KIDMP_MAX_NZ], ncol < 0, nothing requested at all, dz_col_stride neither 0 nor
 * >= nz, a cfg refused above, a frozen input (qi, ni, qs, qg) missing in a mixed-phase context, nc missing in an
 * aerosol-aware context, ncol other than the columns kidmp_set_column_nc bound, a pointer that is not memory of the
 * context's device (device entries).  A NULL context returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK.  A context whose
 * exponents are not the ones the closed forms take (bm_s = 2, mu_r = mu_g = mu_i = 0) returns KIDMP_ESTATE. */
int kidmp_lidar_profiles_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *nc,
        const double *qi, const double *ni, const double *qr, const double *nr, const double *qs, const double *qg,
        const double *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
        const kidmp_lidar_out *out, double *summary, void *stream);
int kidmp32_lidar_profiles_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *nc,
        const float *qi, const float *ni, const float *qr, const float *nr, const float *qs, const float *qg,
        const float *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
        const kidmp32_lidar_out *out, double *summary, void *stream);
int kidmp_lidar_profiles_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *nc,
        const double *qi, const double *ni, const double *qr, const double *nr, const double *qs, const double *qg,
        const double *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
        const kidmp_lidar_out *out, double *summary);
int kidmp32_lidar_profiles_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *nc,
        const float *qi, const float *ni, const float *qr, const float *nr, const float *qs, const float *qg,
        const float *dz, int64_t dz_col_stride, const kidmp_lidar_cfg *cfg,
        const kidmp32_lidar_out *out, double *summary);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_LIDAR_H */
