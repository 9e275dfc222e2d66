/*
 * kidmp_mie.h -- a cloud-radar operator: Mie reflectivity and path attenuation at a chosen wavelength.
 *
 * Every other radar diagnostic of the library is Rayleigh scattering at 10 cm without attenuation.  Here each species'
 * particles are Lorenz-Mie spheres at the caller's wavelength: a table of five numbers per diameter bin is built once on
 * the host (kidmp_mie_table_create) and one launch of kidmp::k_mie_radar folds it into the scheme's size distributions.
 * The particle models and every definition below are the project's own convention: parity with an instrument simulator
 * is unpinned.  Conventions as in kidmp.h and kidmp_brightband.h (return codes, device binding, [ncol][nz] arrays with k
 * fastest, k = 0 the lowest level).  In binary64, every operation rounded once, no contraction:
 *
 *   sphere    Bohren & Huffman's series for size parameter x = pi D/lambda and index m = n + i k, k >= 0: D_n(mx) by
 *             downward recurrence from max(nstop, |mx|) + 15, the Riccati-Bessel functions upward,
 *             nstop = int(x + 4 x**(1/3) + 2).  Q_ext and Q_back = |sum (2n+1)(-1)**n (a_n - b_n)|**2 / x**2, whose Rayleigh
 *             limit is 4 x**4 |K(m**2)|**2, K(e) = (e - 1)/(e + 2).  (kid_amd/csrc/kidmp_mie_sphere.h)
 *   particle  rain: a water sphere of diameter D, m = sqrt(eps_w), mass (PI/6) rho_w D**3.  Snow: a soft sphere of
 *             diameter D and mass am_s D**bm_s, ice volume fraction f = min(1, mass/(rho_i (PI/6) D**3)), permittivity of
 *             ice in air by Maxwell-Garnett (1 + 2 f K(eps_i))/(1 - f K(eps_i)).  Graupel: the same with am_g D**bm_g.
 *   rows      per species and bin (D, dD), in this order:
 *               0 s_mie   lambda**4/(pi**5 kw2) * sigma_back, m**6
 *               1 s_ray   what the closed-form ze_x of M:5127-5136 integrates: D**6 (rain), ZE_SNOW_FAC D**4 (snow),
 *                         ZE_GRAUPEL_FAC D**6 (graupel), on the same scale
 *               2 s_ext   sigma_ext, m**2
 *               3 mass    kg
 *               4 v0      av_x D**bv_x exp(-fv_x D), the fall speed at RHO_NOT, m/s
 *   load      that of kidmp_doppler_moments_device through the same functions (M:4991-5103): rho, L_qr, L_qs, L_qg, ze_r,
 *             ze_s, ze_g (those of kidmp_reflectivity_device bit for bit), rain's lamr and N0_r, snow's smob and smoc,
 *             graupel's lamg and N0_g after the running minimum of its intercept; cloud water is present where qc > R1.
 *             qc, qs or qg NULL mean zero; an iiwarm context has no snow or graupel.  Inputs are never written.
 *   density   n = N_x(D_b)*dD_b, the density kidmp_spectra.h gives the species at that level and bin (rain, graupel:
 *             N0*E(lam*D); snow: the Field shape; E(x) = exp(-x), +0.0 beyond 700).
 *   sums      per level and present species, over the bins ascending into accumulators that start at +0.0:
 *             A = sum n*s_mie, B = sum n*s_ray, E = sum n*s_ext, M = sum n*mass, V = sum (n*s_mie)*v0.
 *   carriers  every output is carried by a closed-form quantity, so the grid's quadrature and truncation cancel:
 *             mie_x = A/B, exactly 1.0 where the species is absent or B is not above 0;  ze_x' = ze_x*mie_x;
 *             dbz = 10*log10(((ze_r' + ze_s') + ze_g')*1e18), dbz_x of ze_x' alone;
 *             ext_x = (rho*q_x)*E/M in 1/m, +0.0 where the species is absent or M is not above 0;
 *             ext_c = kc*((rho*qc)/rho_w) where qc > R1, kc = (6 pi/lambda)*Im(K(eps_w)): Rayleigh absorption (with
 *             Im(eps) >= 0 the absorbing part of K is +Im(K));
 *             ext = (((ext_r + ext_s) + ext_g) + ext_c) + k_gas, k_gas the caller's one-way gas extinction in 1/m;
 *             vd = rhof*((sum_x ze_x'*(V_x/A_x))/(sum_x ze_x')) - w over the species that are present with A_x above 0,
 *             in the order r, s, g; +0.0 where there is none (w is not applied), as in kidmp_doppler.h.
 *   path      tau_up[k] = sum_{j<k} ext_j*dz_j + 0.5*(ext_k*dz_k) and tau_down from the top, by the wave scans of
 *             kidmp_lidar.h (a reversed scan, nothing cancels); pia_up = c*tau_up with c = 20/ln 10, in dB, two-way;
 *             dbz_up = dbz - pia_up; pia_down, dbz_down likewise; pia_total[col] = c * sum_k ext_k*dz_k.
 *   outputs   dbz, dbz_up, dbz_down, dbz_r, dbz_s, dbz_g, mie_r, mie_s, mie_g, ext, pia_up, pia_down, vd [ncol][nz] and
 *             pia_total [ncol]; binary64 inside, the kidmp32_ entries round once on store.  A NULL costs no store; a
 *             request without dbz_up, dbz_down, pia_up and pia_down runs no scan.  The bits of a column do not depend on
 *             the batch, on its position, on a repeated call or on which outputs were requested.
 *
 * Not modelled: non-spherical particles, melting particles (kidmp_brightband.h is Rayleigh), multiple scattering,
 * temperature-dependent permittivities, cloud ice.
 */
#ifndef KIDMP_MIE_H
#define KIDMP_MIE_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_MIE_NSPECIES 3
#define KIDMP_MIE_R 0
#define KIDMP_MIE_S 1
#define KIDMP_MIE_G 2
#define KIDMP_MIE_MAX_BINS 256
#define KIDMP_MIE_NROWS 5

/* kidmp_mie_defaults writes wavelength = 0.10 m, eps_w = 79.5 + 24.9i and eps_i = (1 + 2k)/(1 - k) + 0i with
 * k = sqrt(0.176) (the bright band's permittivities), rho_w = 1000, rho_i = 900, kw2 = 0.93.  A cloud-radar user passes
 * the wavelength and the permittivities of water and ice at that wavelength and temperature; the library holds none.
 * Im(eps) >= 0 marks absorption. */
typedef struct kidmp_mie_cfg {
    double wavelength;
    double eps_w_re, eps_w_im;
    double eps_i_re, eps_i_im;
    double rho_w, rho_i;
    double kw2;
} kidmp_mie_cfg;
void kidmp_mie_defaults(kidmp_mie_cfg *cfg);

/* The diameter grids of rain, snow and graupel as in kidmp_brightband_grids: D[x] and dD[x] both NULL = the scheme's own
 * 100 bins of the context (nb[x] is not read), or both host arrays of nb[x] values, 1 <= nb[x] <= KIDMP_MIE_MAX_BINS. */
typedef struct kidmp_mie_grids {
    const double *D[KIDMP_MIE_NSPECIES];
    const double *dD[KIDMP_MIE_NSPECIES];
    int32_t nb[KIDMP_MIE_NSPECIES];
} kidmp_mie_grids;

/* Each member is an array of the shape stated above or NULL (not wanted: no store).  At least one must be asked for. */
typedef struct kidmp_mie_out { double *dbz, *dbz_up, *dbz_down, *dbz_r, *dbz_s, *dbz_g, *mie_r, *mie_s, *mie_g, *ext, *pia_up, *pia_down, *vd; double *pia_total; } kidmp_mie_out;
typedef struct kidmp32_mie_out { float *dbz, *dbz_up, *dbz_down, *dbz_r, *dbz_s, *dbz_g, *mie_r, *mie_s, *mie_g, *ext, *pia_up, *pia_down, *vd; float *pia_total; } kidmp32_mie_out;

typedef struct kidmp_mie_table kidmp_mie_table;

/* Host entries that need no context and no device.  KIDMP_EINVAL, nothing written: a NULL; x, m or a member of cfg that is
 * not finite; x, Re(m), wavelength, rho_w, rho_i, kw2 or a diameter not above 0; Im(m) or Im(eps) below 0; Re(eps) not
 * above 0 with Im(eps) = 0; an unknown species; nb < 1; a sphere of more than ten million terms.
 * rows is [KIDMP_MIE_NROWS][nb]. */
int kidmp_mie_sphere(double x, double m_re, double m_im, double *qext, double *qback);
int kidmp_mie_bins(const kidmp_mie_cfg *cfg, int32_t species, int32_t nb, const double *D, double *rows);

/* The table: the rows of the three species on their grids, built on the host and uploaded to the context's device.  It
 * may allocate and synchronise.  cfg NULL = the defaults; grids NULL = the scheme's own bins for every species.  The table
 * holds its own copy of everything (the caller's grids may be freed) and belongs to the context it was made with:
 * destroy it before that context's kidmp_finalize.  KIDMP_EINVAL as for kidmp_mie_bins, and for grids with one of
 * D / dD NULL alone, nb outside [1, KIDMP_MIE_MAX_BINS] or a dD that is not finite; *table is then NULL. */
int kidmp_mie_table_create(kidmp_ctx *ctx, const kidmp_mie_cfg *cfg, const kidmp_mie_grids *grids, kidmp_mie_table **table);
void kidmp_mie_table_destroy(kidmp_mie_table *table);
/* Copies a species' grid and rows back to the host: *nb always; D[nb], dD[nb], rows[KIDMP_MIE_NROWS][nb] where not NULL,
 * read back from the device.  cfg, where not NULL, receives the table's configuration. */
int kidmp_mie_table_get(const kidmp_mie_table *table, int32_t species, int32_t *nb, double *D, double *dD, double *rows, kidmp_mie_cfg *cfg);

/* The device entries never allocate, never synchronise and enqueue exactly one launch on `stream`: they can be captured
 * into a hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on
 * its compute stream, then synchronise; the results equal the device entry's bit for bit for any chunking
 * (kidmp_set_host_chunk).  dz with dz_col_stride and k_gas with k_gas_col_stride as dz in kidmp_column_summary_device:
 * stride 0 = one profile of nz values for all columns, otherwise >= nz.  qc, qs, qg, w and k_gas may be NULL (zero); dz
 * may be NULL when no dbz_up, dbz_down, pia_up, pia_down or pia_total is wanted.
 * KIDMP_EINVAL, nothing written: a NULL table or a table of another context; a NULL among t, p, qv, qr, nr; dz NULL where
 * it is needed; nz outside [2, KIDMP_MAX_NZ]; ncol < 0; a stride that is neither 0 nor >= nz; out NULL or all its
 * members NULL; a pointer that is not memory of the context's device (device entries).  A NULL context, or one whose
 * exponents are not those the kernel takes as integers, returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_mie_radar_device(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const double *w,
        const double *k_gas, int64_t k_gas_col_stride, const kidmp_mie_out *out, void *stream);
int kidmp32_mie_radar_device(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const float *w,
        const float *k_gas, int64_t k_gas_col_stride, const kidmp32_mie_out *out, void *stream);
int kidmp_mie_radar_host(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *dz, int64_t dz_col_stride, const double *w,
        const double *k_gas, int64_t k_gas_col_stride, const kidmp_mie_out *out);
int kidmp32_mie_radar_host(kidmp_ctx *ctx, const kidmp_mie_table *table, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *dz, int64_t dz_col_stride, const float *w,
        const float *k_gas, int64_t k_gas_col_stride, const kidmp32_mie_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_MIE_H */
