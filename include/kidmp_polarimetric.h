/*
 * kidmp_polarimetric.h -- a polarimetric radar operator: Z_DR, K_DP and rho_hv of oblate spheroids at 10 cm.
 *
 * The other radar diagnostics of the library treat particles as spheres.  Here each species' particles are oblate
 * spheroids in the Rayleigh-Gans approximation: a table of seven numbers per diameter bin is built once on the host
 * (kidmp_pol_table_create) and one launch of kidmp::k_polarimetric folds it into the scheme's size distributions.  The
 * particle models, the canting moments and every definition below are the project's own convention: parity with an
 * instrument simulator is unpinned.  The header stands over kidmp_mie.h: it reuses kidmp_mie_cfg (wavelength, the
 * permittivities and densities; kw2 is not read), kidmp_mie_grids and the species indices KIDMP_MIE_R, _S, _G.
 * Conventions as in kidmp.h and kidmp_mie.h (return codes, device binding, [ncol][nz] arrays with k fastest, k = 0 the
 * lowest level).  In binary64, every operation rounded once, no contraction:
 *
 *   particle  an oblate spheroid of equal-volume diameter D and axis ratio r = b/a <= 1, the symmetry axis a vertical in
 *             the mean.  f**2 = 1/r**2 - 1;  L_a = ((1 + f**2)/f**2)(1 - atan(f)/f), by its series of twelve terms for
 *             f**2 < 1/64;  L_b = 0.5 (1 - L_a);  r >= 1: L_a = L_b = 1.0/3.0, the sphere.
 *             P_j = (eps - 1)/(3 (1 + L_j (eps - 1))), j = a, b;  P(1/3) = K(eps);  Delta = P_b - P_a.
 *             (kid_amd/csrc/kidmp_spheroid.h)
 *   canting   Gaussian with zero mean and width sigma (radians, per species).  With q = exp(-2 sigma**2) the angular
 *             moments of Ryzhkov et al. (2011), J. Appl. Meteor. Climatol. 50:
 *               A1 = (1/4)(1 + q)**2                A2 = (1/4)(1 - q**2)
 *               A3 = (3/8 + q/2 + q**4/8)**2         A4 = (3/8 - q/2 + q**4/8)(3/8 + q/2 + q**4/8)
 *               A5 = (1/8)(3/8 + q/2 + q**4/8)(1 - q**4)                  A7 = (1/2) q (1 + q)
 *   species   rain: water, eps_w, r(D) = clamp(c0 + d (c1 + d (c2 + d (c3 + d c4))), r_min, 1) with d = D*1e3 and
 *             c = axis_r.  Snow and graupel: the soft particle of kidmp_mie.h (ice volume fraction
 *             min(1, mass/(rho_i (PI/6) D**3)), Maxwell-Garnett ice in air) with the constant axis ratios axis_s, axis_g.
 *   rows      per species and bin (D, dD), in this order:
 *               0 s_h   D**6 (|P_b|**2 - 2 A2 Re(conj(P_b) Delta) + A4 |Delta|**2)
 *               1 s_v   the same with A1, A3
 *               2 c_re, 3 c_im   D**6 (|P_b|**2 + A5 |Delta|**2 - A1 conj(P_b) Delta - A2 P_b conj(Delta))
 *               4 s_0   D**6 |P(1/3)|**2, the equal-volume sphere
 *               5 k     D**3 Re(Delta) A7
 *               6 mass  kg, as row 3 of the Mie table
 *             With Delta = 0 (every axis ratio 1) the rows 0, 1, 2 and 4 are the same bits and row 3 is +0.0.
 *   uniform   a species whose permittivity and axis ratio do not depend on D (a constant axis ratio and a mass exponent of
 *             3: graupel in this scheme) has the same ratios s_h/s_0, s_v/s_0, c_re/s_0, c_im/s_0 and k/mass in every
 *             bin.  The table holds them as five scalars, formed from the rows of the species' first bin, and the kernel
 *             takes them in place of the sums: no loop over the bins and no density for that species.
 *             force_quadrature != 0 marks no species uniform.
 *   load      that of kidmp_mie_radar_device through the same functions: rho, L_qr, L_qs, L_qg, ze_r, ze_s, ze_g (those of
 *             kidmp_reflectivity_device bit for bit), the distributions' slopes and intercepts, graupel's after the running
 *             minimum of its intercept.  qs or qg NULL mean zero; an iiwarm context has no snow or graupel.
 *   density   n = N_x(D_b)*dD_b, the density kidmp_spectra.h gives the species at that level and bin.
 *   sums      per level and present species, over the bins ascending into accumulators that start at +0.0:
 *             H = sum n*s_h, V = sum n*s_v, Cr = sum n*c_re, Ci = sum n*c_im, S = sum n*s_0, K = sum n*k, M = sum n*mass.
 *   carriers  every output is carried by a closed-form quantity, so the grid's quadrature and truncation cancel:
 *             zh_x = ze_x*(H/S), zv_x = ze_x*(V/S), c_x = ze_x*(Cr/S, Ci/S); each ratio is exactly 1.0 (for Ci, +0.0) where
 *             the species is absent or S is not above 0;
 *             Zh = (zh_r + zh_s) + zh_g, Zv and C = (Cre, Cim) likewise;
 *             dbz_h = 10*log10(Zh*1e18), dbz_h_x of zh_x alone;  zdr = 10*log10(Zh/Zv), zdr_x of zh_x/zv_x;
 *             rhohv = min(1, sqrt(Cre**2 + Cim**2)/sqrt(Zh*Zv));
 *             kdp_x = ((90e3*pi/lambda)*(rho*q_x))*(K/M) in degrees per km, +0.0 where the species is absent or M is not
 *             above 0;  kdp = (kdp_r + kdp_s) + kdp_g.
 *             A uniform species takes the table's scalars in place of its ratios where it is present.
 *   outputs   dbz_h, zdr, kdp, rhohv, dbz_h_r, dbz_h_s, dbz_h_g, zdr_r, zdr_s, zdr_g, kdp_r, kdp_s, kdp_g [ncol][nz];
 *             binary64 inside, the kidmp32_ entries round once on store.  A NULL costs no store; a request for one species'
 *             own profiles alone walks that species only.  The bits of a column do not depend on the batch, on its
 *             position, on a repeated call or on which outputs were requested.
 *
 * With every axis ratio 1 the operator returns kidmp_reflectivity_device's dbz bit for bit in dbz_h and dbz_h_x, +0.0 in
 * every zdr and kdp and 1.0 in rhohv, whatever sigma.  The wavelength enters kdp alone.
 *
 * Not modelled: melting particles (the bright band's wet particle is not fed in); Mie or T-matrix scattering, so only
 * wavelengths where Rayleigh-Gans holds for the particles at hand (10 cm); attenuation and differential attenuation;
 * backscatter differential phase; LDR; cloud ice; temperature-dependent permittivity or shape.
 */
#ifndef KIDMP_POLARIMETRIC_H
#define KIDMP_POLARIMETRIC_H

#include "kidmp_mie.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_POL_NROWS 7
#define KIDMP_POL_NSCALARS 5

/* kidmp_pol_defaults writes axis_r = 0.9951, 0.02510, -0.03644, 0.005303, -0.0002492 (Brandes et al. 2002, d in mm),
 * axis_r_min = 0.2, axis_s = 0.75, axis_g = 0.8, sigma = 10, 40, 40 degrees in radians (rain, snow, graupel) and
 * force_quadrature = 0.  These defaults are illustrative, not values of record. */
typedef struct kidmp_pol_cfg {
    double axis_r[5];
    double axis_r_min;
    double axis_s, axis_g;
    double sigma[KIDMP_MIE_NSPECIES];
    int32_t force_quadrature;
} kidmp_pol_cfg;
void kidmp_pol_defaults(kidmp_pol_cfg *cfg);

/* Each member is an array [ncol][nz] or NULL (not wanted: no store).  At least one must be asked for. */
typedef struct kidmp_pol_out { double *dbz_h, *zdr, *kdp, *rhohv, *dbz_h_r, *dbz_h_s, *dbz_h_g, *zdr_r, *zdr_s, *zdr_g, *kdp_r, *kdp_s, *kdp_g; } kidmp_pol_out;
typedef struct kidmp32_pol_out { float *dbz_h, *zdr, *kdp, *rhohv, *dbz_h_r, *dbz_h_s, *dbz_h_g, *zdr_r, *zdr_s, *zdr_g, *kdp_r, *kdp_s, *kdp_g; } kidmp32_pol_out;

typedef struct kidmp_pol_table kidmp_pol_table;

/* Host entries that need no context and no device.  KIDMP_EINVAL, nothing written: a NULL; an argument or a member of a
 * configuration that is not finite; Im(eps) below 0, or Re(eps) not above 0 with Im(eps) = 0; ratio, axis_r_min, axis_s or
 * axis_g outside (0, 1]; a sigma below 0; a diameter not above 0; an unknown species; nb < 1; what kidmp_mie_bins refuses
 * in mie_cfg.  kidmp_pol_spheroid writes the seven rows of a spheroid of unit diameter (D = 1; row 6, the mass, is +0.0:
 * a bare spheroid has none); rows of kidmp_pol_bins is [KIDMP_POL_NROWS][nb]. */
int kidmp_pol_spheroid(double eps_re, double eps_im, double ratio, double sigma, double *rows7_per_unit_D);
int kidmp_pol_bins(const kidmp_mie_cfg *mie_cfg, const kidmp_pol_cfg *pol_cfg, int32_t species, int32_t nb, const double *D, double *rows);

/* The table: the rows of the three species on their grids, and per species the flag `uniform` and its five scalars, built
 * on the host and uploaded to the context's device.  It may allocate and synchronise.  mie_cfg NULL = kidmp_mie_defaults;
 * pol_cfg NULL = kidmp_pol_defaults; grids NULL = the scheme's own bins for every species.  Ownership as
 * kidmp_mie_table_create: the table holds its own copy of everything and belongs to the context it was made with; destroy
 * it before that context's kidmp_finalize.  KIDMP_EINVAL as for kidmp_pol_bins and kidmp_mie_table_create; *table is then
 * NULL. */
int kidmp_pol_table_create(kidmp_ctx *ctx, const kidmp_mie_cfg *mie_cfg, const kidmp_pol_cfg *pol_cfg, const kidmp_mie_grids *grids,
        kidmp_pol_table **table);
void kidmp_pol_table_destroy(kidmp_pol_table *table);
/* Copies a species' grid and rows back to the host: *nb always; D[nb], dD[nb], rows[KIDMP_POL_NROWS][nb] where not NULL,
 * read back from the device.  mie_cfg and pol_cfg, where not NULL, receive the table's configuration; *uniform the
 * species' flag (0 or 1) and scalars[KIDMP_POL_NSCALARS] its s_h/s_0, s_v/s_0, c_re/s_0, c_im/s_0, k/mass, where not NULL. */
int kidmp_pol_table_get(const kidmp_pol_table *table, int32_t species, int32_t *nb, double *D, double *dD, double *rows,
        kidmp_mie_cfg *mie_cfg, kidmp_pol_cfg *pol_cfg, int32_t *uniform, double *scalars);

/* The device entries never allocate, never synchronise and enqueue exactly one launch on `stream`: they can be captured
 * into a hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on
 * its compute stream, then synchronise; the results equal the device entry's bit for bit for any chunking
 * (kidmp_set_host_chunk).  qs and qg may be NULL (zero).  Inputs are never written.
 * KIDMP_EINVAL, nothing written: a NULL table or a table of another context; a NULL among t, p, qv, qr, nr; nz outside
 * [2, KIDMP_MAX_NZ]; ncol < 0; out NULL or all its members NULL; a pointer that is not memory of the context's device
 * (device entries).  A NULL context, or one whose exponents are not those the kernel takes as integers, returns
 * KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_polarimetric_device(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const kidmp_pol_out *out, void *stream);
int kidmp32_polarimetric_device(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const kidmp32_pol_out *out, void *stream);
int kidmp_polarimetric_host(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const kidmp_pol_out *out);
int kidmp32_polarimetric_host(kidmp_ctx *ctx, const kidmp_pol_table *table, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const kidmp32_pol_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_POLARIMETRIC_H */
