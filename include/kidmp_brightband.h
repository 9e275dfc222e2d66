/*
 * kidmp_brightband.h -- the radar bright band: melting snow and graupel in the 10-cm reflectivity.
 *
 * calc_refl10cm as the reference ships it treats snow and graupel below the melting level as dry ice: the melting-layer
 * block (M:5140-5192) keeps its level search and its melt fractions, but its integration loops are empty (nrbins = 0,
 * M:204) and the calls into the wet-particle scattering model are commented out.  kidmp_bright_band_device rebuilds that
 * block from what the reference keeps -- the melting level, the melt fraction, which distribution is integrated -- and a
 * per-particle dielectric model of its own (Maxwell-Garnett mixing, Rayleigh backscatter), in one launch of
 * kidmp::k_bright_band.  The definitions are the project's own: parity with another radar simulator is unpinned.
 * Conventions as in kidmp.h and kidmp_dspectrum.h (return codes, device binding, [ncol][nz] arrays with k fastest,
 * k = 0 the lowest level).  In binary64, every operation rounded once, no contraction:
 *
 *   load      that of kidmp_doppler_moments_device through the same functions (M:4991-5103): rho, rs = qs*rho, rg = qg*rho,
 *             L_qr, L_qs, L_qg, ze_r, ze_s, ze_g, snow's smob and smoc, graupel's lamg and N0_g after the running minimum
 *             of its intercept.  qs or qg NULL mean zero.  Inputs are never written.
 *   level     k0 = k + 1 for the highest k in [0, nz-2] with t[k] > 273.15, L_qr[k] and (L_qs[k+1] or L_qg[k+1])
 *             (M:5109-5118); none, or an iiwarm context: k0 = -1 and every output is the dry one.
 *   fraction  for k < k0: snow is active where L_qs[k] and L_qs[k0], fm_s = max(0.05, min(1 - rs[k]/rs[k0], 0.99))
 *             (M:5152); graupel likewise with rg and L_qg (M:5176).  Elsewhere fm = +0.0 and the species is dry.
 *   particle  per diameter bin (D, dD), with K(e) = (e - 1)/(e + 2) in complex arithmetic (division by one real
 *             reciprocal of |z|**2):
 *               m   = am_x * D**bm_x                   (bm_s = 2: D*D; bm_g = 3: D*D*D)
 *               Vi0 = m / rho_i;  Ve = max((PI/6)*D*D*D, Vi0)       the unmelted particle's ice and its envelope
 *               Vi  = (1 - fm)*Vi0;  Vw = (fm*m)/rho_w;  Va = (1 - fm)*(Ve - Vi0);  c = Vi + Va;  V = c + Vw
 *               Kc  = (Vi/c) * K(eps_i)                ice inclusions in air;  eps_c = (1 + 2Kc)/(1 - Kc)
 *               KIDMP_BB_WATER_MATRIX:  g = c/V;   b = (eps_c - eps_w)/(eps_c + 2 eps_w);  eps_p = eps_w*((1 + 2 g b)/(1 - g b))
 *               KIDMP_BB_ICE_MATRIX:    g = Vw/V;  b = (eps_w - eps_c)/(eps_w + 2 eps_c);  eps_p = eps_c*((1 + 2 g b)/(1 - g b))
 *               s   = |K(eps_p)|**2 * V*V   (wet);      s0 = K(eps_i)**2 * Vi0*Vi0   (dry)
 *               n   = N_x(D)*dD, the density kidmp_spectra.h gives the species at that level and bin from the parameters
 *                     above (snow: the Field shape; graupel: N0_g*E(lamg*D); E(x) = exp(-x), +0.0 beyond 700)
 *   D grids   per species (KIDMP_BB_S, KIDMP_BB_G) as in kidmp_dspectrum.h: NULL = the scheme's own 100 bins Ds/dts, Dg/dtg,
 *             or D[nb], dD[nb] with 1 <= nb <= KIDMP_BB_MAX_BINS, always binary64.
 *   enhance   E_x[k] = (sum_b n s)/(sum_b n s0), exactly 1.0 where the species is not active or the denominator is not
 *             above 0.  The quadrature error of the grid cancels in the ratio and the closed-form ze_x stays the carrier:
 *             ze_s' = ze_s*E_s, ze_g' = ze_g*E_g, dbz = 10*log10((ze_r + ze_s' + ze_g')*1e18) (M:5196).  Towards fm = 1 the
 *             ratio tends to that of a water sphere of the melted mass.
 *   order     lane j of the wavefront takes bins j, j+64, ... ascending into binary64 accumulators that start at +0.0; the
 *             64 partial sums are combined by a butterfly over xor 32, 16, ..., 1.  The bits of a column do not depend on
 *             the batch, on its position, on a repeated call or on which outputs were requested.
 *   outputs   dbz, dbz_s, dbz_g [ncol][nz] (dbz_s, dbz_g: the dBZ of ze_s' and ze_g' alone); enh_s, enh_g [ncol][nz],
 *             linear; fmelt_s, fmelt_g [ncol][nz]; k0 int32 [ncol].
 *
 * Not modelled: Mie scattering, attenuation, temperature-dependent permittivities; the enhancement is not fed into the
 * Doppler moments and spectra.
 */
#ifndef KIDMP_BRIGHTBAND_H
#define KIDMP_BRIGHTBAND_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_BB_NSPECIES 2
#define KIDMP_BB_S 0
#define KIDMP_BB_G 1
#define KIDMP_BB_MAX_BINS 256
#define KIDMP_BB_WATER_MATRIX 0
#define KIDMP_BB_ICE_MATRIX 1

/* NULL in place of the configuration means the defaults, which kidmp_brightband_defaults writes: eps_w = 79.5 + 24.9i
 * (10 cm, 0 C, single Debye relaxation; |K_w|**2 = 0.934), eps_i = (1 + 2k)/(1 - k) with k = sqrt(0.176) (|K_i|**2 is the
 * scheme's 0.176), rho_w = 1000, rho_i = 900 (the scheme's own 900.0 of M:5132-5136), kw2 = 0.93 (the normalisation the
 * carrier ze_x holds), topology = KIDMP_BB_WATER_MATRIX. */
typedef struct kidmp_brightband_cfg {
    double eps_w_re, eps_w_im;
    double eps_i;
    double rho_w, rho_i;
    double kw2;
    int32_t topology;
} kidmp_brightband_cfg;
void kidmp_brightband_defaults(kidmp_brightband_cfg *cfg);

/* Each member is an array of the shape stated above or NULL (not wanted: no store).  At least one member must be asked
 * for.  kidmp32_brightband_out: binary64 inside, one rounding on store. */
typedef struct kidmp_brightband_out { double *dbz, *dbz_s, *dbz_g, *enh_s, *enh_g, *fmelt_s, *fmelt_g; int32_t *k0; } kidmp_brightband_out;
typedef struct kidmp32_brightband_out { float *dbz, *dbz_s, *dbz_g, *enh_s, *enh_g, *fmelt_s, *fmelt_g; int32_t *k0; } kidmp32_brightband_out;
/* The diameter grids of snow and graupel: D[x] and dD[x] both NULL = the scheme's own grid (nb[x] is not read), or both
 * arrays of nb[x] values.  Device memory for the device entries, host memory for the host entries. */
typedef struct kidmp_brightband_grids {
    const double *D[KIDMP_BB_NSPECIES];
    const double *dD[KIDMP_BB_NSPECIES];
    int32_t nb[KIDMP_BB_NSPECIES];
} kidmp_brightband_grids;

/* The device entries never allocate, never synchronise and enqueue exactly one launch on `stream`: they can be captured
 * into a hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on
 * its compute stream, then synchronise; the results equal the device entry's bit for bit for any chunking
 * (kidmp_set_host_chunk).
 * KIDMP_EINVAL, nothing written: a NULL among t, p, qv, qr, nr; nz outside [2, KIDMP_MAX_NZ]; ncol < 0; out NULL or all
 * its members NULL; a configuration with a member that is not finite, rho_w, rho_i or kw2 not above 0, or an unknown
 * topology; grids with one of D / dD NULL alone or nb outside [1, KIDMP_BB_MAX_BINS]; a pointer that is not memory of
 * the context's device (device entries).  A NULL context, or one whose exponents are not those the kernel takes as
 * integers, returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_bright_band_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const kidmp_brightband_cfg *cfg,
        const kidmp_brightband_grids *grids, const kidmp_brightband_out *out, void *stream);
int kidmp32_bright_band_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const kidmp_brightband_cfg *cfg,
        const kidmp_brightband_grids *grids, const kidmp32_brightband_out *out, void *stream);
int kidmp_bright_band_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const kidmp_brightband_cfg *cfg,
        const kidmp_brightband_grids *grids, const kidmp_brightband_out *out);
int kidmp32_bright_band_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const kidmp_brightband_cfg *cfg,
        const kidmp_brightband_grids *grids, const kidmp32_brightband_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_BRIGHTBAND_H */
