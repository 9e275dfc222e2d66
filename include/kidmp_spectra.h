/*
 * kidmp_spectra.h -- the scheme's size distributions on diameter bins, on the device.
 *
 * Comparing a bulk scheme with a bin scheme or with an instrument is done on size distributions.  The other diagnostics
 * give integrals of the Thompson distributions (reflectivity, radii, fall speeds, Doppler moments); this one gives the
 * distributions themselves: per level the slope and intercept of every species as mp_thompson loads the state, and the
 * number of particles per m3 of air in each bin of a diameter grid, formed as the reference's table builders form their
 * N_x(n) (M:3768, M:3967-3975, M:4157-4164, M:4206-4221).  One launch of kidmp::k_size_spectra.  Conventions as in
 * kidmp.h and kidmp_fall.h (return codes, device binding, [ncol][nz] arrays with k fastest, k = 0 the lowest level).
 * Species in a fixed order: cloud water c, cloud ice i, rain r, snow s, graupel g (KIDMP_SPECTRA_C .. KIDMP_SPECTRA_G).
 * In binary64:
 *
 *   load      that of kidmp_fall_speeds_device: rho from qv' = max(1e-10, qv); rain, ice, snow and graupel as M:1420-1492
 *             load them, with the number limiting of ice and rain; snow's smob and smoc of block D; graupel's slope and
 *             intercept of block E with the running minimum of the intercept from the top down.  Cloud water as
 *             M:1395-1410 loads it: nc = Nt_c in a context that is not aerosol-aware (the column's own where
 *             kidmp_set_column_nc bound one, as calc_effectRad honours it; nc is not read and may be NULL); in an
 *             aerosol-aware context nc = MAX(2, nc*rho) limited through xDc (M:1402-1409).  Then nu_c and lamc as block G
 *             forms them (M:1690-1692).  The input arrays are never written.
 *   params    n0_r = nr*org2*lamr**cre(2); n0_g = N0_exp/(cgg(2)*lam_exp)*lamg**cge(2); n0_i = ni*oig1*lami**cie(1);
 *             n0_c = nc*ocg1(nu_c)*lamc**cce(1,nu_c); nu_c (an integer in 2..15) is stored as a floating number; smob
 *             and smoc are snow's moments of order bm_s and cse(1).  Cloud water's gamma functions of integers are exact
 *             (ccg(2,n)*ocg1(n) = (n+1)(n+2)(n+3) as in calc_effectRad's g_ratio, ccg(1,n) = n!), where thompson_init's
 *             WGAMMA is off by up to 9e-12.  A level whose species is absent (q <= R1) has exact
 *             +0.0 in all of the species' parameters: nothing is inherited from the level above.
 *   spectra   N_x[ncol][nb_x][nz], the level fastest: particles per m3 of air in bin b,
 *               rain, graupel, ice   N0 * D_b**mu * EXP(-lam*D_b) * dD_b           (mu_r = mu_g = mu_i = 0)
 *               cloud water          N0_c * D_b**nu_c * EXP(-lamc*D_b) * dD_b
 *               snow, r = smob/smoc  smob*r**3 * (Kap0*EXP(-r*Lam0*D_b) + Kap1*r**mu_s*D_b**mu_s*EXP(-r*Lam1*D_b)) * dD_b
 *             An absent species has +0.0 in all its bins.
 *   underflow An exponential whose argument lam*D_b (snow: r*Lam0*D_b, r*Lam1*D_b) exceeds 700 contributes exact +0.0
 *             (on the scheme's own grids lami*Di reaches 783 and lamc*Dc 1 600).  Below that every factor is a normal
 *             number, and the product is formed intercept first, in an order that cannot overflow.
 *   grids     per species a pair D[nb], dD[nb] of bin diameters and widths (m; positive, finite), 1 <= nb <=
 *             KIDMP_SPECTRA_MAX_BINS, always binary64.  NULL means the scheme's own KIDMP_SPECTRA_DEFAULT_BINS bins, Dc/dtc
 *             .. Dg/dtg of M:605-657, which every context holds on the device; kidmp_spectra_default_grid copies them out.
 *             A caller grid puts the spectra on a bin scheme's own bins (mass-doubling bins, say).
 *
 * An iiwarm context: qi, ni, qs and qg are not read and may be NULL; the frozen parameters and bins are exact +0.0 and
 * their output pointers may be NULL.  A column gives the same bits alone, at any position in any batch, on a repeated
 * call, and however the launch deals its bins to workgroups.  Inputs are assumed finite; a NaN input is memory-safe and
 * gives unspecified values.
 *
 * Not modelled: a Doppler spectrum on a velocity grid, exact incomplete-gamma integrals over the bins (a bin is the
 * density at D_b times dD_b, as in the reference), bin moments on the device, entries over several devices, and any change
 * to the column step.
 */
#ifndef KIDMP_SPECTRA_H
#define KIDMP_SPECTRA_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_SPECTRA_NSPECIES 5
#define KIDMP_SPECTRA_C 0
#define KIDMP_SPECTRA_I 1
#define KIDMP_SPECTRA_R 2
#define KIDMP_SPECTRA_S 3
#define KIDMP_SPECTRA_G 4
#define KIDMP_SPECTRA_MAX_BINS 256
#define KIDMP_SPECTRA_DEFAULT_BINS 100

/* The parameters: each member is [ncol][nz] or NULL (not wanted: it costs no store).  kidmp32_*: binary64 inside, one
 * rounding on store; n0_c can lie beyond binary32's range (it reaches 1e111) and is then stored as +infinity. */
typedef struct kidmp_spectra_out { double *lam_c, *n0_c, *nu_c, *lam_i, *n0_i, *lam_r, *n0_r, *smob, *smoc, *lam_g, *n0_g; } kidmp_spectra_out;
typedef struct kidmp32_spectra_out { float *lam_c, *n0_c, *nu_c, *lam_i, *n0_i, *lam_r, *n0_r, *smob, *smoc, *lam_g, *n0_g; } kidmp32_spectra_out;
/* The spectra: each member is [ncol][nb_x][nz] or NULL (not wanted). */
typedef struct kidmp_spectra_bins { double *n_c, *n_i, *n_r, *n_s, *n_g; } kidmp_spectra_bins;
typedef struct kidmp32_spectra_bins { float *n_c, *n_i, *n_r, *n_s, *n_g; } kidmp32_spectra_bins;
/* The grids, by species: D[x] and dD[x] both NULL = the scheme's own grid (nb[x] is not read), or both arrays of nb[x]
 * values.  Device memory for the device entries, host memory for the host entries. */
typedef struct kidmp_spectra_grids {
    const double *D[KIDMP_SPECTRA_NSPECIES];
    const double *dD[KIDMP_SPECTRA_NSPECIES];
    int32_t nb[KIDMP_SPECTRA_NSPECIES];
} kidmp_spectra_grids;

/* Copies the scheme's own grid of `species` to the host arrays D and dD of `cap` values and returns its number of bins;
 * with D and dD both NULL it only returns the number.  KIDMP_EINVAL: species out of range, one of D / dD NULL alone,
 * cap too small.  A NULL context returns KIDMP_ESTATE. */
int kidmp_spectra_default_grid(kidmp_ctx *ctx, int32_t species, double *D, double *dD, int32_t cap);

/*   par, bins   either may be NULL; at least one member of the two must be asked for
 *   grids       NULL = the scheme's own grid for every species; a species whose spectrum is not wanted is not looked at
 * The device entries never allocate, never synchronise and enqueue one launch on `stream`: they can be captured into a
 * hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on its
 * compute stream, then synchronise; the caller's grids go up once, only what was asked for comes down, and the results
 * equal the device entry's bit for bit for any chunking (kidmp_set_host_chunk).
 * KIDMP_EINVAL, nothing written: a required NULL (t, p, qv, qc, qr, nr), nz outside [2, KIDMP_MAX_NZ], ncol < 0, nothing
 * requested at all, nb outside [1, KIDMP_SPECTRA_MAX_BINS] or one of D / dD NULL alone for a wanted spectrum, a frozen
 * input (qi, ni, qs, qg) missing in a mixed-phase context when a frozen output is wanted, nc missing in an aerosol-aware
 * context when a cloud-water output is wanted, ncol other than the columns kidmp_set_column_nc bound, a pointer that is
 * not memory of the context's device (device entries).  A NULL context returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK.
 * A context whose exponents are not the ones the kernel takes as integers returns KIDMP_ESTATE. */
int kidmp_size_spectra_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *nc,
        const double *qi, const double *ni, const double *qr, const double *nr, const double *qs, const double *qg,
        const kidmp_spectra_out *par, const kidmp_spectra_bins *bins, const kidmp_spectra_grids *grids, void *stream);
int kidmp32_size_spectra_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *nc,
        const float *qi, const float *ni, const float *qr, const float *nr, const float *qs, const float *qg,
        const kidmp32_spectra_out *par, const kidmp32_spectra_bins *bins, const kidmp_spectra_grids *grids, void *stream);
int kidmp_size_spectra_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qc, const double *nc,
        const double *qi, const double *ni, const double *qr, const double *nr, const double *qs, const double *qg,
        const kidmp_spectra_out *par, const kidmp_spectra_bins *bins, const kidmp_spectra_grids *grids);
int kidmp32_size_spectra_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qc, const float *nc,
        const float *qi, const float *ni, const float *qr, const float *nr, const float *qs, const float *qg,
        const kidmp32_spectra_out *par, const kidmp32_spectra_bins *bins, const kidmp_spectra_grids *grids);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_SPECTRA_H */
