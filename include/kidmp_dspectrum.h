/*
 * kidmp_dspectrum.h -- the Doppler spectrum of a vertically pointing radar on the device.
 *
 * A vertically pointing cloud radar records, per range gate, reflectivity as a function of radial velocity.
 * kidmp_doppler_moments_device gives the first three moments of that function; kidmp_doppler_spectrum_device gives the
 * function itself on a uniform velocity grid, from the same load, the same size distributions and the same fall-speed
 * laws, in one launch of kidmp::k_doppler_spectrum.  Conventions as in kidmp.h and kidmp_doppler.h (return codes, device
 * binding, [ncol][nz] arrays with k fastest, k = 0 the lowest level).  In binary64:
 *
 *   load      that of kidmp_doppler_moments_device, operation for operation (M:4991-5028): rho from qv' = max(1e-10, qv);
 *             rain where qr > R1 with nr = max(R2, nr1*rho), the unclamped slope lamr of M:5001 and N0_r = nr*org2*lamr;
 *             snow where qs > R2 with smob = rs*oams, smoc the Field fit at cse(1), Mrat = smob/smoc; graupel where
 *             qg > R2 with the running minimum of its intercept from the top down over all levels (M:5086-5103), then
 *             lamg and N0_g = N0_exp/(cgg(2)*lam_exp)*lamg.  ze_r, ze_s, ze_g of M:5127-5136.  rhof = sqrt(RHO_NOT/rho).
 *             qs and qg NULL mean zero in any context; cloud water and cloud ice are not read.  Inputs are never written.
 *   D grids   per species (KIDMP_DSPECTRUM_R, _S, _G) a pair D[nb], dD[nb] of bin diameters and widths (m; positive,
 *             finite), 1 <= nb <= KIDMP_DSPECTRUM_MAX_BINS, always binary64.  NULL means the scheme's own 100 bins Dr/dtr,
 *             Ds/dts, Dg/dtg (M:605-657), which every context holds on the device (kidmp_spectra_default_grid).
 *   echo      the reflectivity of diameter bin b, in the units of ze (m6 m-3), the density at D_b times dD_b:
 *               rain     z_b = (N0_r * E(lamr*D_b)) * G_b,                    G_b = D_b**6 * dD_b
 *               graupel  z_b = ((ZE_GRAUPEL_FAC*N0_g) * E(lamg*D_b)) * G_b,    G_b = D_b**6 * dD_b,
 *                        ZE_GRAUPEL_FAC = (0.176/0.93)*(6/PI)**2*(am_g/900)**2 (M:5133-5135)
 *               snow     z_b = (zs * (Kap0*E(x0*D_b) + (k1*D_b**mu_s)*E(x1*D_b))) * G_b,   G_b = D_b**4 * dD_b,
 *                        zs = ze_s*(Mrat**5*ia00), x0 = Mrat*Lam0, x1 = Mrat*Lam1, k1 = Kap1*Mrat**mu_s,
 *                        1/ia00 = Kap0 G(5) Lam0**-5 + Kap1 G(5+mu_s) Lam1**-(5+mu_s): the Field shape at the reflectivity
 *                        moment, normalised by its closed integral and scaled to calc_refl10cm's ze_s, as the Doppler
 *                        moments weight snow
 *             E(x) = exp(-x), and exact +0.0 where x exceeds 700 (kidmp_spectra.h's rule).  On an infinitely fine and
 *             wide D grid the sum of z_b tends to ze_x and its velocity moments to vz_x and v2_x of kidmp_doppler.h.
 *   speed     v = rhof * vfac_b - w with vfac_b = av_x * D_b**bv_x * E(fv_x*D_b) (bv_r = 1; graupel has no exponential),
 *             positive downward; w is the vertical air velocity, positive upward and cell-centred (NULL: 0).  No
 *             vts_boost, no MAX(vtg, vtrk), no above-freezing blend.
 *   v grid    uniform: nv bins of width dv > 0, v0 the centre of bin 0, 1 <= nv <= KIDMP_DSPECTRUM_MAX_NV.  1/dv is formed
 *             once on the host.
 *   deposit   linear (cloud in cell) over nv + 2 slots: below, the bins 0 .. nv-1, above.  p = (v - v0)*(1/dv);
 *             p' = !(p >= -1) ? -1 : (p > nv ? nv : p); j = min(floor(p'), nv-1), clamped again to [-1, nv-1] as an
 *             integer; f = p' - j.  (1-f)*z_b goes to slot j and f*z_b to slot j+1, slot -1 being `below` and slot nv
 *             `above`.  The deposit is continuous in v, conserves the sum of z_b, and for bins inside the grid the sum of
 *             v*z_b.
 *   order     at every level rain's bins ascending, then snow's, then graupel's, into binary64 accumulators that start
 *             at +0.0; one rounding on store for the binary32 entries.
 *   outputs   total, rain, snow, graupel  [ncol][nv][nz], the level fastest (kidmp_spectra.h's bin layout), m6 m-3 per bin
 *             below, above                [ncol][nz]: what `total` holds outside the grid
 *             Each is formed in a pass of its own over the same z_b in the same order: the bits of an output do not depend
 *             on which others were requested, on the batch, on the column's position or on how the kernel tiles the
 *             velocity axis.  An absent species deposits nothing; a level with no species has exact +0.0 everywhere, and
 *             w is not read there.
 *   non-finite  A position that is NaN (a NaN w, state or grid value) lies wholly in `below`; -inf and anything under
 *             -1 likewise; +inf and anything over nv wholly in `above`.  The deposited values are then whatever the
 *             arithmetic gives (NaN or inf included); every index formed stays inside the nv + 2 slots.
 *
 * Turbulent and beam broadening are a one-dimensional convolution along the bin axis, which the caller applies.
 * kidmp_spectrum_process_device (kidmp_specproc.h) applies it on the device, with a noise floor, detection and moments.
 * Not modelled: echoes of cloud ice and cloud droplets, Mie scattering, attenuation, the melting layer, noise floors,
 * non-uniform velocity grids, entries over several devices.
 */
#ifndef KIDMP_DSPECTRUM_H
#define KIDMP_DSPECTRUM_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_DSPECTRUM_NSPECIES 3
#define KIDMP_DSPECTRUM_R 0
#define KIDMP_DSPECTRUM_S 1
#define KIDMP_DSPECTRUM_G 2
#define KIDMP_DSPECTRUM_MAX_BINS 256
#define KIDMP_DSPECTRUM_MAX_NV 256

/* Each member is an array of the shape stated above or NULL (not wanted: no pass, no store).  At least one member must
 * be asked for.  kidmp32_dspectrum_out: binary64 inside, one rounding on store. */
typedef struct kidmp_dspectrum_out { double *total, *rain, *snow, *graupel, *below, *above; } kidmp_dspectrum_out;
typedef struct kidmp32_dspectrum_out { float *total, *rain, *snow, *graupel, *below, *above; } kidmp32_dspectrum_out;
/* The diameter grids by species: D[x] and dD[x] both NULL = the scheme's own grid (nb[x] is not read), or both arrays of
 * nb[x] values.  Device memory for the device entries, host memory for the host entries. */
typedef struct kidmp_dspectrum_grids {
    const double *D[KIDMP_DSPECTRUM_NSPECIES];
    const double *dD[KIDMP_DSPECTRUM_NSPECIES];
    int32_t nb[KIDMP_DSPECTRUM_NSPECIES];
} kidmp_dspectrum_grids;

/* The device entries never allocate, never synchronise and enqueue exactly one launch on `stream`, whatever is requested:
 * they can be captured into a hipGraph.  The host entries take host arrays and run chunks of columns through the
 * context's staging memory on its compute stream, then synchronise; the caller's grids go up once, only what was asked
 * for comes down, the chunks are capped so that the staging stays under 256 MiB, and the results equal the device
 * entry's bit for bit for any chunking (kidmp_set_host_chunk).
 * KIDMP_EINVAL, nothing written: a NULL among t, p, qv, qr, nr; nz outside [2, KIDMP_MAX_NZ]; ncol < 0; nv outside
 * [1, KIDMP_DSPECTRUM_MAX_NV]; dv that is not a finite number above 0 with a finite 1/dv; v0 that is not finite; out NULL or
 * all its members NULL; grids with one of D / dD NULL alone or nb outside [1, KIDMP_DSPECTRUM_MAX_BINS]; a pointer that is
 * not memory of the context's device (device entries).  grids NULL = the scheme's own grid for every species.  A NULL
 * context, or one whose exponents are not those the kernel takes as integers, returns KIDMP_ESTATE; ncol == 0 returns
 * KIDMP_OK. */
int kidmp_doppler_spectrum_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *w, double v0, double dv, int32_t nv,
        const kidmp_dspectrum_grids *grids, const kidmp_dspectrum_out *out, void *stream);
int kidmp32_doppler_spectrum_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *w, double v0, double dv, int32_t nv,
        const kidmp_dspectrum_grids *grids, const kidmp32_dspectrum_out *out, void *stream);
int kidmp_doppler_spectrum_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *w, double v0, double dv, int32_t nv,
        const kidmp_dspectrum_grids *grids, const kidmp_dspectrum_out *out);
int kidmp32_doppler_spectrum_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *w, double v0, double dv, int32_t nv,
        const kidmp_dspectrum_grids *grids, const kidmp32_dspectrum_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_DSPECTRUM_H */
