/*
 * kidmp_doppler.h -- the Doppler moments of a vertically pointing radar on the device.
 *
 * A kinematic column is observed by a vertically pointing cloud radar, which measures three moments per range gate:
 * reflectivity, mean Doppler velocity and spectrum width.  kidmp_reflectivity_device gives the first;
 * kidmp_doppler_moments_device forms all three in one launch, from the size distributions and the fall-speed laws the
 * scheme itself states.  Conventions as in kidmp.h (return codes, device binding, [ncol][nz] arrays with k fastest,
 * k = 0 the lowest level).  In binary64:
 *
 *   load      exactly that of calc_refl10cm (M:4991-5028): rho from qv' = max(1e-10, qv); rain where qr > R1 with
 *             nr = max(R2, nr1*rho) and the unclamped slope lamr of M:5001 (no size limiting: this is not block O's
 *             load); snow where qs > R2, smob = rs*oams, smoc the Field fit at cse(1); graupel where qg > R2, its
 *             intercept the running minimum from the top down over all levels (M:5086-5103).  qs and qg NULL mean
 *             zero in any context; cloud water and cloud ice are not read.  The input arrays are never written.
 *   ze        ze_r, ze_s, ze_g of M:5127-5136; 1e-22 where the species is absent.
 *   speeds    v_x(D) = rhof av_x D**bv_x exp(-fv_x D), rhof = sqrt(RHO_NOT/rho); backscatter ~ D**6 (rain, graupel) and
 *             D**(2 bm_s) (snow).  vz_x = <v sigma>/<sigma> and v2_x = <v**2 sigma>/<sigma> over the species' size
 *             distribution, in closed form:
 *               rain     n = 7+mu_r: vz = rhof av_r G(n+bv_r)/G(n) lamr**n/(lamr+fv_r)**(n+bv_r),
 *                        v2 = (rhof av_r)**2 G(n+2bv_r)/G(n) lamr**n/(lamr+2fv_r)**(n+2bv_r)
 *               graupel  n = 7+mu_g: vz = rhof av_g G(n+bv_g)/G(n) ilamg**bv_g, v2 likewise with 2 bv_g; no
 *                        MAX(vtg, vtrk) above T_0, which is a device of the sedimentation
 *               snow     Mrat = smob/smoc, n = 2 bm_s + 1, A(b,f) = Kap0 G(n+b) (Mrat Lam0 + f)**-(n+b)
 *                        + Kap1 Mrat**mu_s G(n+mu_s+b) (Mrat Lam1 + f)**-(n+mu_s+b):
 *                        vz = rhof av_s A(bv_s,fv_s)/A(0,0), v2 = (rhof av_s)**2 A(2bv_s,2fv_s)/A(0,0); no vts_boost
 *                        and no above-freezing blend
 *   outputs   dbz      the bits of kidmp_reflectivity_device on the same inputs
 *             dbz_x    10 log10(ze_x 1e18); an absent species gives -40
 *             vz_x     m s-1, positive downward; exact +0.0 where the species is absent (no inheritance from above)
 *             vd       V - w, with W = ze_r + ze_s + ze_g over the present species only, in that order,
 *                      V = (ze_r vz_r + ze_s vz_s + ze_g vz_g)/W, and w the vertical air velocity, positive upward
 *                      (NULL: 0)
 *             sw       sqrt(max(0, m2 - V**2)), m2 = (ze_r v2_r + ze_s v2_s + ze_g v2_g)/W; w does not enter
 *             A level with no species at all has vd = sw = +0.0: w is NOT applied there (there is no echo to move).
 *
 * Not modelled: echoes of cloud ice and cloud droplets, Mie scattering and attenuation, the melting layer's wet
 * particles, turbulent and beam broadening of sw, full spectra (kidmp_spectrum_process_device of kidmp_specproc.h
 * broadens a spectrum of kidmp_dspectrum.h and takes its moments, noise floor included).  A column gives the same bits alone, at any position
 * in any batch and on a repeated call.  Inputs are assumed finite and physical; a NaN input is memory-safe and gives
 * unspecified values.
 */
#ifndef KIDMP_DOPPLER_H
#define KIDMP_DOPPLER_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Each member is [ncol][nz] or NULL (not wanted: it costs no store).  At least one member must be asked for.
 * kidmp32_doppler_out: binary64 inside, one rounding on store. */
typedef struct kidmp_doppler_out { double *dbz, *vd, *sw, *vz_r, *vz_s, *vz_g, *dbz_r, *dbz_s, *dbz_g; } kidmp_doppler_out;
typedef struct kidmp32_doppler_out { float *dbz, *vd, *sw, *vz_r, *vz_s, *vz_g, *dbz_r, *dbz_s, *dbz_g; } kidmp32_doppler_out;

/* The device entries never allocate, never synchronise and enqueue one launch on `stream`: they can be captured into a
 * hipGraph.  The host entries take host arrays and run chunks of columns through the context's staging memory on its
 * compute stream, then synchronise; beyond the seven inputs only w (if given) and the requested profiles cross PCIe,
 * and the results equal the device entry's bit for bit for any chunking (kidmp_set_host_chunk).
 * KIDMP_EINVAL, nothing written: a NULL among t, p, qv, qr, nr; nz outside [2, KIDMP_MAX_NZ]; ncol < 0; out NULL or all
 * its members NULL; a pointer that is not memory of the context's device (device entries).  A NULL context returns
 * KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_doppler_moments_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *w, const kidmp_doppler_out *out, void *stream);
int kidmp32_doppler_moments_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *w, const kidmp32_doppler_out *out, void *stream);
int kidmp_doppler_moments_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const double *t, const double *p, const double *qv, const double *qr, const double *nr,
        const double *qs, const double *qg, const double *w, const kidmp_doppler_out *out);
int kidmp32_doppler_moments_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz,
        const float *t, const float *p, const float *qv, const float *qr, const float *nr,
        const float *qs, const float *qg, const float *w, const kidmp32_doppler_out *out);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_DOPPLER_H */
