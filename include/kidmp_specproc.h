/*
 * kidmp_specproc.h -- Doppler-spectrum processing on the device: turbulent and beam broadening, a noise floor, detection
 * and the moments of what is detected, in one launch of kidmp::k_spectrum_process.
 *
 * kidmp_doppler_spectrum_device gives the quiet-air spectrum of a vertically pointing radar and leaves the broadening
 * and the noise floor to the caller; kidmp_doppler_moments_device gives moments without either.  This is the operator over
 * [ncol][nv][nz] spectra that closes the chain: it serves the spectra of kidmp_dspectrum.h and any later spectrum on a
 * uniform velocity grid.  THE DEFINITIONS BELOW ARE THE PROJECT'S OWN (nothing in the reference this library was written
 * against corresponds to them): parity with an instrument simulator is unpinned.  Conventions as in kidmp.h and
 * kidmp_dspectrum.h (return codes, device binding, [ncol][nz] arrays with k fastest, k = 0 the lowest level, spectra
 * [ncol][nv][nz] with the level fastest).
 *
 * INPUTS, device memory, never written:
 *   spec    [ncol][nv][nz]  required: a spectrum, m6 m-3 per bin (kidmp_dspectrum_out.total or any of its species)
 *   v0, dv, nv              the velocity grid with kidmp_dspectrum.h's rules: nv bins of width dv > 0, v0 the centre of
 *                           bin 0, 1 <= nv <= KIDMP_SPECPROC_MAX_NV.  1/dv is formed once on the host.
 *   sigma   the standard deviation of the broadening in m/s; NULL = none.  sigma_stride = 0: [nz], shared by the columns;
 *           sigma_stride = nz: [ncol][nz] (the convention of w in kidmp_kid_advect_device)
 *   noise   the mean noise per velocity bin in the units of spec; NULL = 0; noise_stride as sigma_stride
 *   cfg     cut (the window reaches cut standard deviations; finite, above 0; default 4), snr_min (finite, not below 0;
 *           default 1), add_noise (default 0)
 *
 * In binary64, every operation rounded once, no contraction, IEEE division and square root, per column and level k
 * (the window arithmetic is kid_amd/csrc/kidmp_specproc_window.h, shared by host and device):
 *
 *   window    s = sigma_k*(1/dv).  !(sigma_k > 0) -- NaN, zero, negative -- gives H = 0.  Otherwise h = ceil(cut*s) and
 *             H = h > 256 ? 256 : (int)h  (KIDMP_SPECPROC_MAX_HALF = 256).
 *   weights   for d = 1 .. H: r = d/s; t = 0.5*(r*r); g_d = E(-t), E fastmath.h's exp (table-driven, within 2 ulp, the
 *             same bits on host and device) for t <= 700 and exact +0.0 beyond; g_0 = 1 without an exponential.
 *             G = g_0 + sum_{d = 1 .. H} (g_d + g_d), d ascending.
 *   signal    B_j = (sum_i g_|j-i| * in[i]) / G, i ascending over max(0, j-H) .. min(nv-1, j+H), the sum starting at
 *             +0.0, each product rounded before it is added.  With H = 0 B_j is the bits of in[j]: no exponential is
 *             formed and no division made.
 *   leaving   T_m = sum_{d = m .. H} g_d, summed from d = H down to m.
 *             lost_below = (sum_{i = 0 .. min(H, nv)-1} in[i]*T_{i+1}) / G, i ascending, starting at +0.0
 *             lost_above = (sum_{i = max(0, nv-H) .. nv-1} in[i]*T_{nv-i}) / G, i ascending, starting at +0.0
 *             Both [ncol][nz]; exact +0.0 with H = 0.  sum_j B_j + lost_below + lost_above = sum_i in[i] up to rounding.
 *   detect    bin j is detected iff B_j > snr_min*n_k (one product per level); without noise that is B_j > 0.
 *   moments   over the detected bins, j ascending, v_j = v0 + j*dv (a product, then a sum), sums starting at +0.0:
 *               z = sum B_j;   dbz = 10*log10(max(z, 1e-22)*1e18), log10 fastmath.h's
 *               vm = (sum v_j*B_j)/z, then held to [v_lo, v_hi]: v_lo where the quotient is below it, v_hi where above (the
 *                    quotient of two rounded sums can leave the range of its terms by an ulp; a NaN passes)
 *               with e_j = v_j - vm and q_j = e_j*e_j:  c2 = sum q_j*B_j;  c3 = sum (q_j*e_j)*B_j;  c4 = sum (q_j*q_j)*B_j
 *               sw = sqrt(c2/z) where c2/z > 0, else +0.0
 *               skew = (c3/z)/((sw*sw)*sw);   kurt = (c4/z)/((sw*sw)*(sw*sw));   both exact +0.0 where sw == 0
 *               v_lo, v_hi the centres of the first and the last detected bin; nbins (int32) the number of detected bins
 *             With no detected bin every moment is exact +0.0, nbins 0 and dbz -40.
 *   outputs   spec [ncol][nv][nz]: B_j, or B_j + n_k with add_noise != 0; the others [ncol][nz].  The kidmp32_ entry
 *             takes binary32 spec, sigma and noise, widens on load, computes as above and rounds once on store.
 *
 * The bits of an output do not depend on which other outputs were requested, on the batch, on the column's position, on
 * a repeated call or on how the kernel tiles the velocity axis.  Every gather index is range-checked by construction: a
 * bin index is formed only inside 0 .. nv-1, a weight index only inside 0 .. H, H only inside 0 .. 256.  A NaN or infinite
 * sigma, noise or spectrum value is memory-safe and gives whatever the arithmetic above gives.
 *
 * Not modelled: random noise realisations (there is no random number generator: `noise` is the mean floor), spectral
 * averaging, the separation of several peaks, aliasing or folding at the Nyquist velocity, non-uniform velocity grids.
 *
 * There are no host-array entries and no Fortran binding, as for kidmp_scan.h and kidmp_slab.h: the input is a device
 * product, sixteen bytes per bin and level that no caller wants to carry over PCIe twice.
 */
#ifndef KIDMP_SPECPROC_H
#define KIDMP_SPECPROC_H

#include "kidmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KIDMP_SPECPROC_MAX_NV 256
#define KIDMP_SPECPROC_MAX_HALF 256

typedef struct kidmp_specproc_cfg {
    double cut;
    double snr_min;
    int32_t add_noise;
} kidmp_specproc_cfg;

/* spec is [ncol][nv][nz], nbins [ncol][nz] int32, every other member [ncol][nz]; NULL = not wanted: no store and, where
 * possible, no work (a request for moments alone stores no spectrum; one without sw, skew and kurt walks the spectrum
 * once, not twice).  At least one must be asked for. */
typedef struct kidmp_specproc_out { double *spec, *lost_below, *lost_above, *dbz, *vm, *sw, *skew, *kurt, *v_lo, *v_hi; int32_t *nbins; } kidmp_specproc_out;
typedef struct kidmp32_specproc_out { float *spec, *lost_below, *lost_above, *dbz, *vm, *sw, *skew, *kurt, *v_lo, *v_hi; int32_t *nbins; } kidmp32_specproc_out;

/* The entries never allocate, never synchronise and enqueue exactly one launch on `stream`: they can be captured into a
 * hipGraph.  Outputs must not overlap inputs or one another (stated, not checked).
 * KIDMP_EINVAL, nothing written: a NULL spec, cfg or out; nz outside [2, KIDMP_MAX_NZ]; ncol < 0 or more (column, level
 * group) pairs than one launch takes (ncol*ceil(nz/64) > 0x7fffffff); nv outside [1, KIDMP_SPECPROC_MAX_NV]; dv that is
 * not a finite number above 0 with a finite 1/dv; v0 that is not finite; cut that is not finite and above 0; snr_min that
 * is not finite and at least 0; sigma_stride or noise_stride other than 0 or nz; every member of out NULL; a pointer that
 * is not memory of the context's device.  A NULL context returns KIDMP_ESTATE; ncol == 0 returns KIDMP_OK. */
int kidmp_spectrum_process_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *spec, double v0, double dv, int32_t nv,
        const double *sigma, int32_t sigma_stride, const double *noise, int32_t noise_stride,
        const kidmp_specproc_cfg *cfg, const kidmp_specproc_out *out, void *stream);
int kidmp32_spectrum_process_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *spec, double v0, double dv, int32_t nv,
        const float *sigma, int32_t sigma_stride, const float *noise, int32_t noise_stride,
        const kidmp_specproc_cfg *cfg, const kidmp32_specproc_out *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KIDMP_SPECPROC_H */
