// thompson_reflectivity.h -- the wave-per-column diagnostics: calc_refl10cm (M:4946-5244), the 10-cm Rayleigh radar
// reflectivity of the scheme's own size distributions, alone or with calc_effectRad (M:4834-4935) of the same levels.
// Kernels: thompson_reflectivity.hip; per-level arithmetic: thompson_levels.h; C ABI: include/kidmp.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "thompson_params.h"
#include "thompson_levels.h"
#include "kidmp_brightband_mix.h"

namespace kidmp {

// Reports whether the context's exponents are the ones the kernel takes as integer powers / roots (see the .hip).
bool refl_consts_supported(const Consts &hc);
ReflConsts refl_consts(const Consts &hc);
RadConsts rad_consts(const Consts &hc, bool aerosol_aware);

// dbz[col*nz+k] for ncol columns of nz (2 <= nz <= KIDMP_MAX_NZ) levels, device pointers; qs and qg may be null (zero).
// T = double, or float (widened on load, computed in binary64, rounded on store).
template <class T>
hipError_t launch_reflectivity(const ReflConsts &c, int64_t ncol, int nz, const T *t, const T *p, const T *qv,
                               const T *qr, const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t stream);

// The state the two diagnostics read and what they return.  Null means: nc -- the context is not aerosol-aware (Nt_c,
// M:4863); qi and ni, qs and qg -- zero (iiwarm); an output -- not wanted.
template <class T> struct ColumnState { const T *t, *p, *qv, *qc, *nc, *qi, *ni, *qr, *nr, *qs, *qg; };
template <class T> struct ColumnOutputs { T *dbz, *re_qc, *re_qi, *re_qs; };

// dbz and the radii (preset where the species is absent, M:1111-1113) from one read of the state: needs out.dbz and
// out.re_qc; out.re_qi and out.re_qs may be null.
template <class T>
hipError_t launch_column_outputs(const ReflConsts &c, const RadConsts &rc, int64_t ncol, int nz, const ColumnState<T> &in,
                                 const ColumnOutputs<T> &out, hipStream_t stream, const double *set_nc_col = nullptr);
// set_nc_col: null, or [ncol] set_Nc in cm**-3 (kidmp_set_column_nc): the column's own Nt_c = set_nc_col[col]*1.e6 for re_qc

// The per-column summary (include/kidmp_summary.h): SUMMARY_N doubles per column from one read of its profiles.  Null
// means: nc -- the context is not aerosol-aware; qi, qs and qg -- zero (iiwarm); set_nc_col -- the context's Nt_c.
// dz: element (col, k) = dz[col*dz_col_stride + k], dz_col_stride 0 = one profile for all columns.
constexpr int SUMMARY_N = 16;
template <class T> struct SummaryArgs {
    const T *t, *p, *qv, *qc, *nc, *qi, *qr, *nr, *qs, *qg, *dz;
    int64_t dz_col_stride;
    double dbz_echo, q_cloud, t_freeze;
    const double *set_nc_col;
};
template <class T>
hipError_t launch_column_summary(const ReflConsts &c, const RadConsts &rc, int64_t ncol, int nz, const SummaryArgs<T> &a,
                                 double *summary, hipStream_t stream);

// The fall speeds of block O (M:3206-3354) as a diagnostic of a state (include/kidmp_fall.h).  Null means: qi, ni, qs, qg
// -- not read (warm); boost -- 1.0 where T < T_0, 1.5 elsewhere; an output -- not wanted; nstep -- not wanted, and then
// dz and dt are not read.  out: vt_r, vt_nr, vt_i, vt_ni, vt_s, vt_g, flux_r, flux_i, flux_s, flux_g, flux_total.
constexpr int FALL_NOUT = 11;
template <class T> struct FallArgs {
    const T *t, *p, *qv, *qr, *nr, *qi, *ni, *qs, *qg, *boost, *dz;
    int64_t dz_col_stride;
    double dt;
    T *out[FALL_NOUT];
    int32_t *nstep;                                  // [ncol][4]: rain, ice, snow, graupel
    int warm;                                        // iiwarm: the frozen speeds and fluxes are +0.0 (M:3346-3352)
};
bool fall_consts_supported(const Consts &hc);
// d_consts: the context's Consts in device memory (kidmp_ctx::d_consts)
template <class T>
hipError_t launch_fall_speeds(const Consts *d_consts, int64_t ncol, int nz, const FallArgs<T> &a, hipStream_t stream);


// The size spectra (include/kidmp_spectra.h): each species' distribution parameters [ncol][nz] and its numbers per bin
// [ncol][nb][nz].  Species in the order c, i, r, s, g; par in the order of kidmp_spectra_out.  Null means: nc -- Nt_c (the
// context is not aerosol-aware); qi and ni, qs, qg -- the species is absent everywhere (iiwarm); an output -- not wanted;
// set_nc_col -- the context's Nt_c.  D, dD: device arrays of nb[x] doubles, read only where spec[x] is wanted.
constexpr int SPECTRA_NPAR = 11, SPECTRA_NSPEC = 5;
constexpr int SPECTRA_LAM_C = 0, SPECTRA_LAM_I = 3, SPECTRA_LAM_R = 5, SPECTRA_SMOB = 7, SPECTRA_LAM_G = 9;   // each followed by its n0 / smoc (and nu_c)
constexpr int SPECTRA_MAX_SHARES = 16, SPECTRA_MIN_BLOCKS = 1024;
template <class T> struct SpectraArgs {
    const T *t, *p, *qv, *qc, *nc, *qi, *ni, *qr, *nr, *qs, *qg;
    T *par[SPECTRA_NPAR];
    T *spec[SPECTRA_NSPEC];
    const double *D[SPECTRA_NSPEC], *dD[SPECTRA_NSPEC];
    int32_t nb[SPECTRA_NSPEC];
    const double *set_nc_col;                        // null, or the batch's share of a bound per-column droplet number (cm**-3)
    int aero;                                        // the context's is_aerosol_aware: nc is read and size-limited (M:1398-1409)
};
bool spectra_consts_supported(const Consts &hc);
template <class T>
hipError_t launch_size_spectra(const Consts *d_consts, int64_t ncol, int nz, const SpectraArgs<T> &a, hipStream_t stream);

// The lidar operator (include/kidmp_lidar.h): extinction, backscatter, optical depth and attenuated backscatter of every
// level, and eight numbers per column, from the size spectra's load.  Null means: nc -- Nt_c (the context is not
// aerosol-aware); qi and ni, qs, qg -- the species is absent everywhere (iiwarm); an output or the summary -- not wanted;
// dz -- not read when nothing past out[LIDAR_NLOCAL - 1] and no summary is wanted.  out in the order of kidmp_lidar_out.
constexpr int LIDAR_NOUT = 14, LIDAR_NLOCAL = 8, LIDAR_SUMMARY_N = 8;      // out[0..7] need no neighbour: no scan
constexpr int LIDAR_TAU_UP = 8, LIDAR_TAU_DN = 9, LIDAR_ATT_UP = 10, LIDAR_ATT_DN = 11, LIDAR_SR_UP = 12, LIDAR_SR_DN = 13;
template <class T> struct LidarArgs {
    const T *t, *p, *qv, *qc, *nc, *qi, *ni, *qr, *nr, *qs, *qg, *dz;
    int64_t dz_col_stride;
    T *out[LIDAR_NOUT];
    double *summary;                                 // [ncol][LIDAR_SUMMARY_N]
    double s_ratio[SPECTRA_NSPEC], eta, c_mol, beta_detect, trans_lost;
    const double *set_nc_col;
    int aero;
};
// beyond spectra_consts_supported: bm_s = 2 (snow's extinction is its moment smob) and mu_r = mu_g = mu_i = 0
bool lidar_consts_supported(const Consts &hc);
template <class T>
hipError_t launch_lidar_profiles(const Consts *d_consts, int64_t ncol, int nz, const LidarArgs<T> &a, hipStream_t stream);

// The Doppler moments of a vertically pointing radar (include/kidmp_doppler.h): reflectivity, mean Doppler velocity and
// spectrum width of every level, from calc_refl10cm's load and size distributions.  Null means: qs, qg -- zero; w -- zero;
// an output -- not wanted.  out: dbz, vd, sw, vz_r, vz_s, vz_g, dbz_r, dbz_s, dbz_g.
constexpr int DOPPLER_NOUT = 9;
template <class T> struct DopplerArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg, *w;
    T *out[DOPPLER_NOUT];
};
// the exponents lvl:: takes as integer powers beyond those of refl_consts_supported
bool doppler_consts_supported(const Consts &hc);
DopplerConsts doppler_consts(const Consts &hc);
template <class T>
hipError_t launch_doppler_moments(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const DopplerArgs<T> &a,
                                  hipStream_t stream);

// The Doppler spectrum (include/kidmp_dspectrum.h): the reflectivity of every level on a uniform velocity grid, from
// k_doppler_moments' load.  Null means: qs, qg -- zero; w -- zero; an output -- not wanted.  out: total, rain, snow,
// graupel [ncol][nv][nz], below, above [ncol][nz].  D, dD: device arrays of nb[x] doubles by species rain, snow, graupel.
// idv = 1/dv.  One launch; the velocity axis is walked in tiles of DSPECTRUM_TILE slots held in LDS.
// (-DKIDMP_DSPECTRUM_TILE=n builds another tile for tools/bench_doppler_spectrum.py --lib; the results do not depend on it)
#ifndef KIDMP_DSPECTRUM_TILE
#define KIDMP_DSPECTRUM_TILE 24
#endif
constexpr int DSPECTRUM_NOUT = 6, DSPECTRUM_NSPEC = 3, DSPECTRUM_TILE = KIDMP_DSPECTRUM_TILE, DSPECTRUM_MAX_NV = 256;
static_assert(DSPECTRUM_TILE >= 2 && DSPECTRUM_TILE <= 30, "four waves' tiles and the fastmath tables share 64 KiB of LDS");
template <class T> struct DSpectrumArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg, *w;
    T *out[DSPECTRUM_NOUT];
    const double *D[DSPECTRUM_NSPEC], *dD[DSPECTRUM_NSPEC];
    int32_t nb[DSPECTRUM_NSPEC];
    double v0, idv;
    int32_t nv;
};
template <class T>
hipError_t launch_doppler_spectrum(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const DSpectrumArgs<T> &a,
                                   hipStream_t stream);

// The bright band (include/kidmp_brightband.h): calc_refl10cm with melting snow and graupel below the melting level, from
// k_doppler_moments' load.  Null means: qs, qg -- zero; an output -- not wanted.  out: dbz, dbz_s, dbz_g, enh_s, enh_g,
// fmelt_s, fmelt_g [ncol][nz]; k0 [ncol].  D, dD: device arrays of nb[x] doubles by species snow, graupel.  warm: an iiwarm
// context, no melting level.  One launch; the lanes sweep the diameter bins of each active (level, species) pair.
constexpr int BRIGHTBAND_NOUT = 7, BRIGHTBAND_NSPEC = 2, BRIGHTBAND_MAX_BINS = 256;
template <class T> struct BrightBandArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg;
    T *out[BRIGHTBAND_NOUT];
    int32_t *k0;
    const double *D[BRIGHTBAND_NSPEC], *dD[BRIGHTBAND_NSPEC];
    int32_t nb[BRIGHTBAND_NSPEC];
    BBMix mix;
    int warm;
};
template <class T>
hipError_t launch_bright_band(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const BrightBandArgs<T> &a,
                              hipStream_t stream);

// The cloud radar (include/kidmp_mie.h): Mie reflectivity, extinction, path-integrated attenuation and mean Doppler
// velocity from k_doppler_moments' load and a table of five rows per diameter bin.  Null means: qc, qs, qg, w, k_gas --
// zero; an output -- not wanted; dz -- not read when no path integral is wanted.  out in the order of kidmp_mie_out,
// pia_total [ncol].  D, dD: device arrays of nb[x] doubles by species rain, snow, graupel; rows[x]: [MIE_NROWS][nb[x]]
// (s_mie, s_ray, s_ext, mass, v0).  kc: (6 pi/lambda) Im(K(eps_w)); rho_w: the configuration's.  Cloud water enters through
// its mass alone, where qc > R1.  One launch; lanes over levels, a loop over the bins.
constexpr int MIE_NOUT = 13, MIE_NSPEC = 3, MIE_MAX_BINS = 256, MIE_NROWS = 5;
constexpr int MIE_DBZ = 0, MIE_DBZ_UP = 1, MIE_DBZ_DOWN = 2, MIE_DBZ_X = 3, MIE_MIE_X = 6, MIE_EXT = 9, MIE_PIA_UP = 10, MIE_PIA_DOWN = 11, MIE_VD = 12;
template <class T> struct MieArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *w, *k_gas;
    int64_t dz_col_stride, k_gas_col_stride;
    T *out[MIE_NOUT];
    T *pia_total;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC], *rows[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    double kc, rho_w;
};
template <class T>
hipError_t launch_mie_radar(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const MieArgs<T> &a,
                            hipStream_t stream);

// The microwave radiometer (include/kidmp_radiometer.h): absorption and back-hemisphere scattering coefficients from
// k_mie_radar's load and a table of three rows per diameter bin (s_abs, s_bsc, mass), the two-stream layer of every level
// and the adding of the layers by two wave scans.  Null means: qc, qs, qg, k_gas -- zero; t_sfc -- the column's t at level
// 0; an output -- not wanted; dz -- not read when only k_abs and k_bsc are wanted.  out: k_abs, k_bsc, refl, trans, tb_up,
// tb_down [ncol][nz]; tb_toa, tb_ground, tau_abs [ncol].  One launch; lanes over levels, a loop over the bins.
constexpr int RAD_NOUT = 6, RAD_NROWS = 3;
constexpr int RAD_K_ABS = 0, RAD_K_BSC = 1, RAD_REFL = 2, RAD_TRANS = 3, RAD_TB_UP = 4, RAD_TB_DOWN = 5;
template <class T> struct RadiometerArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *k_gas, *t_sfc;
    int64_t dz_col_stride, k_gas_col_stride;
    T *out[RAD_NOUT];
    T *tb_toa, *tb_ground, *tau_abs;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC], *rows[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    double kc, rho_w, mu, emissivity, t_cosmic;
};
template <class T>
hipError_t launch_radiometer(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const RadiometerArgs<T> &a,
                             hipStream_t stream);

// Several channels of the radiometer or of the cloud radar in one launch (include/kidmp_multichannel.h): the load and the
// densities of the bin loop are formed once and shared by the channels, which are taken in tiles of
// multichannel_tile(which, nz) inside the launch.  The state, dz, w and t_sfc are the single-channel kernels'; everything
// else is per channel c < nch: rows[c][x] the species' rows of the channel's table (all tables on the grids D, dD, nb, the
// rows that do not depend on the wavelength equal bit for bit), kc, rho_w and the radiometer's closure, k_gas at
// k_gas + c*k_gas_ch_stride, and the slab of every output: a profile at out + c*prof_ch_stride, a per-column one at
// + c*col_ch_stride.  Slab c holds the bits the single-channel kernel writes with channel c's table.
constexpr int MC_MAX_CHANNELS = 16;
template <class T> struct RadiometerMultiArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *k_gas, *t_sfc;
    int64_t dz_col_stride, k_gas_col_stride, k_gas_ch_stride, prof_ch_stride, col_ch_stride;
    T *out[RAD_NOUT];
    T *tb_toa, *tb_ground, *tau_abs;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    int32_t nch;
    const double *rows[MC_MAX_CHANNELS][MIE_NSPEC];
    double kc[MC_MAX_CHANNELS], rho_w[MC_MAX_CHANNELS], mu[MC_MAX_CHANNELS], emissivity[MC_MAX_CHANNELS], t_cosmic[MC_MAX_CHANNELS];
};
template <class T> struct MieMultiArgs {
    const T *t, *p, *qv, *qc, *qr, *nr, *qs, *qg, *dz, *w, *k_gas;
    int64_t dz_col_stride, k_gas_col_stride, k_gas_ch_stride, prof_ch_stride, col_ch_stride;
    T *out[MIE_NOUT];
    T *pia_total;
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    int32_t nch;
    const double *rows[MC_MAX_CHANNELS][MIE_NSPEC];
    double kc[MC_MAX_CHANNELS], rho_w[MC_MAX_CHANNELS];
};
// how many channels one pass of the kernel carries at nz levels; which: 0 the radiometer, 1 the radar
int multichannel_tile(int which, int nz);
template <class T>
hipError_t launch_radiometer_multi(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const RadiometerMultiArgs<T> &a,
                                   hipStream_t stream);
template <class T>
hipError_t launch_mie_radar_multi(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const MieMultiArgs<T> &a,
                                  hipStream_t stream);

// The polarimetric radar (include/kidmp_polarimetric.h): Z_DR, K_DP and rho_hv of oblate spheroids from k_mie_radar's load
// and a table of seven rows per diameter bin (s_h, s_v, c_re, c_im, s_0, k, mass).  Null means: qs, qg -- zero; an output
// -- not wanted.  out in the order of kidmp_pol_out.  uniform[x] != 0: the species walks no bins and takes scal[x] (s_h/s_0,
// s_v/s_0, c_re/s_0, c_im/s_0, k/mass) in place of the ratios of its sums; its D, dD, rows and nb are not read.
// kfac: 90e3 pi/lambda.  One launch; lanes over levels, a loop over the bins.
constexpr int POL_NOUT = 13, POL_NROWS = 7, POL_NSCAL = 5;
constexpr int POL_DBZ_H = 0, POL_ZDR = 1, POL_KDP = 2, POL_RHOHV = 3, POL_DBZ_H_X = 4, POL_ZDR_X = 7, POL_KDP_X = 10;
template <class T> struct PolArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg;
    T *out[POL_NOUT];
    const double *D[MIE_NSPEC], *dD[MIE_NSPEC], *rows[MIE_NSPEC];
    int32_t nb[MIE_NSPEC];
    int32_t uniform[MIE_NSPEC];
    double scal[MIE_NSPEC][POL_NSCAL];
    double kfac;
};
template <class T>
hipError_t launch_polarimetric(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const PolArgs<T> &a,
                               hipStream_t stream);

}  // namespace kidmp
