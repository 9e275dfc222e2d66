// thompson_reflectivity.h -- calc_refl10cm (M:4946-5244), the 10-cm Rayleigh radar reflectivity of the scheme's own size
// distributions, alone or with calc_effectRad (M:4834-4935) of the same levels, and the constants the radar operators that
// share its load pick from the context.  Kernels: thompson_reflectivity.hip; what they share with the other wave-per-column
// kernels: kidmp_column.h; per-level arithmetic: thompson_levels.h; C ABI: include/kidmp.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "thompson_params.h"
#include "thompson_levels.h"

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

// What the Doppler moments add to ReflConsts, read by every operator built on calc_refl10cm's load (kidmp_doppler.hip and the
// radar, radiometer and polarimetric units); supported: the exponents lvl:: takes as integer powers beyond those of
// refl_consts_supported.
bool doppler_consts_supported(const Consts &hc);
DopplerConsts doppler_consts(const Consts &hc);

}  // namespace kidmp
