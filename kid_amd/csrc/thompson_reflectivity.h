// thompson_reflectivity.h -- calc_refl10cm (M:4946-5244): 10-cm Rayleigh radar reflectivity of the scheme's own size
// distributions, one wavefront per column.  Kernel: thompson_reflectivity.hip; C ABI: include/kidmp.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "thompson_params.h"

namespace kidmp {

// the values of thompson_init (M:442-602) the live part of calc_refl10cm reads, taken from the context's Consts
struct ReflConsts {
    double crg3, crg4, org2;           // rain: crg(3), crg(4), org2   (obmr = 1/3: cube root; cre(2) = 1, cre(4) = 7)
    double cse3, oams, sa[10], sb[10]; // snow: the Field et al. fit at the bm_s*2 moment (cse(3)); bm_s = 2: smo2 = smob
    double cgg1, cgg2, cgg4, lamg_fac; // graupel: cgg(1), cgg(2), cgg(4), (cgg(3)*ogg2*ogg1)**obmg   (oge1 = 1/4;
                                       //          cge(2) = 1, cge(4) = 7)
};

// Reports whether the context's exponents are the ones the kernel takes as integer powers / roots (see the .hip).
bool refl_consts_supported(const Consts &hc);
ReflConsts refl_consts(const Consts &hc);

// dbz[col*nz+k] for ncol columns of nz (2 <= nz <= KIDMP_MAX_NZ) levels, device pointers; qs and qg may be null (zero).
// T = double, or float (widened on load, computed in binary64, rounded on store).
template <class T>
hipError_t launch_reflectivity(const ReflConsts &c, int64_t ncol, int nz, const T *t, const T *p, const T *qv,
                               const T *qr, const T *nr, const T *qs, const T *qg, T *dbz, hipStream_t stream);

}  // namespace kidmp
