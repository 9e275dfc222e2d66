// kidmp_face.h -- internal to kidmp_kinematic.hip and kidmp_slab.hip (not installed): the value of a field at an interior
// face, one __device__ function template with an instantiation per advection scheme of include/kidmp_advection.h.  Both
// kernels call it for their z faces and the slab kernel for its x faces too, so the z part of the slab stays the 1-D
// kernel's operation for operation.
// Built with the library's plain flags (IEEE division, no contraction): every operation below rounds once.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/kidmp_advection.h"

namespace kidmp {
namespace face {
// What the members of a face share is formed once per face and column from its Courant number c and kept in registers:
// hc = 0.5*(1.0 - c) for both schemes; ULTIMATE adds g = (1.0 - c*c)/6.0 and rc = 1.0/c (c == +0.0: +inf).  A kernel
// holds hc[NJ] and g, rc[coef_count<S>(NJ)]: van Leer leaves the one element of g and rc untouched, and it is gone.
template <int S> constexpr int coef_count(int nj) { return S == KIDMP_ADVECT_ULTIMATE ? nj : 1; }
template <int S> __device__ __forceinline__ void coef(double c, double &hc, double &g, double &rc)
{
    hc = 0.5 * (1.0 - c);
    if constexpr (S == KIDMP_ADVECT_ULTIMATE) {
        g = (1.0 - c * c) / 6.0;
        rc = 1.0 / c;
    }
}

// x with its sign bit XORed by that of m (0 or 0x80000000): x or -x, exactly
__device__ __forceinline__ double flip(double x, unsigned int m)
{
    return __longlong_as_double(__double_as_longlong(x) ^ (static_cast<long long>(m) << 32));
}

// qu, qd, quu: the upwind, downwind and second upwind cell; second: quu exists (always, in x)
template <int S> __device__ __forceinline__ double value(double hc, double g, double rc, bool second, double qu, double qd, double quu)
{
    const double dq = qd - qu, b = qu - quu, bd = b * dq;
    if constexpr (S == KIDMP_ADVECT_ULTIMATE) {
        // Leonard's universal limiter on the QUICKEST face value (uniform-grid weights).  Where the three cells are
        // monotonic b != 0, so ref is +-inf at c == 0 and never NaN.  The selects are comparisons, not fmin / fmax:
        // signed zeros are fixed.  The falling case (dq < 0: t = qq < qu ? qq : qu, h = ref > qd ? ref : qd, t > h ? t : h)
        // is the rising one on the negated values, and a negation is exact, so both run as the rising case on values
        // whose sign bit is flipped by that of dq (bd > 0 leaves dq neither zero nor NaN) and flipped back: the same
        // bits as two sets of selects, without the wave-mask arithmetic that choosing between comparisons costs.
        const double curv = dq - b;
        const double qq = (qu + hc * dq) - g * curv;
        const double ref = quu + b * rc;
        const unsigned int m = static_cast<unsigned int>(__double_as_longlong(dq) >> 32) & 0x80000000u;
        const double fqq = flip(qq, m), fqu = flip(qu, m), fref = flip(ref, m), fqd = flip(qd, m);
        const double t = fqq > fqu ? fqq : fqu;
        const double h = fref < fqd ? fref : fqd;
        const double lim = flip(t < h ? t : h, m);
        return second && bd > 0. ? lim : qu;                        // else first-order upwind
    } else {
        // van Leer, harmonic form: no ratio, no NaN
        const double s = second && bd > 0. ? (2.0 * bd) / (b + dq) : 0.;
        return qu + hc * s;
    }
}
}  // namespace face
}  // namespace kidmp
