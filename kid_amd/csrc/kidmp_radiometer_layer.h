// kidmp_radiometer_layer.h -- the two-stream layer and the adding of layers of include/kidmp_radiometer.h.  Plain C++ for
// host and device alike, with nothing of HIP in it, so that the functions the kernel calls are the functions a host
// program can test (tests/native/radiometer_check.cpp).  Binary64, every operation written out and rounded once: build
// without contraction.  Of libm only a correctly rounded sqrt: the caller hands in e = exp(-y) and f = 1 - e.
//
// The layer is the hemispheric-constant two-stream of Meador & Weaver (1980) with the stream cosine mu as a parameter,
// isothermal, in Rayleigh-Jeans brightness temperatures.  ta = k_abs*dz, b = k_bsc*dz, x = sqrt(ta (ta + 2b)), y = x/mu:
//   ta <= 0, b <= 0    R = 0, T = 1, a = 0
//   ta <= 0 <  b       c = b/mu;  R = c/(1 + c), T = 1/(1 + c), a = 0        (conservative scattering)
//   otherwise          S = (ta + b) + x;  G = b/S;  H = (ta + x)/S  (= 1 - G);  p = H + G f;  q = 1 + G e
//                      R = (G f (1 + e))/(p q);  T = (H (1 + G) e)/(p q);  a = (H f)/q  (= 1 - R - T, never negative)
// A layer's state is (Rt, Rb, T, Eu, Ed) = (R, R, T, a t, a t): reflection seen from above and from below, transmission,
// emission upwards and downwards.  combine(lower A, upper B) adds two stacks; it is associative, not commutative, and
// (0, 0, 1, 0, 0) is its identity on either side, to the bit.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KIDMP_RADLAYER_FN __host__ __device__ inline
#else
#define KIDMP_RADLAYER_FN inline
#endif

namespace kidmp {

struct RadLayer { double R, T, a; };
struct RadState { double Rt, Rb, T, Eu, Ed; };

KIDMP_RADLAYER_FN RadState rad_identity() { return RadState{0., 0., 1., 0., 0.}; }

// x of the layer; +0.0 in the two branches that take no exponential
KIDMP_RADLAYER_FN double rad_layer_x(double ta, double b) { return ta > 0. ? std::sqrt(ta * (ta + 2. * b)) : 0.; }

// x = rad_layer_x(ta, b), e = exp(-x/mu), f = 1 - e formed without cancellation
KIDMP_RADLAYER_FN RadLayer rad_layer(double ta, double b, double x, double mu, double e, double f)
{
    RadLayer l;
    if (!(ta > 0.)) {
        if (!(b > 0.)) { l.R = 0.; l.T = 1.; l.a = 0.; return l; }
        const double c = b / mu;
        l.R = c / (1. + c);
        l.T = 1. / (1. + c);
        l.a = 0.;
        return l;
    }
    const double S = (ta + b) + x;
    const double G = b / S;
    const double H = (ta + x) / S;
    const double p = H + G * f;
    const double q = 1. + G * e;
    l.R = (G * f * (1. + e)) / (p * q);
    l.T = (H * (1. + G) * e) / (p * q);
    l.a = (H * f) / q;
    return l;
}

KIDMP_RADLAYER_FN RadState rad_state(const RadLayer &l, double t)
{
    const double em = l.a * t;
    return RadState{l.R, l.R, l.T, em, em};
}

// the stack of A below B
KIDMP_RADLAYER_FN RadState rad_combine(const RadState &A, const RadState &B)
{
    const double d = 1. - A.Rt * B.Rb;
    RadState c;
    c.T = (A.T * B.T) / d;
    c.Rb = A.Rb + ((A.T * A.T) * B.Rb) / d;
    c.Rt = B.Rt + ((B.T * B.T) * A.Rt) / d;
    c.Eu = B.Eu + (B.T * (A.Eu + A.Rt * B.Ed)) / d;
    c.Ed = A.Ed + (A.T * (B.Ed + B.Rb * A.Eu)) / d;
    return c;
}

// The closure at a face: P the stack below it down to the surface, S the stack above it up to space.  rs = 1 - emissivity,
// ts the surface temperature, tc the cosmic background.  up: the brightness temperature going upwards through the face,
// down: the one coming down through it.
struct RadFace { double up, down; };
KIDMP_RADLAYER_FN RadFace rad_face(const RadState &P, const RadState &S, double emissivity, double rs, double ts, double tc)
{
    const double ds = 1. - rs * P.Rb;
    const double Rt = P.Rt + ((P.T * P.T) * rs) / ds;
    const double Eu = P.Eu + (P.T * (emissivity * ts + rs * P.Ed)) / ds;
    const double Dn = S.Ed + S.T * tc;
    const double d = 1. - Rt * S.Rb;
    RadFace f;
    f.up = (Eu + Rt * Dn) / d;
    f.down = (Dn + S.Rb * Eu) / d;
    return f;
}

}  // namespace kidmp
