// kidmp_spheroid.h -- the per-particle model of include/kidmp_polarimetric.h: Rayleigh-Gans scattering by an oblate
// spheroid and the seven numbers per diameter bin that k_polarimetric folds into the scheme's size distributions.  Host
// code in plain C++ with nothing of HIP in it, binary64, every operation written out in real and imaginary parts and
// rounded once (build without contraction), so that tests/polarimetric_ref.py can follow it operation for operation and a
// host program can run it under the sanitizers (tests/native/spheroid_check.cpp).  Of libm it uses sqrt, atan and exp.
//
// The particle: an oblate spheroid of equal-volume diameter D and axis ratio r = b/a <= 1, the symmetry axis a vertical in
// the mean.
//   shape     f**2 = 1/r**2 - 1;   L_a = ((1 + f**2)/f**2) (1 - atan(f)/f), the depolarisation factor along the symmetry
//             axis.  For f**2 < 1/64 the closed form loses 1/f**2 ulps, so the series
//             L_a = (1 + f**2) sum_{n=1..12} (-1)**(n+1) f**(2(n-1))/(2n+1) takes over, ascending in n from +0.0 (the two
//             agree to 1.2e-14 at the switch).  L_b = 0.5 (1 - L_a).  r >= 1: L_a = L_b = 1.0/3.0 explicitly, the sphere.
//   P_j       = (eps - 1)/(3 (1 + L_j (eps - 1))), j = a, b: the polarisability per unit volume; P(1/3) = K(eps).
//             Delta = P_b - P_a.
//   canting   Gaussian with zero mean and width sigma (radians).  With q = exp(-2 sigma**2) the angular moments are those of
//             Ryzhkov et al. (2011), and from here on the project's definition:
//               A1 = (1/4)(1 + q)**2                A2 = (1/4)(1 - q**2)
//               A3 = (3/8 + q/2 + q**4/8)**2         A4 = (3/8 - q/2 + q**4/8)(3/8 + q/2 + q**4/8)
//               A5 = (1/8)(3/8 + q/2 + q**4/8)(1 - q**4)                  A7 = (1/2) q (1 + q)
//             sigma = 0 gives (1, 0, 1, 0, 0, 1) exactly.
//   rows      0 s_h   D**6 (|P_b|**2 - 2 A2 Re(conj(P_b) Delta) + A4 |Delta|**2)
//             1 s_v   the same with A1, A3
//             2 c_re, 3 c_im   D**6 (|P_b|**2 + A5 |Delta|**2 - A1 conj(P_b) Delta - A2 P_b conj(Delta))
//             4 s_0   D**6 |P(1/3)|**2, through the function of row 0 with Delta = 0
//             5 k     D**3 Re(Delta) A7
//             6 mass  the species' mass, as row 3 of the Mie table
//             With Delta = 0 the rows 0, 1, 2 and 4 are the same bits and row 3 is +0.0.
//   species   rain: water, eps_w, r(D) = clamp(c0 + d (c1 + d (c2 + d (c3 + d c4))), r_min, 1) with d = D*1e3;
//             snow, graupel: the soft particle of kidmp_mie_sphere.h (mie_permittivity) with a constant axis ratio each.
// The defaults of pol_defaults (Brandes et al. 2002 for rain, 0.75 and 0.8, sigma = 10, 40, 40 degrees) are illustrative,
// not values of record.
#pragma once

#include <cmath>

#include "kidmp_mie_sphere.h"

namespace kidmp {

constexpr int POL_ROWS = 7;

// what kidmp_pol_cfg holds
struct PolCfg {
    double axis_r[5], axis_r_min, axis_s, axis_g, sigma[3];
    int force_quadrature;
};
// Illustrative, not values of record: Brandes et al. (2002) for rain, constant ratios for snow and graupel, canting
// widths of 10, 40 and 40 degrees.
inline PolCfg pol_defaults()
{
    const double deg = MIE_PI / 180.;
    return PolCfg{{0.9951, 0.02510, -0.03644, 0.005303, -0.0002492}, 0.2, 0.75, 0.8, {10. * deg, 40. * deg, 40. * deg}, 0};
}
// nullptr where the configuration is good, else what is wrong with it
inline const char *pol_bad_cfg(const PolCfg &p)
{
    const double members[] = {p.axis_r[0], p.axis_r[1], p.axis_r[2], p.axis_r[3], p.axis_r[4], p.axis_r_min, p.axis_s, p.axis_g,
                              p.sigma[0], p.sigma[1], p.sigma[2]};
    for (double m : members)
        if (!std::isfinite(m)) return "a member of the polarimetric configuration is not finite";
    if (!(p.axis_r_min > 0. && p.axis_r_min <= 1.) || !(p.axis_s > 0. && p.axis_s <= 1.) || !(p.axis_g > 0. && p.axis_g <= 1.))
        return "axis_r_min, axis_s and axis_g must be in (0, 1]";
    if (p.sigma[0] < 0. || p.sigma[1] < 0. || p.sigma[2] < 0.) return "sigma must not be below 0";
    return nullptr;
}

struct SpheroidShape { double La, Lb; };
inline SpheroidShape spheroid_shape(double r)
{
    if (r >= 1.) return SpheroidShape{1.0 / 3.0, 1.0 / 3.0};
    const double f2 = 1. / (r * r) - 1.;
    double La;
    if (f2 < 1. / 64.) {
        double sum = 0., p = 1., sign = 1.;                  // p = f**(2(n-1))
        for (int n = 1; n <= 12; ++n) {
            sum = sum + (sign * p) / double(2 * n + 1);
            p = p * f2;
            sign = -sign;
        }
        La = (1. + f2) * sum;
    } else {
        const double f = std::sqrt(f2);
        La = ((1. + f2) / f2) * (1. - std::atan(f) / f);
    }
    return SpheroidShape{La, 0.5 * (1. - La)};
}

// P = (eps - 1)/(3 (1 + L (eps - 1)))
inline BBComplex spheroid_P(BBComplex eps, double L)
{
    const BBComplex e1 = {eps.re - 1., eps.im};
    const BBComplex den = {3. * (1. + L * e1.re), 3. * (L * e1.im)};
    return bb_div(e1, den);
}

struct PolMoments { double A1, A2, A3, A4, A5, A7; };
inline PolMoments pol_moments(double sigma)
{
    const double q = std::exp(-2. * (sigma * sigma));
    const double q2 = q * q, q4 = q2 * q2;
    const double plus = (0.375 + 0.5 * q) + 0.125 * q4, minus = (0.375 - 0.5 * q) + 0.125 * q4;
    PolMoments m;
    m.A1 = 0.25 * ((1. + q) * (1. + q));
    m.A2 = 0.25 * (1. - q2);
    m.A3 = plus * plus;
    m.A4 = minus * plus;
    m.A5 = 0.125 * (plus * (1. - q4));
    m.A7 = 0.5 * (q * (1. + q));
    return m;
}

// d6 (|P_b|**2 - 2 Aa Re(conj(P_b) Delta) + Ab |Delta|**2): s_h with (A2, A4), s_v with (A1, A3), s_0 with Delta = 0
inline double pol_copolar(double d6, BBComplex Pb, BBComplex dl, double Aa, double Ab)
{
    const double pb2 = Pb.re * Pb.re + Pb.im * Pb.im;
    const double re = Pb.re * dl.re + Pb.im * dl.im;
    const double dd = dl.re * dl.re + dl.im * dl.im;
    return d6 * ((pb2 - (2. * Aa) * re) + Ab * dd);
}

// rows 0..5 of a spheroid of permittivity eps, axis ratio `ratio` and equal-volume diameter D
inline void pol_spheroid(BBComplex eps, double ratio, const PolMoments &A, double D, double *r)
{
    const SpheroidShape s = spheroid_shape(ratio);
    const BBComplex Pa = spheroid_P(eps, s.La), Pb = spheroid_P(eps, s.Lb), P0 = spheroid_P(eps, 1.0 / 3.0);
    const BBComplex dl = {Pb.re - Pa.re, Pb.im - Pa.im}, none = {0., 0.};
    const double d3 = (D * D) * D, d6 = d3 * d3;
    const double pb2 = Pb.re * Pb.re + Pb.im * Pb.im;
    const double dd = dl.re * dl.re + dl.im * dl.im;
    const double re = Pb.re * dl.re + Pb.im * dl.im;         // Re(conj(P_b) Delta) = Re(P_b conj(Delta))
    const double im1 = Pb.re * dl.im - Pb.im * dl.re;        // Im(conj(P_b) Delta)
    const double im2 = Pb.im * dl.re - Pb.re * dl.im;        // Im(P_b conj(Delta))
    r[0] = pol_copolar(d6, Pb, dl, A.A2, A.A4);
    r[1] = pol_copolar(d6, Pb, dl, A.A1, A.A3);
    r[2] = d6 * (((pb2 + A.A5 * dd) - A.A1 * re) - A.A2 * re);
    r[3] = d6 * ((0. - A.A1 * im1) - A.A2 * im2);
    r[4] = pol_copolar(d6, P0, none, A.A2, A.A4);
    r[5] = (d3 * dl.re) * A.A7;
}

// rain's axis ratio at diameter D
inline double pol_rain_ratio(const PolCfg &p, double D)
{
    const double d = D * 1e3;
    const double r = p.axis_r[0] + d * (p.axis_r[1] + d * (p.axis_r[2] + d * (p.axis_r[3] + d * p.axis_r[4])));
    return r < p.axis_r_min ? p.axis_r_min : r > 1. ? 1. : r;
}

// rows[r*nb + b], r = s_h, s_v, c_re, c_im, s_0, k, mass, of the nb diameters D.  False: an unknown species or a D that
// is not finite or not above 0; the rows are then unspecified.
inline bool pol_bins(const MieCfg &c, const PolCfg &p, int species, int nb, const double *D, double *rows)
{
    if (species < MIE_RAIN || species > MIE_GRAUPEL) return false;
    const PolMoments A = pol_moments(p.sigma[species]);
    for (int b = 0; b < nb; ++b) {
        const double d = D[b];
        if (!std::isfinite(d) || !(d > 0.)) return false;
        const double d2 = d * d, d3 = d2 * d;
        const double mass = species == MIE_RAIN ? (PI / 6.0) * c.rho_w * d3 : species == MIE_SNOW ? am_s * d2 : am_g * d3;   // as mie_bins
        const double ratio = species == MIE_RAIN ? pol_rain_ratio(p, d) : species == MIE_SNOW ? p.axis_s : p.axis_g;
        double r[POL_ROWS - 1];
        pol_spheroid(mie_permittivity(c, species, d, mass), ratio, A, d, r);
        for (int i = 0; i < POL_ROWS - 1; ++i) rows[i * nb + b] = r[i];
        rows[(POL_ROWS - 1) * nb + b] = mass;
    }
    return true;
}

// Whether the species' permittivity and axis ratio do not depend on D, so that the ratios of its rows are the same in every
// bin: a constant axis ratio and a mass exponent of 3.  Graupel in this scheme; rain's ratio follows D, snow's bm_s is 2.
inline bool pol_uniform(int species) { return species == MIE_GRAUPEL ? bm_g == 3.0 : species == MIE_SNOW ? bm_s == 3.0 : false; }

}  // namespace kidmp
