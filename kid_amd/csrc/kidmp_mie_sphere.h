// kidmp_mie_sphere.h -- the per-particle model of include/kidmp_mie.h: the Lorenz-Mie series of a homogeneous sphere and
// the five numbers per diameter bin that k_mie_radar folds into the scheme's size distributions.  Host code in plain C++
// with nothing of HIP in it, binary64, every operation written out in real and imaginary parts and rounded once (build
// without contraction), so that tests/mie_ref.py can follow it operation for operation and a host program can run it
// under the sanitizers (tests/native/mie_sphere_check.cpp).  Of libm it uses sin, cos, sqrt, pow and exp.
//
// The series is Bohren & Huffman's (1983, appendix A), in the convention m = n + i k with k >= 0:
//   y      = m x
//   nstop  = int(x + 4 x**(1/3) + 2);   nmx = int(max(nstop, |y|)) + 15
//   D_n(y) downward from D_nmx = 0:     D_{n-1} = n/y - 1/(D_n + n/y)
//   psi_n, chi_n upward from psi_0 = cos x, psi_1 = sin x, chi_0 = -sin x, chi_1 = cos x:
//                                       psi_n = ((2n-1)/x) psi_{n-1} - psi_{n-2};   xi_n = psi_n - i chi_n
//   a_n = ((D_n/m + n/x) psi_n - psi_{n-1}) / ((D_n/m + n/x) xi_n - xi_{n-1})
//   b_n = ((m D_n + n/x) psi_n - psi_{n-1}) / ((m D_n + n/x) xi_n - xi_{n-1})
//   Q_ext  = (2/x**2) sum (2n+1) Re(a_n + b_n);     Q_back = |sum (2n+1) (-1)**n (a_n - b_n)|**2 / x**2
// Q_back is the radar backscatter efficiency sigma_back/(pi a**2); its Rayleigh limit is 4 x**4 |K(m**2)|**2.
//
// The particle models are the project's own convention, not a standard's and not any instrument simulator's:
//   rain     a water sphere of diameter D: m = sqrt(eps_w), mass = (PI/6) rho_w D**3
//   snow     a soft sphere of diameter D and mass am_s D**bm_s: ice volume fraction f = min(1, mass/(rho_i (PI/6) D**3)),
//            permittivity of ice inclusions in air by Maxwell-Garnett, eps = (1 + 2 f K(eps_i))/(1 - f K(eps_i)) with the
//            K and the complex division of kidmp_brightband_mix.h; m = sqrt(eps)
//   graupel  the same with am_g D**bm_g
// (PI is the scheme's ten-digit one in masses and volumes, as in kidmp_brightband_mix.h; the size parameter x = pi D/lambda
// and the cross-sections pi D**2/4 take pi in full.)  Per bin:
//   s_mie = lambda**4/(pi**5 kw2) * sigma_back          m**6
//   s_ray = D**6 (rain), ZE_SNOW_FAC D**4 (snow), ZE_GRAUPEL_FAC D**6 (graupel): what ze_x of M:5127-5136 integrates
//   s_ext = sigma_ext                                   m**2
//   mass                                                kg
//   v0    = av_x D**bv_x exp(-fv_x D)                   m/s at RHO_NOT (graupel has no exponential)
#pragma once

#include <cmath>
#include <vector>

#include "kidmp_brightband_mix.h"
#include "thompson_params.h"

namespace kidmp {

constexpr double MIE_PI = 3.14159265358979323846;
constexpr int MIE_ROWS = 5, MIE_RAIN = 0, MIE_SNOW = 1, MIE_GRAUPEL = 2;
constexpr int MIE_MAX_TERMS = 10000000;              // nmx beyond this is refused: |m| x of ten million

// what kidmp_mie_cfg holds, with eps_w and eps_i as complex numbers
struct MieCfg {
    double wavelength;
    BBComplex eps_w, eps_i;
    double rho_w, rho_i, kw2;
};

// the root of eps with a real part above 0; Im(eps) >= 0 gives Im(m) >= 0.  The imaginary part comes from the product
// 2 Re(m) Im(m) = Im(eps), not from |eps| - Re(eps), which cancels for a weak absorber.
inline BBComplex mie_sqrt(BBComplex e)
{
    const double mod = std::sqrt(e.re * e.re + e.im * e.im);
    BBComplex m;
    if (e.re >= 0.) {
        m.re = std::sqrt(0.5 * (mod + e.re));
        m.im = m.re > 0. ? e.im / (2. * m.re) : 0.;
    } else {
        m.im = std::sqrt(0.5 * (mod - e.re));
        m.re = e.im / (2. * m.im);
    }
    return m;
}

// Q_ext and Q_back of a sphere of size parameter x and refractive index m.  False, nothing written: x or m not finite,
// x not above 0, Re(m) not above 0, Im(m) below 0, or more than MIE_MAX_TERMS terms of D_n.
inline bool mie_sphere(double x, double m_re, double m_im, double &qext, double &qback)
{
    if (!(std::isfinite(x) && std::isfinite(m_re) && std::isfinite(m_im)) || !(x > 0.) || !(m_re > 0.) || m_im < 0.) return false;
    const BBComplex m = {m_re, m_im};
    const BBComplex y = {m_re * x, m_im * x};
    const double ymod = std::sqrt(y.re * y.re + y.im * y.im);
    const double xstop = x + 4. * std::pow(x, 1. / 3.) + 2.;
    if (!(xstop < double(MIE_MAX_TERMS)) || !(ymod < double(MIE_MAX_TERMS))) return false;
    const int nstop = int(xstop);
    const int nmx = int(double(nstop) > ymod ? double(nstop) : ymod) + 15;
    std::vector<double> d_re(size_t(nmx) + 1), d_im(size_t(nmx) + 1);
    d_re[size_t(nmx)] = 0.;
    d_im[size_t(nmx)] = 0.;
    const BBComplex one = {1., 0.};
    for (int n = nmx; n >= 1; --n) {
        const BBComplex en = {double(n), 0.};
        const BBComplex ny = bb_div(en, y);
        const BBComplex s = {d_re[size_t(n)] + ny.re, d_im[size_t(n)] + ny.im};
        const BBComplex r = bb_div(one, s);
        d_re[size_t(n) - 1] = ny.re - r.re;
        d_im[size_t(n) - 1] = ny.im - r.im;
    }
    double psi0 = std::cos(x), psi1 = std::sin(x);
    double chi0 = -std::sin(x), chi1 = std::cos(x);
    double sum_ext = 0., back_re = 0., back_im = 0., sign = -1.;
    for (int n = 1; n <= nstop; ++n) {
        const double en = double(n), f = (2. * en - 1.) / x, nx = en / x;
        const double psi = f * psi1 - psi0;
        const double chi = f * chi1 - chi0;
        const BBComplex d = {d_re[size_t(n)], d_im[size_t(n)]};
        const BBComplex dm = bb_div(d, m), md = bb_mul(m, d);
        const BBComplex ta = {dm.re + nx, dm.im}, tb = {md.re + nx, md.im};
        // xi_n = psi - i chi, xi_{n-1} = psi1 - i chi1
        const BBComplex xi = {psi, -chi}, xi1 = {psi1, -chi1};
        const BBComplex txa = bb_mul(ta, xi), txb = bb_mul(tb, xi);
        const BBComplex an_num = {ta.re * psi - psi1, ta.im * psi}, an_den = {txa.re - xi1.re, txa.im - xi1.im};
        const BBComplex bn_num = {tb.re * psi - psi1, tb.im * psi}, bn_den = {txb.re - xi1.re, txb.im - xi1.im};
        const BBComplex an = bb_div(an_num, an_den), bn = bb_div(bn_num, bn_den);
        const double w = 2. * en + 1.;
        sum_ext = sum_ext + w * (an.re + bn.re);
        back_re = back_re + (w * sign) * (an.re - bn.re);
        back_im = back_im + (w * sign) * (an.im - bn.im);
        sign = -sign;
        psi0 = psi1; psi1 = psi;
        chi0 = chi1; chi1 = chi;
    }
    const double x2 = x * x;
    qext = (2. / x2) * sum_ext;
    qback = (back_re * back_re + back_im * back_im) / x2;
    return true;
}

// the refractive index of the species' particle of diameter D
inline BBComplex mie_index(const MieCfg &c, int species, double D, double mass)
{
    if (species == MIE_RAIN) return mie_sqrt(c.eps_w);
    const double PI_6 = PI / 6.0;
    const double sphere = PI_6 * D * D * D;
    const double vi = mass / c.rho_i;
    const double f = vi < sphere ? vi / sphere : 1.;
    const BBComplex k = bb_K(c.eps_i);
    const BBComplex fk = {f * k.re, f * k.im};
    const BBComplex num = {1. + 2. * fk.re, 2. * fk.im}, den = {1. - fk.re, -fk.im};
    return mie_sqrt(bb_div(num, den));
}

// rows[r*nb + b], r = s_mie, s_ray, s_ext, mass, v0, of the nb diameters D.  False: an unknown species, a D that is not
// finite or not above 0, or a sphere that mie_sphere refuses; the rows are then unspecified.
inline bool mie_bins(const MieCfg &c, int species, int nb, const double *D, double *rows)
{
    if (species < MIE_RAIN || species > MIE_GRAUPEL) return false;
    const double ZE_ICE = (0.176 / 0.93) * (6.0 / PI) * (6.0 / PI);                  // M:5131-5135, as thompson_levels.h
    const double ZE_SNOW = ZE_ICE * (am_s / 900.0) * (am_s / 900.0), ZE_GRAUPEL = ZE_ICE * (am_g / 900.0) * (am_g / 900.0);
    const double lam = c.wavelength, lam2 = lam * lam;
    const double pi2 = MIE_PI * MIE_PI, pi5 = pi2 * pi2 * MIE_PI;
    const double scale = (lam2 * lam2) / (pi5 * c.kw2);
    for (int b = 0; b < nb; ++b) {
        const double d = D[b];
        if (!std::isfinite(d) || !(d > 0.)) return false;
        const double d2 = d * d, d3 = d2 * d;
        double mass, ray, v0;
        if (species == MIE_RAIN) {
            mass = (PI / 6.0) * c.rho_w * d3;
            ray = d3 * d3;
            v0 = av_r * std::pow(d, bv_r) * std::exp(-fv_r * d);
        } else if (species == MIE_SNOW) {
            mass = am_s * d2;                                                         // bm_s = 2
            ray = ZE_SNOW * (d2 * d2);
            v0 = av_s * std::pow(d, bv_s) * std::exp(-fv_s * d);
        } else {
            mass = am_g * d3;                                                         // bm_g = 3
            ray = ZE_GRAUPEL * (d3 * d3);
            v0 = av_g * std::pow(d, bv_g);
        }
        const BBComplex m = mie_index(c, species, d, mass);
        const double x = MIE_PI * d / lam;
        double qext, qback;
        if (!mie_sphere(x, m.re, m.im, qext, qback)) return false;
        const double area = 0.25 * MIE_PI * d2;
        rows[0 * nb + b] = scale * (qback * area);
        rows[1 * nb + b] = ray;
        rows[2 * nb + b] = qext * area;
        rows[3 * nb + b] = mass;
        rows[4 * nb + b] = v0;
    }
    return true;
}

// the closed-form Rayleigh absorption of cloud water per unit of liquid volume fraction: (6 pi/lambda) Im(K(eps_w)), 1/m.
// (In this file's convention, Im(eps) >= 0, the absorbing part of K is +Im(K); a text that writes eps = e' - i e'' has
// Im(-K) in its place.)
inline double mie_cloud_absorption(const MieCfg &c)
{
    const BBComplex k = bb_K(c.eps_w);
    return (6. * MIE_PI / c.wavelength) * k.im;
}

}  // namespace kidmp
