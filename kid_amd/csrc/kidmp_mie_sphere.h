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
//   Q_sca  = (2/x**2) sum (2n+1) (|a_n|**2 + |b_n|**2)
//   g Q_sca = (4/x**2) [sum (n(n+2)/(n+1)) Re(a_n conj(a_{n+1}) + b_n conj(b_{n+1})) + sum ((2n+1)/(n(n+1))) Re(a_n conj(b_n))]
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

// The sums of the series, for mie_sphere and for the radiometer's efficiencies (include/kidmp_radiometer.h): the a_n, b_n
// loop exists once.  ext = sum (2n+1) Re(a_n + b_n); back = sum (2n+1)(-1)**n (a_n - b_n); sca = sum (2n+1)(|a_n|**2 +
// |b_n|**2); adj = sum_{n<nstop} (n(n+2)/(n+1)) Re(a_n conj(a_{n+1}) + b_n conj(b_{n+1})); ab = sum ((2n+1)/(n(n+1)))
// Re(a_n conj(b_n)).  Each sum ascends in n from +0.0.
struct MieSeries { double ext, back_re, back_im, sca, adj, ab, x2; };

// False, nothing written: x or m not finite, x not above 0, Re(m) not above 0, Im(m) below 0, or more than MIE_MAX_TERMS
// terms of D_n.
inline bool mie_series(double x, double m_re, double m_im, MieSeries &out)
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
    double sum_sca = 0., sum_adj = 0., sum_ab = 0.;
    BBComplex pa = {0., 0.}, pb = {0., 0.};                // a_{n-1}, b_{n-1}
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
        sum_sca = sum_sca + w * ((an.re * an.re + an.im * an.im) + (bn.re * bn.re + bn.im * bn.im));
        if (n > 1) {
            const double e1 = en - 1.;                       // the pair (n-1, n)
            sum_adj = sum_adj + ((e1 * (e1 + 2.)) / (e1 + 1.)) * ((pa.re * an.re + pa.im * an.im) + (pb.re * bn.re + pb.im * bn.im));
        }
        sum_ab = sum_ab + (w / (en * (en + 1.))) * (an.re * bn.re + an.im * bn.im);
        pa = an; pb = bn;
        sign = -sign;
        psi0 = psi1; psi1 = psi;
        chi0 = chi1; chi1 = chi;
    }
    out = MieSeries{sum_ext, back_re, back_im, sum_sca, sum_adj, sum_ab, x * x};
    return true;
}

// Q_ext and Q_back of a sphere of size parameter x and refractive index m.  False, nothing written: as mie_series.
inline bool mie_sphere(double x, double m_re, double m_im, double &qext, double &qback)
{
    MieSeries s;
    if (!mie_series(x, m_re, m_im, s)) return false;
    qext = (2. / s.x2) * s.ext;
    qback = (s.back_re * s.back_re + s.back_im * s.back_im) / s.x2;
    return true;
}

// The efficiencies a radiometer needs beside them: Q_sca = (2/x**2) sca, gQ = g*Q_sca = (4/x**2) (adj + ab), and the
// asymmetry factor g = gQ/Q_sca (+0.0 where Q_sca is not above 0).  Q_ext and Q_back are mie_sphere's bit for bit.
struct MieEff { double qext, qsca, qback, g, gq; };
inline bool mie_efficiencies(double x, double m_re, double m_im, MieEff &e)
{
    MieSeries s;
    if (!mie_series(x, m_re, m_im, s)) return false;
    e.qext = (2. / s.x2) * s.ext;
    e.qback = (s.back_re * s.back_re + s.back_im * s.back_im) / s.x2;
    e.qsca = (2. / s.x2) * s.sca;
    e.gq = (4. / s.x2) * (s.adj + s.ab);
    e.g = e.qsca > 0. ? e.gq / e.qsca : 0.;
    return true;
}

// the permittivity of the species' particle of diameter D: water, or the soft particle's Maxwell-Garnett ice in air
// (kidmp_spheroid.h takes it from here too)
inline BBComplex mie_permittivity(const MieCfg &c, int species, double D, double mass)
{
    if (species == MIE_RAIN) return c.eps_w;
    const double PI_6 = PI / 6.0;
    const double sphere = PI_6 * D * D * D;
    const double vi = mass / c.rho_i;
    const double f = vi < sphere ? vi / sphere : 1.;
    const BBComplex k = bb_K(c.eps_i);
    const BBComplex fk = {f * k.re, f * k.im};
    const BBComplex num = {1. + 2. * fk.re, 2. * fk.im}, den = {1. - fk.re, -fk.im};
    return bb_div(num, den);
}
// the refractive index of the species' particle of diameter D
inline BBComplex mie_index(const MieCfg &c, int species, double D, double mass)
{ return mie_sqrt(mie_permittivity(c, species, D, mass)); }

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

// The radiometer's rows (include/kidmp_radiometer.h), rows[r*nb + b], r = s_abs, s_bsc, mass, with the particle models
// above: s_abs = max(Q_ext - Q_sca, 0) (pi D**2/4), s_bsc = max(0.5 (Q_sca - gQ), 0) (pi D**2/4), the cross-section
// scattered into the backward hemisphere.  A particle whose index is real does not absorb: with Im(m) = 0 s_abs is +0.0, not
// the rounding residue of Q_ext - Q_sca (of either sign; the max would keep the positive half of it).  False as mie_bins.
constexpr int RADIOMETER_ROWS = 3;
inline bool radiometer_bins(const MieCfg &c, int species, int nb, const double *D, double *rows)
{
    if (species < MIE_RAIN || species > MIE_GRAUPEL) return false;
    for (int b = 0; b < nb; ++b) {
        const double d = D[b];
        if (!std::isfinite(d) || !(d > 0.)) return false;
        const double d2 = d * d, d3 = d2 * d;
        const double mass = species == MIE_RAIN ? (PI / 6.0) * c.rho_w * d3 : species == MIE_SNOW ? am_s * d2 : am_g * d3;
        const BBComplex m = mie_index(c, species, d, mass);
        const double x = MIE_PI * d / c.wavelength;
        MieEff e;
        if (!mie_efficiencies(x, m.re, m.im, e)) return false;
        const double area = 0.25 * MIE_PI * d2;
        const double qa = m.im > 0. ? e.qext - e.qsca : 0., qb = 0.5 * (e.qsca - e.gq);
        rows[0 * nb + b] = (qa > 0. ? qa : 0.) * area;
        rows[1 * nb + b] = (qb > 0. ? qb : 0.) * area;
        rows[2 * nb + b] = mass;
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
