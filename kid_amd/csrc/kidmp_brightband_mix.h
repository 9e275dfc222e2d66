// kidmp_brightband_mix.h -- the per-particle dielectric model of include/kidmp_brightband.h: the Rayleigh backscatter
// weight of one melting snow or graupel particle, from Maxwell-Garnett mixing of ice, air and meltwater.  Plain C++ for
// host and device alike, with nothing of HIP in it, so that the function the kernel calls is the function a host program
// can test (tests/native/brightband_mix_check.cpp).  Binary64, every operation written out and rounded once: build
// without contraction.  Complex division multiplies by one real reciprocal of |z|**2.
//
//   m   = am * D**bm                      the particle's mass (the caller forms it: bm_s = 2, bm_g = 3)
//   Vi0 = m / rho_i                       the ice of the unmelted particle
//   Ve  = max((PI/6)*D*D*D, Vi0)          its envelope
//   Vi  = (1 - fm)*Vi0;  Vw = (fm*m)/rho_w;  Va = (1 - fm)*(Ve - Vi0);  c = Vi + Va;  V = c + Vw
//   Kc  = (Vi/c) * K(eps_i)               ice inclusions in air; eps_c = (1 + 2Kc)/(1 - Kc); c not above 0: Kc = 0
//   water matrix:  g = c/V;   b = (eps_c - eps_w)/(eps_c + 2 eps_w);  eps_p = eps_w*((1 + 2 g b)/(1 - g b))
//   ice matrix:    g = Vw/V;  b = (eps_w - eps_c)/(eps_w + 2 eps_c);  eps_p = eps_c*((1 + 2 g b)/(1 - g b))
//   wet = |K(eps_p)|**2 * V * V;          dry = K(eps_i)**2 * Vi0 * Vi0;      K(e) = (e - 1)/(e + 2)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KIDMP_BBMIX_FN __host__ __device__ inline
#else
#define KIDMP_BBMIX_FN inline
#endif

namespace kidmp {

struct BBComplex { double re, im; };

// the configuration as the kernel takes it: kidmp_brightband_cfg with K(eps_i) formed once
struct BBMix {
    double ew_re, ew_im;     // eps_w
    double eps_i, k_i;       // eps_i and K(eps_i) = (eps_i - 1)/(eps_i + 2)
    double rho_w, rho_i;
    int ice_matrix;          // 0: water is the matrix, 1: the ice-air core is
};
// what depends on the bin alone
struct BBBin { double m, Vi0, Ve, dry; };

KIDMP_BBMIX_FN BBComplex bb_div(BBComplex a, BBComplex b)
{
    const double r = 1. / (b.re * b.re + b.im * b.im);
    BBComplex q;
    q.re = (a.re * b.re + a.im * b.im) * r;
    q.im = (a.im * b.re - a.re * b.im) * r;
    return q;
}
KIDMP_BBMIX_FN BBComplex bb_mul(BBComplex a, BBComplex b)
{
    BBComplex q;
    q.re = a.re * b.re - a.im * b.im;
    q.im = a.re * b.im + a.im * b.re;
    return q;
}
// K(e) = (e - 1)/(e + 2)
KIDMP_BBMIX_FN BBComplex bb_K(BBComplex e)
{
    const BBComplex n = {e.re - 1., e.im}, d = {e.re + 2., e.im};
    return bb_div(n, d);
}
KIDMP_BBMIX_FN double bb_K_real(double e) { return (e - 1.) / (e + 2.); }

// m = am * D**bm as the caller formed it; D the bin's diameter
KIDMP_BBMIX_FN BBBin bb_bin(const BBMix &x, double m, double D)
{
    const double PI_6 = 3.1415926536 / 6.0;                          // the scheme's PI (M:53)
    BBBin b;
    b.m = m;
    b.Vi0 = m / x.rho_i;
    const double sphere = PI_6 * D * D * D;
    b.Ve = sphere > b.Vi0 ? sphere : b.Vi0;
    b.dry = x.k_i * x.k_i * b.Vi0 * b.Vi0;
    return b;
}

// the wet particle's weight at melt fraction fm
KIDMP_BBMIX_FN double bb_wet(const BBMix &x, const BBBin &b, double fm)
{
    const double dryf = 1. - fm;
    const double Vi = dryf * b.Vi0;
    const double Vw = (fm * b.m) / x.rho_w;
    const double Va = dryf * (b.Ve - b.Vi0);
    const double c = Vi + Va;
    const double V = c + Vw;
    const double Kc = c > 0. ? (Vi / c) * x.k_i : 0.;
    const double eps_c = (1. + 2. * Kc) / (1. - Kc);
    const BBComplex ew = {x.ew_re, x.ew_im};
    BBComplex bn, bd;
    double g;
    if (!x.ice_matrix) {
        g = c / V;
        bn.re = eps_c - ew.re; bn.im = -ew.im;
        bd.re = eps_c + 2. * ew.re; bd.im = 2. * ew.im;
    } else {
        g = Vw / V;
        bn.re = ew.re - eps_c; bn.im = ew.im;
        bd.re = ew.re + 2. * eps_c; bd.im = ew.im;
    }
    const BBComplex bq = bb_div(bn, bd);
    const BBComplex gb = {g * bq.re, g * bq.im};
    const BBComplex num = {1. + 2. * gb.re, 2. * gb.im}, den = {1. - gb.re, -gb.im};
    const BBComplex q = bb_div(num, den);
    BBComplex ep;
    if (!x.ice_matrix) ep = bb_mul(ew, q);
    else { ep.re = eps_c * q.re; ep.im = eps_c * q.im; }
    const BBComplex Kp = bb_K(ep);
    return (Kp.re * Kp.re + Kp.im * Kp.im) * V * V;
}

}  // namespace kidmp
