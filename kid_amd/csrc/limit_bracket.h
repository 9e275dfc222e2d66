// limit_bracket.h -- the scheme's size-limit tests decided without the cube root.
//
// The scheme bounds a number concentration by a test on a characteristic diameter (M:1420-1445, M:2422-2530):
//
//     lam = (num / den)**(1/3)        num = K n  (K: constants of the species),  den = q (mass content)
//     xD  = c / lam
//     if (xD < D_lo) ... else if (xD > D_hi) ...
//
// Where the branches themselves do not read lam or xD (they install a constant slope c/D, or call nr_from_mvd with a
// constant diameter) the cube root and the two quotients only feed the comparison, and
//
//     xD < D   <=>   lam > c/D   <=>   num > T den,   T = (c/D)**3
//
// decides it with a product and a comparison.  The computed xD carries the roundings of the original path, the product
// T den carries its own, so the two can disagree when num / den lies within a few ulp of T.  decide() therefore tests
// against T (1 + EPS) and T (1 - EPS) and answers AMBIGUOUS when the two disagree; the caller (one wave) then evaluates
// the original expression for all its lanes.  A certain answer is the answer of the original path, whatever the last
// bits of its cube root and quotients are: no result depends on which path was taken.
//
// The margin.  u = 2**-53 (half an ulp, relative); an operation "within 1 ulp" is within 2u.
//   the original path, xD_computed = xD_exact (1 + e):
//     num / den              fm::div, <= 1 ulp (tests/test_fastmath.py, tests/test_gpu_fastmath.py): 2u, a third of it
//                            after the cube root                                                        2/3 u
//     root3                  fm::cbrt_pos, <= 1 ulp                                                     2   u
//     c / lam                fm::div <= 1 ulp (2u), or c * fm::rcp(lam): <= 1 ulp, then a product       3   u
//                                                                                          |e| <=  E_X = 6 u
//   (num and den themselves are the values the original path forms, so their roundings are common to both.)
//   xD (1 + e) < D  <=>  num / den > T (1 + e)**3: the cube triples it                                  18  u
//   the bracket's own roundings:
//     T = (c/D)**3 folded in binary64: quotient u, cubed 3u, two products 2u; the cloud site forms c**3 exactly
//       (c = nu + 4 <= 19) and multiplies by the folded 1/D**3 (two products 2u, quotient u) instead        5 u
//     T (1 +- EPS)           one product                                                                    1 u
//     ... * den              one product (the cloud site: den * c**3, then the constant: two)               2 u
//                                                                                                   total  26 u
//   BOUND = 26 u = 13 * 2**-52 = 2.9e-15;  EPS = 16 * BOUND = 208 * 2**-52 = 4.6e-14 (substeps() of the column kernel
//   brackets a single product by 4e-15, the same order).  A pair is ambiguous only if num / den lies within
//   EPS (1 + 2**-40) of a threshold: a sliver no physical state sits in for long, and harmless when one does.
//
// Domain: num and den positive, finite and within [LIM_TINY, LIM_HUGE], which the sites guarantee for every sane column
// (den > R1, n >= R2).  Anything else -- zero, negative, NaN, Inf, or so large that T den could overflow -- is
// AMBIGUOUS, i.e. handed to the original path, whose behaviour on such input stays what it was.
//
// Plain C++ (host + device, no LDS, no divergent branch): tests/test_limit_bracket.py checks the claims above against
// exact rational arithmetic on the host build, tests/test_gpu_limit_bracket.py against the device's original path.
#pragma once
#include "thompson_params.h"

#if defined(__HIPCC__)
#define KLB_FN __host__ __device__ inline
#else
#define KLB_FN inline
#endif

namespace kidmp {
namespace lb {

enum : int { BELOW = 0, INSIDE = 1, ABOVE = 2, AMBIGUOUS = 3 };

constexpr double ULP = 2.220446049250313e-16;              // 2**-52
constexpr double E_X = 3. * ULP;                           // bound of the original path's relative error in xD (6 u)
constexpr double BOUND = 13. * ULP;                        // original path cubed + the bracket's own roundings (26 u)
constexpr double EPS = 16. * BOUND;
constexpr double LIM_TINY = 1.e-150, LIM_HUGE = 1.e150;

// the four margined factors of one site; lo / hi name the diameters, so lo holds the LARGER ratio (c/D_lo)**3
struct Factors {
    double lo_up, lo_dn, hi_up, hi_dn;
};
// scale**3 / D**3 with margins, folded at compile time.  scale = c for a site whose c is a constant; scale = 1 for the
// cloud site, which multiplies den by c**3 itself (decide_scaled)
constexpr double cube_ratio(double c, double D) { return (c / D) * (c / D) * (c / D); }
constexpr Factors factors(double c, double D_lo, double D_hi)
{
    return Factors{cube_ratio(c, D_lo) * (1. + EPS), cube_ratio(c, D_lo) * (1. - EPS), cube_ratio(c, D_hi) * (1. + EPS),
                   cube_ratio(c, D_hi) * (1. - EPS)};
}

// xD = c / cbrt(num / den) against D_lo < D_hi, f = factors(c, D_lo, D_hi): two products and two comparisons per threshold
KLB_FN bool in_domain(double num, double den) { return num >= LIM_TINY && num <= LIM_HUGE && den >= LIM_TINY && den <= LIM_HUGE; }
KLB_FN int classify(double num, double den, const Factors &f)
{
    const bool below = num > den * f.lo_up, not_below = num < den * f.lo_dn;
    const bool above = num < den * f.hi_dn, not_above = num > den * f.hi_up;
    int r = AMBIGUOUS;
    r = not_below && not_above ? INSIDE : r;
    r = below ? BELOW : r;
    r = above ? ABOVE : r;
    return r;
}
KLB_FN int decide(double num, double den, const Factors &f) { return in_domain(num, den) ? classify(num, den, f) : int(AMBIGUOUS); }
// the same with a run-time c whose cube c3 is exact in binary64 (the cloud site: c = nu + 4), f = factors(1., D_lo, D_hi)
KLB_FN int decide_scaled(double num, double den, double c3, const Factors &f)
{
    return in_domain(num, den) ? classify(num, den * c3, f) : int(AMBIGUOUS);
}

// decide(...) == INSIDE and nothing else, for a caller that has nothing to do inside the limits and hands every other
// case to the original path: one product and one comparison per threshold.  den >= LIM_TINY keeps the products normal,
// num <= LIM_HUGE makes an overflowing den * f.lo_dn harmless (den * f.hi_up is then far above num); zero, negative,
// NaN and Inf operands fail one of the four comparisons.
KLB_FN bool certainly_inside(double num, double den, const Factors &f)
{
    return den >= LIM_TINY && num <= LIM_HUGE && num < den * f.lo_dn && num > den * f.hi_up;
}
KLB_FN bool certainly_inside_scaled(double num, double den, double c3, const Factors &f)
{
    return den >= LIM_TINY && num <= LIM_HUGE && num < den * c3 * f.lo_dn && num > den * c3 * f.hi_up;
}

// ---- the scheme's sites(binary64 values of the expressions the column kernel writes; it asserts that they agree) ----
struct Site {
    double c, D_lo, D_hi;
};
constexpr Site SITE_ICE{bm_i + mu_i + 1., 5.E-6, 300.E-6};             // M:1420-1445, M:2457-2480
constexpr Site SITE_RAIN{3.0 + mu_r + 0.672, D0r * 0.75, 2.5E-3};      // M:2508-2530
constexpr Site SITE_CLOUD{1., D0c, D0r * 2.};                          // M:2422-2445, c = cloud_c(nu)
constexpr double cloud_c(int nu) { return bm_r + nu + 1.; }            // nu = 2 .. 15: c**3 <= 19**3, exact
constexpr Factors F_ICE = factors(SITE_ICE.c, SITE_ICE.D_lo, SITE_ICE.D_hi);
constexpr Factors F_RAIN = factors(SITE_RAIN.c, SITE_RAIN.D_lo, SITE_RAIN.D_hi);
constexpr Factors F_CLOUD = factors(SITE_CLOUD.c, SITE_CLOUD.D_lo, SITE_CLOUD.D_hi);
static_assert(cloud_c(15) <= 32., "c**3 of the cloud test must stay exact in binary64");

}  // namespace lb
}  // namespace kidmp
