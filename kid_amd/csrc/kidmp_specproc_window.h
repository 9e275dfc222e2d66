// kidmp_specproc_window.h -- the per-level window arithmetic of include/kidmp_specproc.h, shared by host and device: the
// half-width H of the broadening kernel, its weights g_d, their norm G, the tails T_m that leave the grid and the
// detection rule.  The kernel (kidmp_specproc.hip) calls exactly these functions, lane by lane; the host program
// tests/native/specproc_window_check.cpp runs them with and without ASan + UBSan.  The exponential is fastmath.h's
// fm::exp, whose host and device results are the same bits, so what the host program prints is what the kernel holds.
// Every operation rounds once (no contraction).
#pragma once
#include <cmath>
#include <cstdint>

#include "fastmath.h"

#if defined(__HIPCC__)
#define KSP_FN __host__ __device__ inline
#else
#define KSP_FN inline
#endif

namespace kidmp {
namespace specproc {

constexpr int MAX_HALF = 256;                            // KIDMP_SPECPROC_MAX_HALF
constexpr double EXP_MAX = 700.;                         // a weight whose exponent exceeds this is exact +0.0 (kidmp_spectra.h's rule)

struct Window { double s; int H; };                      // s = sigma/dv in bins; H = 0: no broadening, s is not read

// sigma that is not above 0 (NaN, zero, negative): H = 0.  Otherwise h = ceil(cut*s), capped at MAX_HALF.  cut is finite and
// above 0 and inv_dv finite and above 0 (the entry refuses anything else), so h is never NaN; the comparison is written so
// that a NaN would take the cap and the conversion to int is always defined.
KSP_FN Window window(double sigma, double inv_dv, double cut)
{
    Window w{0., 0};
    if (!(sigma > 0.)) return w;
    w.s = sigma * inv_dv;
    const double h = std::ceil(cut * w.s);
    w.H = !(h <= double(MAX_HALF)) ? MAX_HALF : int(h);
    return w;
}

// g_d for 1 <= d <= H (g_0 = 1 is taken without an exponential)
KSP_FN double weight(int d, double s)
{
    const double r = double(d) / s;
    const double t = 0.5 * (r * r);
    return t <= EXP_MAX ? fm::exp(-t) : 0.;
}

// G = g_0 + sum_{d = 1 .. H} (g_d + g_d), ascending; keep(d, g_d) sees every weight as it is formed
template <class Keep>
KSP_FN double norm(const Window &w, Keep &&keep)
{
    double G = 1.;
    for (int d = 1; d <= w.H; ++d) {
        const double g = weight(d, w.s);
        keep(d, g);
        G += g + g;
    }
    return G;
}

// T_m = sum_{d = m .. H} g_d, summed from d = H down: keep(m, T_m) for m = H down to 1; g(d) returns g_d
template <class Get, class Keep>
KSP_FN void tails(const Window &w, Get &&g, Keep &&keep)
{
    double t = 0.;
    for (int d = w.H; d >= 1; --d) {
        t += g(d);
        keep(d, t);
    }
}

// bin j is detected iff B_j > snr_min*n_k; a NaN on either side is not detected
KSP_FN bool detected(double B, double threshold) { return B > threshold; }
KSP_FN double threshold(double snr_min, double noise) { return snr_min * noise; }

}  // namespace specproc
}  // namespace kidmp
