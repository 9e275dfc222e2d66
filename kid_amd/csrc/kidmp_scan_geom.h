// kidmp_scan_geom.h -- internal to kidmp_scan.hip (not installed): where the centre of range gate g of a slant beam lies
// in a slab, as include/kidmp_scan.h states it operation by operation.  Host and device, so that the classification that
// guards every gather of k_scan is checked on the CPU (tests/native/scan_geom_check.cpp).  Binary64, every operation
// rounded once: compile without contraction.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KSG_FN __host__ __device__ inline
#else
#define KSG_FN inline
#endif

namespace kidmp {
namespace scan {
constexpr int RAY_WORDS = 6;                             // a row of the ray table: slab, x0, z0, ce, se, wgt
struct Ray { double slab, x0, z0, ce, se, wgt; };
struct Grid {
    double r0, dr, dx, half_inv_ae;
    int64_t nslab;
    int32_t nx, nz, periodic;
};
// inside: (i, k) name a cell of the slab; otherwise i = k = -1.  h is what the formula gives either way.
struct Sample { double h; int32_t i, k; bool inside; };

KSG_FN bool is_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }   // false for a NaN

// the row can hit a cell at all: slab a whole number in [0, nslab), wgt finite and above 0
KSG_FN bool ray_valid(const Ray &r, int64_t nslab)
{
    return r.slab >= 0. && r.slab < double(nslab) && r.slab == __builtin_floor(r.slab) && r.wgt > 0. && is_finite(r.wgt);
}

// the trip count of level_of: the smallest t with 2**t > nz, so that the steps 2**(t-1) .. 1 can reach every count up to nz + 1
KSG_FN int level_steps(int nz)
{
    int t = 0;
    while ((1 << t) <= nz) ++t;
    return t;
}

// (the number of faces zf[0 .. nz] that are <= h) - 1, by a binary search whose trip count depends on nz alone.  Every
// index it forms lies in [0, nz] whatever zf holds; for an ascending zf the count is exact.
template <class ZF>
KSG_FN int level_of(const ZF &zf, int nz, int steps, double h)
{
    int pos = 0;
    for (int t = steps - 1; t >= 0; --t) {
        const int next = pos + (1 << t);
        if (next <= nz + 1 && zf[next - 1] <= h) pos = next;
    }
    return pos - 1;
}

template <class ZF>
KSG_FN Sample sample(const Ray &ray, const Grid &g, const ZF &zf, int steps, int gate)
{
    const double r = g.r0 + (double(gate) + 0.5) * g.dr;
    const double s = r * ray.ce;
    const double x = ray.x0 + s;
    const double h = (ray.z0 + r * ray.se) + (s * s) * g.half_inv_ae;
    Sample out{h, -1, -1, false};
    if (!is_finite(x) || !is_finite(h)) return out;
    const double xi = __builtin_floor(x / g.dx);
    if (!(__builtin_fabs(xi) < 4503599627370496.)) return out;       // 2**52: beyond it xi is no cell index
    int64_t i = int64_t(xi);
    if (g.periodic) {
        i %= int64_t(g.nx);
        if (i < 0) i += g.nx;
    } else if (i < 0 || i >= g.nx) {
        return out;
    }
    if (!(zf[0] <= h && h < zf[g.nz])) return out;
    const int k = level_of(zf, g.nz, steps, h);
    if (k < 0 || k >= g.nz) return out;                              // only a zf that does not ascend gets here
    out.i = int32_t(i);
    out.k = k;
    out.inside = true;
    return out;
}
}  // namespace scan
}  // namespace kidmp
