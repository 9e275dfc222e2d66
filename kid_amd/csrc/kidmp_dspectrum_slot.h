// kidmp_dspectrum_slot.h -- where a position on the velocity grid of include/kidmp_dspectrum.h lands: the one place where
// a floating number becomes an index of the Doppler spectrum.  Plain C++ for host and device alike, with nothing of HIP
// in it, so that the function the kernel calls is the function a host program can test (tests/native/dspectrum_slot_check.cpp).
//
// The grid has nv bins of width dv, v0 the centre of bin 0, and nv + 2 slots: `below` (index -1), the bins 0 .. nv-1 and
// `above` (index nv).  A position p = (v - v0)/dv is clamped to [-1, nv]; its mass goes to slot j = min(floor(p), nv-1)
// with weight 1 - f and to slot j + 1 with weight f = p - j, so that j is in [-1, nv-1], j + 1 in [0, nv] and f in [0, 1].
// The clamp is written so that a NaN takes its first branch: a NaN position lies in `below` (j = -1, f = 0), -inf and any
// p < -1 likewise, +inf and any p > nv in `above` (j = nv-1, f = 1).  The integer is clamped again after the conversion.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KIDMP_SLOT_FN __host__ __device__ inline
#else
#define KIDMP_SLOT_FN inline
#endif

namespace kidmp {

struct DSpectrumSlot {
    int j;          // -1 .. nv-1: the lower of the two slots, -1 = below
    double f;       // 0 .. 1: the share of slot j + 1
};

// 1 <= nv; p may be anything
KIDMP_SLOT_FN DSpectrumSlot dspectrum_slot(double p, int nv)
{
    const double top = double(nv);
    const double q = !(p >= -1.) ? -1. : (p > top ? top : p);       // in [-1, nv], NaN -> -1
    // floor of a number in [-1, nv], without <cmath>: truncation rounds towards zero, which is one too high below zero
    int j = int(q);
    if (double(j) > q) --j;
    j = j < -1 ? -1 : (j > nv - 1 ? nv - 1 : j);
    DSpectrumSlot s;
    s.j = j;
    s.f = q - double(j);
    return s;
}

}  // namespace kidmp
