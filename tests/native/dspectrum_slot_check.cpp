// dspectrum_slot_check.cpp -- kidmp::dspectrum_slot (kid_amd/csrc/kidmp_dspectrum_slot.h), the function that turns a
// position on the velocity grid into the two slots of the Doppler spectrum, as a host program: built with
// -fsanitize=address,undefined by tests/test_doppler_spectrum_abi.py and run there.  Every position is deposited into a heap
// array of exactly nv + 2 doubles, so a slot outside the array is an AddressSanitizer report, and a conversion of an
// out-of-range double to int is an UndefinedBehaviorSanitizer report.  Exit status 0 and the line "slot ok" mean all held.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "kidmp_dspectrum_slot.h"

using kidmp::DSpectrumSlot;
using kidmp::dspectrum_slot;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void deposit(double *slots, int nv, double p)
{
    const DSpectrumSlot s = dspectrum_slot(p, nv);
    EXPECT(s.j >= -1 && s.j <= nv - 1, "nv=%d p=%g: j=%d", nv, p, s.j);
    EXPECT(s.f >= 0. && s.f <= 1., "nv=%d p=%g: f=%g", nv, p, s.f);
    slots[s.j + 1] += 1. - s.f;                                      // slot -1 = below is element 0
    slots[s.j + 2] += s.f;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int sizes[] = {1, 2, 3, 63, 64, 65, 255, 256};
    for (int nv : sizes) {
        double *slots = new double[nv + 2]();                       // exactly the nv + 2 slots: one past is a report
        std::vector<double> ps = {nan, -nan, inf, -inf, 1e308, -1e308, 1e300, -1e300, 4294967296., -4294967296., 2147483648., -2147483649.,
                                  -1., -1. - 1e-16, std::nextafter(-1., 0.), -0.5, -0., 0., 5e-324, -5e-324, 0.5, 1., double(nv) - 1.,
                                  std::nextafter(double(nv) - 1., 0.), double(nv) - 0.5, double(nv), std::nextafter(double(nv), inf),
                                  std::nextafter(double(nv), 0.), double(nv) + 1., 1e9};
        for (int i = -2; i <= nv + 2; ++i) ps.push_back(double(i));
        for (double p : ps) deposit(slots, nv, p);
        double sum = 0.;
        for (int s = 0; s < nv + 2; ++s) sum += slots[s];
        EXPECT(std::fabs(sum - double(ps.size())) < 1e-9, "nv=%d: the weights sum to %.17g, not %zu", nv, sum, ps.size());
        delete[] slots;

        DSpectrumSlot s = dspectrum_slot(nan, nv);
        EXPECT(s.j == -1 && s.f == 0., "nv=%d: NaN lies in below", nv);
        s = dspectrum_slot(-inf, nv);
        EXPECT(s.j == -1 && s.f == 0., "nv=%d: -inf lies in below", nv);
        s = dspectrum_slot(-1e308, nv);
        EXPECT(s.j == -1 && s.f == 0., "nv=%d: -1e308 lies in below", nv);
        s = dspectrum_slot(-1., nv);
        EXPECT(s.j == -1 && s.f == 0., "nv=%d: -1 is below's centre", nv);
        s = dspectrum_slot(inf, nv);
        EXPECT(s.j == nv - 1 && s.f == 1., "nv=%d: +inf lies in above", nv);
        s = dspectrum_slot(1e308, nv);
        EXPECT(s.j == nv - 1 && s.f == 1., "nv=%d: 1e308 lies in above", nv);
        s = dspectrum_slot(double(nv), nv);
        EXPECT(s.j == nv - 1 && s.f == 1., "nv=%d: nv is above's centre", nv);
        s = dspectrum_slot(-0.25, nv);
        EXPECT(s.j == -1 && s.f == 0.75, "nv=%d: -0.25", nv);
        for (int i = 0; i < nv; ++i) {                               // an exact integer is a bin's centre: all of it in that bin
            s = dspectrum_slot(double(i), nv);
            EXPECT(s.j == i && s.f == 0., "nv=%d: p=%d gives j=%d f=%g", nv, i, s.j, s.f);
            s = dspectrum_slot(double(i) + 0.25, nv);
            EXPECT(s.j == i && s.f == 0.25, "nv=%d: p=%d.25 gives j=%d f=%g", nv, i, s.j, s.f);
        }
        // continuity: one ulp either side of a bin's centre moves an ulp of mass, never a bin
        for (int i = 0; i < nv; ++i) {
            const DSpectrumSlot lo = dspectrum_slot(std::nextafter(double(i), -inf), nv), hi = dspectrum_slot(std::nextafter(double(i), inf), nv);
            EXPECT(lo.j == i - 1 && 1. - lo.f < 1e-13 && hi.j == i && hi.f < 1e-13, "nv=%d: about %d", nv, i);
        }
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("slot ok\n");
    return 0;
}
