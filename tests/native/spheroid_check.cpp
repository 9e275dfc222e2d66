// spheroid_check.cpp -- kidmp::spheroid_shape / pol_moments / pol_spheroid / pol_bins (kid_amd/csrc/kidmp_spheroid.h), the
// per-particle model of the polarimetric radar, as a host program: built twice by tests/test_polarimetric_abi.py, with and
// without -fsanitize=address,undefined, and run there; the two outputs must be the same text.  Every number is printed as
// a hex float, so a difference of one bit shows, and tests/polarimetric_ref.py recomputes the lines.  The sweep: the shape
// factors of sixteen axis ratios on both sides of the series' switch ("l" lines), the moments of six canting widths ("a"
// lines), the rows of a unit spheroid for three permittivities, four ratios and three widths ("s" lines), then the seven
// rows of rain, snow and graupel on 24 diameters from 1e-6 to 0.05 m for the default and for a second configuration ("b"
// lines), then the sphere limit and what the header refuses.  Exit status 0 and the last line "spheroid ok" mean all held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kidmp_spheroid.h"

using namespace kidmp;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main()
{
    const double ratios[16] = {1., 0.9999999, 0.999, 0.9925, 0.99228, 0.99227, 0.992, 0.99, 0.95, 0.9, 0.75, 0.5, 0.2, 0.05, 1.5, 1e-3};
    for (double r : ratios) {
        const SpheroidShape s = spheroid_shape(r);
        EXPECT(s.La >= 1. / 3. && s.La < 1. && s.Lb > 0. && s.Lb <= 1. / 3., "shape r=%g: %g %g", r, s.La, s.Lb);
        std::printf("l %a %a %a\n", r, s.La, s.Lb);
    }
    const double sigmas[6] = {0., 1e-3, 0.17453292519943295, 0.6981317007977318, 3., 10.};
    for (double sg : sigmas) {
        const PolMoments m = pol_moments(sg);
        std::printf("a %a %a %a %a %a %a %a\n", sg, m.A1, m.A2, m.A3, m.A4, m.A5, m.A7);
    }
    const PolMoments m0 = pol_moments(0.);
    EXPECT(m0.A1 == 1. && m0.A2 == 0. && m0.A3 == 1. && m0.A4 == 0. && m0.A5 == 0. && m0.A7 == 1., "the moments at sigma = 0");
    const double eps[3][2] = {{79.5, 24.9}, {3.17, 0.01}, {1.3, 0.}};
    const double rs[4] = {1., 0.995, 0.8, 0.3}, sg3[3] = {0., 0.17453292519943295, 0.6981317007977318};
    for (const auto &e : eps)
        for (double r : rs)
            for (double sg : sg3) {
                double row[POL_ROWS - 1];
                pol_spheroid(BBComplex{e[0], e[1]}, r, pol_moments(sg), 1., row);
                std::printf("s %a %a %a %a %a %a %a %a %a %a\n", e[0], e[1], r, sg, row[0], row[1], row[2], row[3], row[4], row[5]);
                EXPECT(row[0] > 0. && row[1] > 0. && row[4] > 0. && row[5] >= 0., "rows eps=%g r=%g", e[0], r);
                if (r == 1.) {                                     // the sphere: the same bits, +0.0
                    EXPECT(!std::memcmp(&row[0], &row[1], 8) && !std::memcmp(&row[0], &row[2], 8) && !std::memcmp(&row[0], &row[4], 8), "sphere rows");
                    const double zero = 0.;
                    EXPECT(!std::memcmp(&row[3], &zero, 8) && !std::memcmp(&row[5], &zero, 8), "sphere zeros");
                }
            }
    const double k = std::sqrt(0.176);
    const MieCfg mcs[2] = {{0.10, {79.5, 24.9}, {(1. + 2. * k) / (1. - k), 0.}, 1000., 900., 0.93},
                           {0.055, {72.0, 35.0}, {3.17, 0.003}, 1000., 917., 0.93}};                 // illustrative values
    PolCfg pcs[2] = {pol_defaults(), pol_defaults()};
    pcs[1].axis_s = 0.6; pcs[1].axis_g = 1.; pcs[1].sigma[0] = 0.; pcs[1].sigma[1] = 0.3; pcs[1].axis_r_min = 0.5;
    const int nb = 24;
    std::vector<double> *D = new std::vector<double>(nb), *rows = new std::vector<double>(size_t(POL_ROWS) * nb);   // on the heap: what the sanitizer watches
    for (int i = 0; i < nb; ++i) (*D)[size_t(i)] = 1e-6 * std::pow(0.05 / 1e-6, i / double(nb - 1));
    for (int c = 0; c < 2; ++c)
        for (int sp = 0; sp < 3; ++sp) {
            EXPECT(pol_bins(mcs[c], pcs[c], sp, nb, D->data(), rows->data()), "bins refused cfg=%d sp=%d", c, sp);
            const double *r = rows->data();
            for (int b = 0; b < nb; ++b) {
                std::printf("b %d %d %a %a %a %a %a %a %a %a\n", c, sp, (*D)[size_t(b)], r[b], r[nb + b], r[2 * nb + b], r[3 * nb + b], r[4 * nb + b],
                            r[5 * nb + b], r[6 * nb + b]);
                EXPECT(r[b] > 0. && r[nb + b] > 0. && r[4 * nb + b] > 0. && r[5 * nb + b] >= 0. && r[6 * nb + b] > 0., "row cfg=%d sp=%d b=%d", c, sp, b);
            }
        }
    EXPECT(pol_uniform(MIE_GRAUPEL) && !pol_uniform(MIE_SNOW) && !pol_uniform(MIE_RAIN), "uniform");
    const double nan = std::nan(""), inf = HUGE_VAL;
    PolCfg bad = pol_defaults();
    EXPECT(!pol_bad_cfg(bad), "the defaults");
    bad.axis_s = 0.; EXPECT(pol_bad_cfg(bad) != nullptr, "axis_s = 0");
    bad = pol_defaults(); bad.axis_g = 1.5; EXPECT(pol_bad_cfg(bad) != nullptr, "axis_g > 1");
    bad = pol_defaults(); bad.axis_r_min = -0.1; EXPECT(pol_bad_cfg(bad) != nullptr, "r_min < 0");
    bad = pol_defaults(); bad.sigma[2] = -1e-9; EXPECT(pol_bad_cfg(bad) != nullptr, "sigma < 0");
    bad = pol_defaults(); bad.axis_r[3] = nan; EXPECT(pol_bad_cfg(bad) != nullptr, "nan");
    bad = pol_defaults(); bad.sigma[0] = inf; EXPECT(pol_bad_cfg(bad) != nullptr, "inf");
    (*D)[3] = 0.;
    EXPECT(!pol_bins(mcs[0], pcs[0], 0, nb, D->data(), rows->data()) && !pol_bins(mcs[0], pcs[0], 3, 1, D->data(), rows->data()), "bins");
    delete D;
    delete rows;
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("spheroid ok\n");
    return 0;
}
