// mie_sphere_check.cpp -- kidmp::mie_sphere / kidmp::mie_bins (kid_amd/csrc/kidmp_mie_sphere.h), the per-particle model
// of the cloud radar, as a host program: built twice by tests/test_mie_abi.py, with and without
// -fsanitize=address,undefined, and run there; the two outputs must be the same text.  Every number is printed as a hex
// float, so a difference of one bit shows, and tests/mie_ref.py recomputes the lines.  The sweep: four refractive indices
// at ten size parameters from 1e-3 to 49 ("q" lines), then the five rows of rain, snow and graupel on 24 diameters from
// 1e-6 to 0.05 m at 3.19 mm and at 10 cm ("b" lines), then what the header refuses.  Exit status 0 and the last line
// "mie ok" mean all held.
#include <cmath>
#include <cstdio>
#include <vector>

#include "kidmp_mie_sphere.h"

using namespace kidmp;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main()
{
    const double ms[4][2] = {{3.0, 1.7}, {8.9, 1.4}, {1.3, 0.002}, {1.78, 0.003}};
    const double xs[10] = {1e-3, 0.01, 0.1, 0.5, 1., 2., 5., 10., 20., 49.};
    for (const auto &m : ms)
        for (double x : xs) {
            double qe = 0., qb = 0.;
            EXPECT(mie_sphere(x, m[0], m[1], qe, qb), "refused x=%g", x);
            EXPECT(std::isfinite(qe) && std::isfinite(qb) && qe > 0. && qb > 0., "x=%g m=%g+%gi: %g %g", x, m[0], m[1], qe, qb);
            std::printf("q %a %a %a %a %a\n", x, m[0], m[1], qe, qb);
        }
    const double k = std::sqrt(0.176);
    const MieCfg cfgs[2] = {{3.19e-3, {7.7, 14.2}, {3.17, 0.01}, 1000., 917., 0.75},          // illustrative W-band values
                            {0.10, {79.5, 24.9}, {(1. + 2. * k) / (1. - k), 0.}, 1000., 900., 0.93}};
    const int nb = 24;
    std::vector<double> *D = new std::vector<double>(nb), *rows = new std::vector<double>(size_t(MIE_ROWS) * nb);   // on the heap: what the sanitizer watches
    for (int i = 0; i < nb; ++i) (*D)[size_t(i)] = 1e-6 * std::pow(0.05 / 1e-6, i / double(nb - 1));
    for (int c = 0; c < 2; ++c)
        for (int sp = 0; sp < 3; ++sp) {
            EXPECT(mie_bins(cfgs[c], sp, nb, D->data(), rows->data()), "bins refused cfg=%d sp=%d", c, sp);
            for (int b = 0; b < nb; ++b) {
                const double *r = rows->data();
                std::printf("b %d %d %a %a %a %a %a %a\n", c, sp, (*D)[size_t(b)], r[b], r[nb + b], r[2 * nb + b], r[3 * nb + b], r[4 * nb + b]);
                EXPECT(r[b] > 0. && r[nb + b] > 0. && r[2 * nb + b] >= 0. && r[3 * nb + b] > 0. && r[4 * nb + b] > 0., "row cfg=%d sp=%d b=%d", c, sp, b);
            }
        }
    double qe = -1., qb = -1.;
    const double nan = std::nan(""), inf = HUGE_VAL;
    EXPECT(!mie_sphere(0., 1.3, 0., qe, qb) && !mie_sphere(-1., 1.3, 0., qe, qb) && !mie_sphere(nan, 1.3, 0., qe, qb), "x");
    EXPECT(!mie_sphere(1., 0., 0., qe, qb) && !mie_sphere(1., 1.3, -0.1, qe, qb) && !mie_sphere(1., inf, 0., qe, qb), "m");
    EXPECT(!mie_sphere(1e9, 1.3, 0., qe, qb) && !mie_sphere(inf, 1.3, 0., qe, qb), "terms");
    EXPECT(qe == -1. && qb == -1., "a refusal wrote");
    (*D)[3] = 0.;
    EXPECT(!mie_bins(cfgs[0], 0, nb, D->data(), rows->data()) && !mie_bins(cfgs[0], 3, 1, D->data(), rows->data()), "bins");
    delete D;
    delete rows;
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("mie ok\n");
    return 0;
}
