// radiometer_check.cpp -- the host side of the radiometer (include/kidmp_radiometer.h) as a host program: the sphere's four
// efficiencies (kid_amd/csrc/kidmp_mie_sphere.h) and the two-stream layer with the adding of layers
// (kid_amd/csrc/kidmp_radiometer_layer.h, the functions the kernel calls).  Built twice by tests/test_radiometer_abi.py,
// with and without -fsanitize=address,undefined, and run there; the two outputs must be the same text.  Every number is
// printed as a hex float, so a difference of one bit shows, and tests/radiometer_ref.py recomputes the lines.  The sweep:
// four refractive indices at ten size parameters ("q" lines: x, m, Q_ext, Q_sca, Q_back, g); the layer at a list of
// (ta, b, mu, t) that takes every branch ("l" lines: ta, b, mu, t, e, f, R, T, a), with e = exp(-y) and f = -expm1(-y) of
// the host libm; combine on every ordered pair of them ("c" lines: i, j and the five numbers), and the identity on both
// sides of each.  Exit status 0 and the last line "radiometer ok" mean all held.
#include <cmath>
#include <cstdio>
#include <vector>

#include "kidmp_mie_sphere.h"
#include "kidmp_radiometer_layer.h"

using namespace kidmp;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same(const RadState &a, const RadState &b) { return a.Rt == b.Rt && a.Rb == b.Rb && a.T == b.T && a.Eu == b.Eu && a.Ed == b.Ed; }

int main()
{
    const double ms[4][2] = {{3.0, 1.7}, {8.9, 1.4}, {1.3, 0.002}, {1.78, 0.003}};
    const double xs[10] = {1e-3, 0.01, 0.1, 0.5, 1., 2., 5., 10., 20., 49.};
    for (const auto &m : ms)
        for (double x : xs) {
            MieEff e{};
            double qe = 0., qb = 0.;
            EXPECT(mie_efficiencies(x, m[0], m[1], e) && mie_sphere(x, m[0], m[1], qe, qb), "refused x=%g", x);
            EXPECT(e.qext == qe && e.qback == qb, "x=%g: Q_ext, Q_back are not mie_sphere's", x);
            // (g may be negative: a sphere of high index near its magnetic dipole resonance scatters backwards)
            EXPECT(e.qsca > 0. && e.qsca <= e.qext && e.g > -1. && e.g < 1.,"x=%g m=%g+%gi: %g %g %g", x, m[0], m[1], e.qext, e.qsca, e.g);
            std::printf("q %a %a %a %a %a %a %a\n", x, m[0], m[1], e.qext, e.qsca, e.qback, e.g);
        }
    // ta, b, mu, t: identity, conservative, b = 0 (Schwarzschild), ta tiny beside b, thin, thick, y beyond 700
    const double cases[][4] = {{0., 0., 1., 250.}, {0., 0.3, 0.6, 260.}, {0., 1e-9, 1., 270.}, {0.2, 0., 0.5, 280.}, {3., 0., 1., 255.},
                               {1e-300, 1., 0.7, 265.}, {1e-12, 1e-3, 1., 240.}, {1e-6, 1e-6, 0.3, 230.}, {0.05, 0.4, 0.6, 275.},
                               {2., 5., 1., 268.}, {40., 10., 0.9, 290.}, {800., 0., 1., 300.}, {500., 300., 0.4, 285.}, {1e5, 1e6, 1., 273.15}};
    const int n = int(sizeof(cases) / sizeof(cases[0]));
    std::vector<RadState> *st = new std::vector<RadState>();        // on the heap: what the sanitizer watches
    for (int i = 0; i < n; ++i) {
        const double ta = cases[i][0], b = cases[i][1], mu = cases[i][2], t = cases[i][3];
        const double x = rad_layer_x(ta, b), y = x / mu;
        const double e = std::exp(-y), f = -std::expm1(-y);
        const RadLayer l = rad_layer(ta, b, x, mu, e, f);
        EXPECT(l.R >= 0. && l.T >= 0. && l.a >= 0. && l.R <= 1. && l.T <= 1. && l.a <= 1., "layer %d: %g %g %g", i, l.R, l.T, l.a);
        EXPECT(std::fabs((l.R + l.T + l.a) - 1.) <= 4. * 2.220446049250313e-16, "layer %d: R + T + a = 1 + %g", i, (l.R + l.T + l.a) - 1.);
        std::printf("l %a %a %a %a %a %a %a %a %a\n", ta, b, mu, t, e, f, l.R, l.T, l.a);
        st->push_back(rad_state(l, t));
    }
    const RadState id = rad_identity();
    for (int i = 0; i < n; ++i) {
        EXPECT(same(rad_combine((*st)[size_t(i)], id), (*st)[size_t(i)]) && same(rad_combine(id, (*st)[size_t(i)]), (*st)[size_t(i)]), "identity %d", i);
        for (int j = 0; j < n; ++j) {
            const RadState c = rad_combine((*st)[size_t(i)], (*st)[size_t(j)]);
            EXPECT(std::isfinite(c.Rt) && std::isfinite(c.Rb) && std::isfinite(c.T) && std::isfinite(c.Eu) && std::isfinite(c.Ed), "combine %d %d", i, j);
            std::printf("c %d %d %a %a %a %a %a\n", i, j, c.Rt, c.Rb, c.T, c.Eu, c.Ed);
        }
    }
    delete st;
    MieEff e{-1., -1., -1., -1., -1.};
    EXPECT(!mie_efficiencies(0., 1.3, 0., e) && !mie_efficiencies(1., 1.3, -0.1, e) && !mie_efficiencies(1e9, 1.3, 0., e) && e.qsca == -1. && e.g == -1.,
           "a refusal wrote");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("radiometer ok\n");
    return 0;
}
