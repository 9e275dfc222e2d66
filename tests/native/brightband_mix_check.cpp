// brightband_mix_check.cpp -- kidmp::bb_bin / kidmp::bb_wet (kid_amd/csrc/kidmp_brightband_mix.h), the per-particle
// dielectric model of the bright band, as a host program: built twice by tests/test_bright_band_abi.py, with and without
// -fsanitize=address,undefined, and run there; the two outputs must be the same text.  Every weight is printed as a hex
// float, so a difference of one bit shows.  The sweep: fm in {0.05, 0.5, 0.99}, both topologies, snow and graupel masses,
// D from 1e-6 to 0.3 m; then the guarded corner c = 0 (a particle with no ice and no air left) and the limits the header
// states.  Exit status 0 and the last line "mix ok" mean all held.
#include <cmath>
#include <cstdio>
#include <vector>

#include "kidmp_brightband_mix.h"

using namespace kidmp;

static int failures = 0;
static const double ULP = 2.220446049250313e-16;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static BBMix mix(double ew_re, double ew_im, int ice_matrix)
{
    const double k = std::sqrt(0.176), eps_i = (1. + 2. * k) / (1. - k);
    return BBMix{ew_re, ew_im, eps_i, bb_K_real(eps_i), 1000., 900., ice_matrix};
}

int main()
{
    const double PI = 3.1415926536, am_s = 0.069, am_g = PI * 500.0 / 6.0;
    const double fms[] = {0.05, 0.5, 0.99};
    std::vector<double> *weights = new std::vector<double>();       // on the heap: what the sanitizer watches
    for (int topo = 0; topo < 2; ++topo) {
        const BBMix x = mix(79.5, 24.9, topo), vac = mix(1., 0., topo);
        for (int sp = 0; sp < 2; ++sp)
            for (int i = 0; i <= 64; ++i) {
                const double D = 1e-6 * std::pow(0.3 / 1e-6, i / 64.);
                const double m = sp == 0 ? am_s * (D * D) : am_g * (D * D * D);
                const BBBin b = bb_bin(x, m, D);
                EXPECT(b.Vi0 > 0. && b.Ve >= b.Vi0 && b.dry > 0., "bin D=%g", D);
                for (double fm : fms) {
                    const double w = bb_wet(x, b, fm);
                    EXPECT(std::isfinite(w) && w > 0., "topo=%d sp=%d D=%g fm=%g: %g", topo, sp, D, fm, w);
                    weights->push_back(w);
                    std::printf("%d %d %a %a %a %a\n", topo, sp, D, fm, w, w / b.dry);
                    // The vacuum limit with water as the matrix: (1 - fm)**2 of the dry weight.  K(eps_p) is formed from
                    // eps_p - 1, which cancels: an ulp of eps_p is 1/(3 |K|) ulp of K, |K| = (1 - fm) K_i Vi0/V.  64 ulp over
                    // |K| bounds that.  (With the core as the matrix the limit is no identity: Maxwell-Garnett is not
                    // symmetric in matrix and inclusion; tests/test_bright_band_abi.py records by how much.)
                    const double v = bb_wet(vac, b, fm) / b.dry, lim = (1. - fm) * (1. - fm);
                    const double V = (1. - fm) * b.Ve + (fm * b.m) / x.rho_w, kmag = (1. - fm) * x.k_i * b.Vi0 / V;
                    if (topo == 0) EXPECT(std::fabs(v / lim - 1.) < 64 * ULP / kmag, "vacuum D=%g fm=%g: %.17g", D, fm, v / lim);
                    std::printf("v %a\n", v);
                }
                // fm = 0 is the dry particle in either topology; with water as the matrix eps_w*(1 + 2b)/(1 - b) returns to
                // eps_c through numbers of the size of |eps_w| = 83, so its ulp counts 83-fold in eps_p - 1
                const double w0 = bb_wet(x, b, 0.), k0 = x.k_i * b.Vi0 / b.Ve;
                EXPECT(std::fabs(w0 / b.dry - 1.) < 64 * 83 * ULP / k0, "fm=0 topo=%d D=%g: %.17g", topo, D, w0 / b.dry);
            }
        // c = 0: all ice melted and no air left (fm = 1 is outside the kernel's 0.99, the guard keeps it finite)
        const BBBin solid = bb_bin(x, 900. * (PI / 6.0) * 1e-9, 1e-3);
        const double w1 = bb_wet(x, solid, 1.);
        EXPECT(std::isfinite(w1) && w1 > 0., "c = 0: %g", w1);
        std::printf("c0 %d %a\n", topo, w1);
    }
    std::printf("%zu weights\n", weights->size());
    delete weights;
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("mix ok\n");
    return 0;
}
