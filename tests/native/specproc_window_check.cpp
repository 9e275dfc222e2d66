// specproc_window_check.cpp -- kidmp::specproc::window / weight / norm / tails / detected
// (kid_amd/csrc/kidmp_specproc_window.h), the per-level window arithmetic of the spectrum processor, as a host program:
// built twice by tests/test_specproc_abi.py, with and without -fsanitize=address,undefined, and run there on the cases
// that test wrote (argv[1]); the two outputs must be the same text, and tests/specproc_ref.py's H, s and detection mask
// must equal them to the bit, its weights, norm and tails to the rounding of the two exponentials.  Every number goes in
// and out as a hex float.  The weights and tails of a level live on the heap at their exact size H + 1, so an index
// outside 0 .. H is an error the sanitizer reports.
//
// Input, whitespace separated: ncase, then per case  inv_dv cut snr_min nsig npair  sigma[nsig]  (B, noise)[npair].
// Output per case "c <index>", per sigma "w <H> <s> <G>", then "g <d> <g_d>" for d = 1 .. H ascending and "t <m> <T_m>" for
// m = H .. 1 descending; per pair "d <0|1>".  Exit status 0 and the last line "specproc ok" mean all held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kidmp_specproc_window.h"

using namespace kidmp;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool next(std::FILE *f, double &v)
{
    char tok[128];
    if (std::fscanf(f, "%127s", tok) != 1) return false;
    char *end = nullptr;
    v = std::strtod(tok, &end);
    return end != tok && *end == 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: specproc_window_check CASES\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    double v = 0.;
    if (!next(f, v)) return 2;
    const int ncase = int(v);
    for (int c = 0; c < ncase; ++c) {
        double head[5];
        for (double &h : head)
            if (!next(f, h)) return 2;
        const double inv_dv = head[0], cut = head[1], snr_min = head[2];
        const int nsig = int(head[3]), npair = int(head[4]);
        std::printf("c %d\n", c);
        for (int n = 0; n < nsig; ++n) {
            double sigma;
            if (!next(f, sigma)) return 2;
            const specproc::Window w = specproc::window(sigma, inv_dv, cut);
            EXPECT(w.H >= 0 && w.H <= specproc::MAX_HALF, "case %d sigma %d: H = %d", c, n, w.H);
            EXPECT(sigma > 0. || w.H == 0, "case %d sigma %d: H = %d without a positive sigma", c, n, w.H);
            std::vector<double> *g = new std::vector<double>(size_t(w.H) + 1), *t = new std::vector<double>(size_t(w.H) + 1);
            (*g)[0] = 1.;
            const double G = specproc::norm(w, [&](int d, double gd) { g->at(size_t(d)) = gd; });
            specproc::tails(w, [&](int d) { return g->at(size_t(d)); }, [&](int m, double tm) { t->at(size_t(m)) = tm; });
            std::printf("w %d %a %a\n", w.H, w.s, G);
            for (int d = 1; d <= w.H; ++d) {
                EXPECT((*g)[size_t(d)] >= 0. && (*g)[size_t(d)] <= 1., "case %d sigma %d: g_%d = %a", c, n, d, (*g)[size_t(d)]);
                EXPECT(d == 1 || (*g)[size_t(d)] <= (*g)[size_t(d) - 1], "case %d sigma %d: g_%d above g_%d", c, n, d, d - 1);
                std::printf("g %d %a\n", d, (*g)[size_t(d)]);
            }
            for (int m = w.H; m >= 1; --m) std::printf("t %d %a\n", m, (*t)[size_t(m)]);
            EXPECT(w.H == 0 || (G >= 1. && G <= 2. * w.H + 1.), "case %d sigma %d: G = %a", c, n, G);
            EXPECT(w.H > 0 || G == 1., "case %d sigma %d: G = %a with H = 0", c, n, G);
            delete g;
            delete t;
        }
        for (int n = 0; n < npair; ++n) {
            double B, noise;
            if (!next(f, B) || !next(f, noise)) return 2;
            std::printf("d %d\n", int(specproc::detected(B, specproc::threshold(snr_min, noise))));
        }
    }
    std::fclose(f);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("specproc ok\n");
    return 0;
}
