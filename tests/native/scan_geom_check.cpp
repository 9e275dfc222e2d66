// scan_geom_check.cpp -- kidmp::scan::sample / ray_valid (kid_amd/csrc/kidmp_scan_geom.h), the classification that guards
// every gather of the range-height scan, as a host program: built twice by tests/test_scan_abi.py, with and without
// -fsanitize=address,undefined, and run there on the cases that test wrote (argv[1]); the two outputs must be the same
// text and equal tests/scan_ref.py's (i, k, h) to the bit.  Every number goes in and out as a hex float.  zf lives on the
// heap at its exact size, so a face index outside [0, nz] is an error the sanitizer reports.
//
// Input, whitespace separated:  ncase, then per case  nz nx nslab ngate periodic nrow  r0 dr dx half_inv_ae  zf[nz+1]
// rows[nrow][6].  Output per case "c <index>", per row "r <valid>", per gate "g <i> <k> <inside> <h>".  After the cases the
// program feeds sample() faces that do not ascend and faces of NaN and checks only that every answer names a cell.
// Exit status 0 and the last line "scan ok" mean all held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kidmp_scan_geom.h"

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
    if (argc != 2) { std::printf("usage: scan_geom_check CASES\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    double v = 0.;
    if (!next(f, v)) return 2;
    const int ncase = int(v);
    for (int c = 0; c < ncase; ++c) {
        double head[10];
        for (double &h : head)
            if (!next(f, h)) return 2;
        const int nz = int(head[0]), ngate = int(head[3]), nrow = int(head[5]);
        scan::Grid g{head[6], head[7], head[8], head[9], int64_t(head[2]), int32_t(head[1]), int32_t(nz), int32_t(head[4])};
        std::vector<double> *zf = new std::vector<double>(size_t(nz) + 1);
        for (double &z : *zf)
            if (!next(f, z)) return 2;
        const double *faces = zf->data();
        const int steps = scan::level_steps(nz);
        EXPECT((1 << steps) > nz && (steps == 0 || (1 << (steps - 1)) <= nz), "level_steps(%d) = %d", nz, steps);
        std::printf("c %d\n", c);
        for (int r = 0; r < nrow; ++r) {
            double w[scan::RAY_WORDS];
            for (double &x : w)
                if (!next(f, x)) return 2;
            const scan::Ray ray{w[0], w[1], w[2], w[3], w[4], w[5]};
            std::printf("r %d\n", int(scan::ray_valid(ray, g.nslab)));
            for (int gate = 0; gate < ngate; ++gate) {
                const scan::Sample s = scan::sample(ray, g, faces, steps, gate);
                EXPECT(s.inside ? (s.i >= 0 && s.i < g.nx && s.k >= 0 && s.k < nz) : (s.i == -1 && s.k == -1), "case %d row %d gate %d: (%d, %d)", c, r,
                       gate, s.i, s.k);
                EXPECT(!s.inside || (faces[s.k] <= s.h && s.h < faces[s.k + 1]), "case %d row %d gate %d: h outside its level", c, r, gate);
                std::printf("g %d %d %d %a\n", s.i, s.k, int(s.inside), s.h);
            }
        }
        delete zf;
    }
    std::fclose(f);
    // faces that no caller should pass: descending, constant, NaN, infinite.  Whatever comes out names a cell or nothing.
    const double nan = std::nan(""), inf = HUGE_VAL;
    for (int nz : {2, 3, 64, 65, 255, 256}) {
        const int steps = scan::level_steps(nz);
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<double> *zf = new std::vector<double>(size_t(nz) + 1);
            for (int k = 0; k <= nz; ++k)
                (*zf)[size_t(k)] = kind == 0 ? double(nz - k) : kind == 1 ? 5. : kind == 2 ? nan : kind == 3 ? (k % 2 ? inf : -inf) : ((k * 7919) % 13) * 100.;
            (*zf)[0] = kind == 2 ? nan : -1.;
            (*zf)[size_t(nz)] = kind == 2 ? nan : 1e9;
            const scan::Grid g{0., 50., 100., 0., 1, 5, int32_t(nz), 1};
            const scan::Ray ray{0., 10., 0., 0.6, 0.8, 1.};
            for (int gate = 0; gate < 64; ++gate) {
                const scan::Sample s = scan::sample(ray, g, zf->data(), steps, gate);
                EXPECT(s.inside ? (s.i >= 0 && s.i < g.nx && s.k >= 0 && s.k < nz) : (s.i == -1 && s.k == -1), "bad faces %d nz %d gate %d", kind, nz, gate);
            }
            delete zf;
        }
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("scan ok\n");
    return 0;
}
