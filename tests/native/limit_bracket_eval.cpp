// Host evaluation of kid_amd/csrc/limit_bracket.h (no GPU), the counterpart of KIDMP_MATH_LIMIT_BRACKET's bracket half.
//   limit_bracket_eval consts            prints the header's constants, and num at each site's number floor, as hexadecimal
//                                        floats, one "name value" per line
//   limit_bracket_eval IN OUT            IN: int64 n, then num[n], den[n], site[n] as raw doubles (site 0: ice, 1: rain,
//                                        2 .. 15: cloud droplets with nu = site).  OUT: n int32: decide()'s answer (0 below,
//                                        1 inside, 2 above, 3 ambiguous) + 4 * certainly_inside()
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "limit_bracket.h"
#include "thompson_host_init.h"

namespace lb = kidmp::lb;

// decide() + 4 * certainly_inside()
static int answer(double num, double den, int site)
{
    if (site == 0) return lb::decide(num, den, lb::F_ICE) + 4 * lb::certainly_inside(num, den, lb::F_ICE);
    if (site == 1) return lb::decide(num, den, lb::F_RAIN) + 4 * lb::certainly_inside(num, den, lb::F_RAIN);
    const double c = lb::cloud_c(site);
    return lb::decide_scaled(num, den, c * c * c, lb::F_CLOUD) + 4 * lb::certainly_inside_scaled(num, den, c * c * c, lb::F_CLOUD);
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "consts")) {
        const lb::Site s[3] = {lb::SITE_ICE, lb::SITE_RAIN, lb::SITE_CLOUD};
        const char *name[3] = {"ice", "rain", "cloud"};
        for (int i = 0; i < 3; ++i) printf("%s_c %a\n%s_D_lo %a\n%s_D_hi %a\n", name[i], s[i].c, name[i], s[i].D_lo, name[i], s[i].D_hi);
        for (int nu = 2; nu <= 15; ++nu) printf("cloud_c_%d %a\n", nu, lb::cloud_c(nu));
        printf("E_X %a\nBOUND %a\nEPS %a\nLIM_TINY %a\nLIM_HUGE %a\n", lb::E_X, lb::BOUND, lb::EPS, lb::LIM_TINY, lb::LIM_HUGE);
        printf("R1 %a\nR2 %a\n", kidmp::R1, kidmp::R2);
        // num at the number floors, formed as the column kernel forms it (left to right) from the library's own host init:
        // n = R2 for ice and rain (fmax(R2, ...)), n = 2. for the droplets (fmax(2., ...))
        static kidmp::Consts c;
        static kidmp::Bins b;
        kidmp::host_init(0, 1, 100.0, c, b);
        printf("floor_num_0 %a\n", kidmp::am_i * c.cig[1] * c.oig1 * kidmp::R2);
        printf("floor_num_1 %a\n", kidmp::am_r * c.crg[2] * c.org2 * kidmp::R2);
        for (int nu = 2; nu <= 15; ++nu) printf("floor_num_%d %a\n", nu, 2. * kidmp::am_r * c.ccg[1][nu - 1] * c.ocg1[nu - 1]);
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: limit_bracket_eval consts | IN OUT\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    int64_t n;
    if (!f || fread(&n, sizeof n, 1, f) != 1 || n < 0) return 1;
    std::vector<double> num(n), den(n), site(n);
    for (std::vector<double> *v : {&num, &den, &site})
        if (n && fread(v->data(), sizeof(double), size_t(n), f) != size_t(n)) return 1;
    fclose(f);
    std::vector<int32_t> out(n);
    for (int64_t i = 0; i < n; ++i) {
        if (!(site[i] >= 0. && site[i] <= 15.)) return 2;
        out[i] = answer(num[i], den[i], int(site[i]));
    }
    f = fopen(argv[2], "wb");
    if (!f || (n && fwrite(out.data(), sizeof(int32_t), size_t(n), f) != size_t(n)) || fclose(f) != 0) return 1;
    return 0;
}
