// kidmp_scan.hip -- the entries of include/kidmp_scan.h: range-height scans of an x-z slab in one launch of k_scan.  The
// operator is stated operation by operation in that header; the classification of a gate centre is kidmp_scan_geom.h,
// shared with the host.  Built with the library's plain flags (IEEE division, no contraction): every operation below
// rounds once.
#include <cmath>

#include "kidmp_ctx.h"
#include "kidmp_wave.h"
#include "kidmp_scan_geom.h"
#include "fastmath.h"
#include "../../include/kidmp_scan.h"

using namespace kidmp;
using namespace kidmp::wave;

static_assert(sizeof(kidmp_scan_out) == 6 * sizeof(void *) && sizeof(kidmp32_scan_out) == 6 * sizeof(void *)
                  && sizeof(kidmp_scan_cfg) == 6 * sizeof(double) && KIDMP_SCAN_MAX_SUB <= 64 && sizeof(scan::Ray) == scan::RAY_WORDS * sizeof(double),
              "include/kidmp_scan.h");

namespace {
constexpr int SCAN_WAVES = 4;                            // rays (wavefronts) per workgroup
constexpr int SCAN_THREADS = 64 * SCAN_WAVES;
constexpr int SCAN_NOUT = 5;                             // dbz, dbz_att, pia, vr, height
enum { O_DBZ, O_ATT, O_PIA, O_VR, O_HEIGHT };
constexpr double LN10 = 2.302585092994045684;
constexpr double SCAN_PIA = 20. / LN10;                  // two-way dB per unit of one-way optical depth, kidmp_mie.h's c
constexpr double DB_TO_LN = LN10 / 10., LN_TO_DB = 10. / LN10;
constexpr double SMALLEST_NORMAL = 2.2250738585072014e-308;

template <class T> struct ScanArgs {
    const T *dbz, *ext, *vd, *u;                         // ext, vd, u null: zero
    const double *zf, *rays;
    T *out[SCAN_NOUT];                                   // null: not wanted
    int32_t *cell;
    scan::Grid g;
    double missing;
    int64_t nray;
    int32_t ngate, nsub, shared_flow, steps;             // steps: scan::level_steps(nz)
};

// E and L of the header: fastmath's exp and ln with the ends of their domains closed
__device__ inline double lin_of(double t) { return t > -700. ? fm::exp(fmin(t, 700.)) : 0.; }
__device__ inline double db_of(double q) { return q >= SMALLEST_NORMAL ? LN_TO_DB * fm::log(q) : -double(__builtin_inf()); }

// One wavefront per output ray, four rays per workgroup, lanes over gates: gate g = 64 gg + lane of gate group gg.  The
// groups are walked in a loop and the sub-rays in an inner loop of the same wave: neighbouring sub-rays hit mostly the
// same cells, so what the first one pulled in the others find in the cache.  zf is staged once per workgroup in LDS and the
// level is found by scan::level_of, whose trip count is wave-uniform.  Every gather index is formed from a sample that
// scan::sample judged inside.  The path is column_depths' upward scan with gates in place of levels (wave_prefix_sum, then
// a carry per sub-ray from one gate group to the next); the nsub carries are wave-uniform and live in the lanes 0 .. nsub-1
// of ONE register pair (v_readlane with the sub-ray's index, a masked move back), so that the sub-ray loop needs no
// array and no scratch.  BEAM = false (nsub == 1) is the pass-through: no transcendental, no table, no weight.  The only
// barrier is the one behind the staging; a wave without a ray leaves after it.  No atomics.
template <class T, bool BEAM>
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan(const ScanArgs<T> a)
{
    __shared__ double s_zf[KIDMP_MAX_NZ + 1];
    const int tid = int(threadIdx.x), lane = tid & 63;
    const int nz = a.g.nz, nx = a.g.nx;
    for (int t = tid; t <= nz; t += SCAN_THREADS) s_zf[t] = a.zf[t];
    if (BEAM) fm::tab::load_tables(tid, SCAN_THREADS);
    __syncthreads();
    const int64_t ray = int64_t(blockIdx.x) * SCAN_WAVES + __builtin_amdgcn_readfirstlane(tid >> 6);
    if (ray >= a.nray) return;

    const int nsub = BEAM ? a.nsub : 1, centre = nsub / 2;
    const double *__restrict__ rows = a.rays + ray * int64_t(nsub) * scan::RAY_WORDS;
    const double *zf = s_zf;
    const T missing = T(a.missing);
    const int ngroup = (a.ngate + 63) >> 6;
    double carry = 0.;                                               // lane j: the optical depth of sub-ray j before this group
    for (int gg = 0; gg < ngroup; ++gg) {
        const int gate = 64 * gg + lane;
        const bool live = gate < a.ngate;
        double Sz = 0., Sa = 0., Sv = 0., W = 0.;                    // BEAM: sum z, sum z', sum z'*v, sum wgt
        int hits = 0;
        double o_dbz = 0., o_att = 0., o_pia = 0., o_vr = 0., height = double(__builtin_nan(""));
        int32_t cell = -1;
        for (int j = 0; j < nsub; ++j) {
            const double *__restrict__ w = rows + j * scan::RAY_WORDS;
            const scan::Ray r{w[0], w[1], w[2], w[3], w[4], w[5]};
            const bool ok = scan::ray_valid(r, a.g.nslab);           // wave-uniform
            const scan::Sample sm = scan::sample(r, a.g, zf, a.steps, gate);
            const bool in = ok && live && sm.inside;
            double d = 0., av = 0., v = 0.;
            int64_t idx = -1;
            if (in) {
                const int64_t col = int64_t(r.slab) * nx + sm.i;
                idx = col * nz + sm.k;
                d = double(a.dbz[idx]);
                if (a.ext) av = double(a.ext[idx]) * a.g.dr;
                double uc = 0., vd = 0.;
                if (a.u) {
                    const int ir = sm.i + 1 < nx ? sm.i + 1 : 0;
                    const int64_t c0 = a.shared_flow ? int64_t(sm.i) : col, c1 = a.shared_flow ? int64_t(ir) : col - sm.i + ir;
                    uc = 0.5 * (double(a.u[c0 * nz + sm.k]) + double(a.u[c1 * nz + sm.k]));
                }
                if (a.vd) vd = double(a.vd[idx]);
                v = uc * r.ce - vd * r.se;
            }
            double tau = 0.;
            if (a.ext) {                                             // whole wavefronts: lanes past ngate hold +0.0
                double total;
                const double below = __shfl_up(wave_prefix_sum<false>(av, lane, total), 1, 64);
                const double c = readlane(carry, j);
                tau = (c + (lane > 0 ? below : 0.)) + 0.5 * av;
                if (lane == j) carry = c + total;
            }
            const double p = SCAN_PIA * tau, e = d - p;
            if (j == centre) {
                if (ok) height = sm.h;
                if (in) cell = int32_t(idx);
            }
            if (BEAM) {
                if (in) {
                    const double z = r.wgt * lin_of(DB_TO_LN * d), za = r.wgt * lin_of(DB_TO_LN * e);
                    Sz += z;
                    Sa += za;
                    Sv += za * v;
                    W += r.wgt;
                    ++hits;
                }
            } else if (in) {
                o_dbz = d; o_att = e; o_pia = p; o_vr = v;
                hits = 1;
            }
        }
        if (!live) continue;
        if (BEAM && hits) {
            o_dbz = db_of(Sz / W);
            o_att = db_of(Sa / W);
            o_pia = o_dbz - o_att;
            o_vr = Sa > 0. ? Sv / Sa : 0.;
        }
        const int64_t o = ray * a.ngate + gate;
        if (a.out[O_DBZ]) a.out[O_DBZ][o] = hits ? T(o_dbz) : missing;
        if (a.out[O_ATT]) a.out[O_ATT][o] = hits ? T(o_att) : missing;
        if (a.out[O_PIA]) a.out[O_PIA][o] = hits ? T(o_pia) : missing;
        if (a.out[O_VR]) a.out[O_VR][o] = hits ? T(o_vr) : missing;
        if (a.out[O_HEIGHT]) a.out[O_HEIGHT][o] = T(height);
        if (a.cell) a.cell[o] = cell;
    }
}

template <class T, class O>
int scan_device(kidmp_ctx *ctx, const char *who, int64_t nslab, int32_t nx, int32_t nz, double dx, const T *dbz, const T *ext, const T *vd,
                const T *u, int32_t shared_flow, const double *zf, const double *rays, int64_t nray, const kidmp_scan_cfg *cfg, const O *out,
                void *stream)
{
    const std::string me(who);
    if (int rc = require_ready(ctx)) return rc;
    if (nx < 1) return fail(ctx, KIDMP_EINVAL, me + ": nx < 1");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, me + ": nz outside [2, KIDMP_MAX_NZ]");
    if (nslab < 0) return fail(ctx, KIDMP_EINVAL, me + ": nslab < 0");
    if (nslab > int64_t(0x7fffffff) / nx) return fail(ctx, KIDMP_EINVAL, me + ": more columns than one launch takes");
    if (nray < 0 || nray > int64_t(0x7fffffff)) return fail(ctx, KIDMP_EINVAL, me + ": nray outside [0, 0x7fffffff]");
    if (!(dx > 0.) || !std::isfinite(dx)) return fail(ctx, KIDMP_EINVAL, me + ": dx must be finite and > 0");
    if (!cfg || !out) return fail(ctx, KIDMP_EINVAL, me + ": null argument (cfg and out are required)");
    if (cfg->ngate < 1 || cfg->ngate > KIDMP_SCAN_MAX_GATES) return fail(ctx, KIDMP_EINVAL, me + ": ngate outside [1, KIDMP_SCAN_MAX_GATES]");
    if (cfg->nsub < 1 || cfg->nsub > KIDMP_SCAN_MAX_SUB) return fail(ctx, KIDMP_EINVAL, me + ": nsub outside [1, KIDMP_SCAN_MAX_SUB]");
    if (!(cfg->dr > 0.) || !std::isfinite(cfg->dr)) return fail(ctx, KIDMP_EINVAL, me + ": dr must be finite and > 0");
    if (!(cfg->r0 >= 0.) || !std::isfinite(cfg->r0)) return fail(ctx, KIDMP_EINVAL, me + ": r0 must be finite and >= 0");
    if (!std::isfinite(cfg->half_inv_ae)) return fail(ctx, KIDMP_EINVAL, me + ": half_inv_ae must be finite");
    ScanArgs<T> a{};
    T *const wanted[SCAN_NOUT] = {out->dbz, out->dbz_att, out->pia, out->vr, out->height};
    bool any = out->cell != nullptr;
    for (int v = 0; v < SCAN_NOUT; ++v) { a.out[v] = wanted[v]; any = any || wanted[v]; }
    if (!any) return fail(ctx, KIDMP_EINVAL, me + ": nothing requested: every member of out is null");
    if (out->vr && !vd && !u) return fail(ctx, KIDMP_EINVAL, me + ": vr needs vd or u");
    if (out->cell && nslab * nx > int64_t(0x7fffffff) / nz) return fail(ctx, KIDMP_EINVAL, me + ": cell is 32 bits wide: nslab*nx*nz > 0x7fffffff");
    if (nray == 0 || nslab == 0) return KIDMP_OK;                    // an empty batch has nothing to point at
    if (!dbz || !zf || !rays) return fail(ctx, KIDMP_EINVAL, me + ": null argument (dbz, zf and rays are required)");
    GUARD(ctx);
    const void *ptrs[] = {dbz, ext, vd, u, zf, rays, out->dbz, out->dbz_att, out->pia, out->vr, out->height, out->cell};
    const char *what[] = {"dbz", "ext", "vd", "u", "zf", "rays", "out.dbz", "out.dbz_att", "out.pia", "out.vr", "out.height", "out.cell"};
    for (int i = 0; i < 12; ++i)
        if (int rc = check_device_array(ctx, who, ptrs[i], what[i])) return rc;
    a.dbz = dbz; a.ext = ext; a.vd = vd; a.u = u; a.zf = zf; a.rays = rays; a.cell = out->cell;
    a.g = scan::Grid{cfg->r0, cfg->dr, dx, cfg->half_inv_ae, nslab, nx, nz, cfg->periodic != 0};
    a.missing = cfg->missing;
    a.nray = nray; a.ngate = cfg->ngate; a.nsub = cfg->nsub; a.shared_flow = shared_flow != 0;
    a.steps = scan::level_steps(nz);
    const dim3 grid((unsigned)((nray + SCAN_WAVES - 1) / SCAN_WAVES)), block(SCAN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (a.nsub > 1) hipLaunchKernelGGL((k_scan<T, true>), grid, block, 0, st, a);
    else            hipLaunchKernelGGL((k_scan<T, false>), grid, block, 0, st, a);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}
}  // namespace

extern "C" {
int kidmp_scan_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dx, const double *dbz, const double *ext, const double *vd,
                      const double *u, int32_t shared_flow, const double *zf, const double *rays, int64_t nray, const kidmp_scan_cfg *cfg,
                      const kidmp_scan_out *out, void *stream)
{
    return scan_device<double>(ctx, "kidmp_scan_device", nslab, nx, nz, dx, dbz, ext, vd, u, shared_flow, zf, rays, nray, cfg, out, stream);
}
int kidmp32_scan_device(kidmp_ctx *ctx, int64_t nslab, int32_t nx, int32_t nz, double dx, const float *dbz, const float *ext, const float *vd,
                        const float *u, int32_t shared_flow, const double *zf, const double *rays, int64_t nray, const kidmp_scan_cfg *cfg,
                        const kidmp32_scan_out *out, void *stream)
{
    return scan_device<float>(ctx, "kidmp32_scan_device", nslab, nx, nz, dx, dbz, ext, vd, u, shared_flow, zf, rays, nray, cfg, out, stream);
}
}  // extern "C"
