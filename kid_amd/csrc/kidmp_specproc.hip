// kidmp_specproc.hip -- the entries of include/kidmp_specproc.h: broadening, noise floor, detection and moments of a
// Doppler spectrum in one launch of k_spectrum_process.  The operator is stated operation by operation in that header; the
// per-level window arithmetic is kidmp_specproc_window.h, shared with the host.  Built with the library's plain flags
// (IEEE division and square root, no contraction): every operation below rounds once.
#include <cmath>

#include "kidmp_ctx.h"
#include "kidmp_specproc_window.h"
#include "fastmath.h"
#include "../../include/kidmp_specproc.h"

using namespace kidmp;

static_assert(sizeof(kidmp_specproc_out) == 11 * sizeof(void *) && sizeof(kidmp32_specproc_out) == 11 * sizeof(void *)
                  && sizeof(kidmp_specproc_cfg) == 3 * sizeof(double) && KIDMP_SPECPROC_MAX_HALF == specproc::MAX_HALF,
              "include/kidmp_specproc.h");

namespace {
constexpr int SP_TJ = 8;                                 // output bins per tile of the velocity axis, held in registers
constexpr int SP_U = 8;                                  // steps of the offset per block (SP_U <= SP_TJ: the window moves by whole blocks)
constexpr int SP_WCAP = 16;                              // weights g_0 .. g_WCAP (and tails T_1 .. T_WCAP) of a lane are kept in LDS
constexpr int SP_NVAL = 9;                               // lost_below, lost_above, dbz, vm, sw, skew, kurt, v_lo, v_hi
enum { V_BELOW, V_ABOVE, V_DBZ, V_VM, V_SW, V_SKEW, V_KURT, V_LO, V_HI };

template <class T> struct SpecArgs {
    const T *spec, *sigma, *noise;                       // sigma, noise null: none
    T *ospec, *val[SP_NVAL];                             // null: not wanted
    int32_t *nbins;
    double v0, dv, inv_dv, cut, snr_min;
    int32_t nz, nv, sigma_stride, noise_stride, add_noise, ngroup;
};

// One tile walk of the velocity axis for one lane (= one level): use(j, B_j) for j = 0 .. nv-1 ascending.  The tile is
// SP_TJ output bins whose sums live in registers; the offset dd = i - j runs upward from -Hw, Hw the largest H of the wave,
// so the trip count is wave-uniform, and a lane whose own H is smaller masks the steps beyond it.  For bin j the source
// bin i = j + dd ascends with dd, which is the order the header states, whatever the tile.  The steps are taken in blocks
// of SP_U: a block's SP_TJ + SP_U source bins sit in registers under compile-time indices, its SP_U weights are read
// together, and the SP_U bins the NEXT block adds are requested before this block's sums begin, so that a load has a whole
// block of arithmetic to arrive in (one load per step consumed in the next step left the wave waiting on memory at every
// step: 2.6 times slower).  The steps past Hw that fill the last block are masked like any step beyond a
// lane's H.  Every load sits behind a test of its bin against 0 .. nv-1.  x points at the lane's value of bin 0; bins are nz
// values apart.  With Hw = 0 the walk hands the input through.
template <class T, class Weight, class Use>
__device__ __forceinline__ void walk_bins(const T *__restrict__ x, int nz, int nv, const specproc::Window &w, int Hw, double G, Weight &&gw, Use &&use)
{
    auto bin = [&](int i) { return (i >= 0 && i < nv) ? double(x[i * nz]) : 0.; };
    if (Hw == 0) {
        for (int j0 = 0; j0 < nv; j0 += SP_TJ) {
            double v[SP_TJ];
#pragma unroll
            for (int jj = 0; jj < SP_TJ; ++jj) v[jj] = bin(j0 + jj);
#pragma unroll
            for (int jj = 0; jj < SP_TJ; ++jj)
                if (j0 + jj < nv) use(j0 + jj, v[jj]);
        }
        return;
    }
    const int nblock = (2 * Hw + SP_U) / SP_U;                       // ceil((2 Hw + 1)/SP_U)
    for (int j0 = 0; j0 < nv; j0 += SP_TJ) {
        double acc[SP_TJ], xw[SP_TJ + SP_U], nxt[SP_U];
        const int base = j0 - Hw;                                    // the bin under xw[0] in block 0
#pragma unroll
        for (int jj = 0; jj < SP_TJ; ++jj) acc[jj] = 0.;
#pragma unroll
        for (int q = 0; q < SP_TJ + SP_U; ++q) xw[q] = bin(base + q);
        for (int b = 0; b < nblock; ++b) {
            const int dd0 = b * SP_U - Hw;                           // the offset of this block's first step
            double g[SP_U];
            bool on[SP_U];
#pragma unroll
            for (int u = 0; u < SP_U; ++u) {
                const int dd = dd0 + u, ad = dd < 0 ? -dd : dd;
                on[u] = ad <= w.H;
                g[u] = on[u] ? gw(ad) : 0.;
            }
#pragma unroll
            for (int u = 0; u < SP_U; ++u) nxt[u] = b + 1 < nblock ? bin(base + (b + 1) * SP_U + SP_TJ + u) : 0.;
#pragma unroll
            for (int u = 0; u < SP_U; ++u) {
#pragma unroll
                for (int jj = 0; jj < SP_TJ; ++jj) {
                    const int i = j0 + jj + dd0 + u;
                    const double sum = acc[jj] + g[u] * xw[jj + u];
                    acc[jj] = (on[u] && i >= 0 && i < nv) ? sum : acc[jj];
                }
            }
#pragma unroll
            for (int q = 0; q < SP_TJ; ++q) xw[q] = xw[q + SP_U];
#pragma unroll
            for (int u = 0; u < SP_U; ++u) xw[SP_TJ + u] = nxt[u];
        }
#pragma unroll
        for (int jj = 0; jj < SP_TJ; ++jj)
            if (j0 + jj < nv) use(j0 + jj, w.H > 0 ? acc[jj] / G : bin(j0 + jj));
    }
}

// One wavefront per (column, group of 64 levels), one wavefront per workgroup, lanes over levels: every row of the
// spectrum is read and written as one coalesced line.  A lane forms its weights once (specproc::norm) and keeps g_0 ..
// g_WCAP in its own column of an LDS table; a weight beyond WCAP is formed again where it is used (the same function
// of the same arguments: the same bits), which only windows wider than 2*WCAP + 1 bins pay (and which is cheaper than the occupancy a longer table costs: DESIGN 4.5r).  LOST adds the table of the
// tails.  A lane past nz shadows level nz-1 and stores nothing, so that no load needs a test of its own.  The moments take
// a second walk for the central sums, only when sw, skew or kurt is wanted.  No atomics, no scratch; the only barrier is the
// one behind the math tables.
template <class T, bool LOST>
__global__ void __launch_bounds__(64)
k_spectrum_process(const SpecArgs<T> a)
{
    __shared__ double s_g[(SP_WCAP + 1) * 64];
    __shared__ double s_t[LOST ? (SP_WCAP + 1) * 64 : 64];
    const int lane = int(threadIdx.x);
    fm::tab::load_tables(lane, 64);
    __syncthreads();
    const int nz = a.nz, nv = a.nv;
    const int64_t c = int64_t(blockIdx.x) / a.ngroup;
    const int gg = int(int64_t(blockIdx.x) - c * a.ngroup);
    const int k = 64 * gg + lane;
    const bool live = k < nz;
    const int kk = live ? k : nz - 1;
    const double sig = a.sigma ? double(a.sigma[c * a.sigma_stride + kk]) : 0.;
    const double nk = a.noise ? double(a.noise[c * a.noise_stride + kk]) : 0.;
    const specproc::Window w = specproc::window(sig, a.inv_dv, a.cut);
    int Hw = w.H;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int other = __shfl_xor(Hw, off, 64);
        Hw = other > Hw ? other : Hw;
    }
    Hw = __builtin_amdgcn_readfirstlane(Hw);

    s_g[lane] = 1.;
    const double G = specproc::norm(w, [&](int d, double g) { if (d <= SP_WCAP) s_g[d * 64 + lane] = g; });
    auto gw = [&](int d) { return d <= SP_WCAP ? s_g[d * 64 + lane] : specproc::weight(d, w.s); };   // 0 <= d <= w.H
    const T *__restrict__ x = a.spec + (c * nv) * nz + kk;
    const int64_t o = c * nz + k;

    if (LOST) {
        specproc::tails(w, gw, [&](int m, double t) { if (m <= SP_WCAP) s_t[m * 64 + lane] = t; });
        auto tw = [&](int m) {                                                                      // 1 <= m <= w.H
            if (m <= SP_WCAP) return s_t[m * 64 + lane];
            double t = 0.;
            for (int d = w.H; d >= m; --d) t += gw(d);
            return t;
        };
        double below = 0., above = 0.;
        if (w.H > 0) {
            const int nb = w.H < nv ? w.H : nv;
            if (a.val[V_BELOW]) {
                for (int i = 0; i < nb; ++i) below += double(x[i * nz]) * tw(i + 1);
                below = below / G;
            }
            if (a.val[V_ABOVE]) {
                for (int i = nv - nb; i < nv; ++i) above += double(x[i * nz]) * tw(nv - i);
                above = above / G;
            }
        }
        if (live && a.val[V_BELOW]) a.val[V_BELOW][o] = T(below);
        if (live && a.val[V_ABOVE]) a.val[V_ABOVE][o] = T(above);
    }

    const bool central = a.val[V_SW] || a.val[V_SKEW] || a.val[V_KURT];
    const bool moments = central || a.val[V_DBZ] || a.val[V_VM] || a.val[V_LO] || a.val[V_HI] || a.nbins;
    if (!moments && !a.ospec) return;

    const double thr = specproc::threshold(a.snr_min, nk);
    double z = 0., m1 = 0., v_lo = 0., v_hi = 0.;
    int nb = 0;
    T *const os = a.ospec ? a.ospec + (c * nv) * nz + kk : nullptr;
    walk_bins(x, nz, nv, w, Hw, G, gw, [&](int j, double B) {
        if (os && live) os[j * nz] = a.add_noise ? T(B + nk) : T(B);
        if (moments && specproc::detected(B, thr)) {
            const double v = a.v0 + double(j) * a.dv;
            z += B;
            m1 += v * B;
            if (nb == 0) v_lo = v;
            v_hi = v;
            ++nb;
        }
    });
    if (!moments) return;
    double vm = nb > 0 ? m1 / z : 0.;
    vm = vm < v_lo ? v_lo : (vm > v_hi ? v_hi : vm);                 // the quotient of two rounded sums can leave [v_lo, v_hi] by an ulp
    double sw = 0., skew = 0., kurt = 0.;
    if (central) {
        double c2 = 0., c3 = 0., c4 = 0.;
        walk_bins(x, nz, nv, w, Hw, G, gw, [&](int j, double B) {
            if (specproc::detected(B, thr)) {
                const double e = (a.v0 + double(j) * a.dv) - vm;
                const double q = e * e;
                c2 += q * B;
                c3 += (q * e) * B;
                c4 += (q * q) * B;
            }
        });
        if (nb > 0) {
            const double var = c2 / z;
            sw = var > 0. ? sqrt(var) : 0.;
            if (sw != 0.) {
                skew = (c3 / z) / ((sw * sw) * sw);
                kurt = (c4 / z) / ((sw * sw) * (sw * sw));
            }
        }
    }
    if (!live) return;
    if (a.val[V_DBZ]) a.val[V_DBZ][o] = T(nb > 0 ? 10. * fm::log10((z > 1e-22 ? z : 1e-22) * 1e18) : -40.);
    if (a.val[V_VM]) a.val[V_VM][o] = T(vm);
    if (a.val[V_SW]) a.val[V_SW][o] = T(sw);
    if (a.val[V_SKEW]) a.val[V_SKEW][o] = T(skew);
    if (a.val[V_KURT]) a.val[V_KURT][o] = T(kurt);
    if (a.val[V_LO]) a.val[V_LO][o] = T(v_lo);
    if (a.val[V_HI]) a.val[V_HI][o] = T(v_hi);
    if (a.nbins) a.nbins[o] = nb;
}

template <class T, class O>
int specproc_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const T *spec, double v0, double dv, int32_t nv, const T *sigma,
                    int32_t sigma_stride, const T *noise, int32_t noise_stride, const kidmp_specproc_cfg *cfg, const O *out, void *stream)
{
    const std::string me(who);
    if (int rc = require_ready(ctx)) return rc;
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, me + ": nz outside [2, KIDMP_MAX_NZ]");
    const int32_t ngroup = (nz + 63) / 64;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, me + ": ncol < 0");
    if (ncol > int64_t(0x7fffffff) / ngroup) return fail(ctx, KIDMP_EINVAL, me + ": more columns than one launch takes");
    if (nv < 1 || nv > KIDMP_SPECPROC_MAX_NV) return fail(ctx, KIDMP_EINVAL, me + ": nv outside [1, KIDMP_SPECPROC_MAX_NV]");
    if (!(dv > 0.) || !std::isfinite(dv) || !std::isfinite(1. / dv)) return fail(ctx, KIDMP_EINVAL, me + ": dv must be finite and above 0");
    if (!std::isfinite(v0)) return fail(ctx, KIDMP_EINVAL, me + ": v0 must be finite");
    if (!cfg || !out) return fail(ctx, KIDMP_EINVAL, me + ": null argument (cfg and out are required)");
    if (!(cfg->cut > 0.) || !std::isfinite(cfg->cut)) return fail(ctx, KIDMP_EINVAL, me + ": cut must be finite and above 0");
    if (!(cfg->snr_min >= 0.) || !std::isfinite(cfg->snr_min)) return fail(ctx, KIDMP_EINVAL, me + ": snr_min must be finite and not below 0");
    if (sigma_stride != 0 && sigma_stride != nz) return fail(ctx, KIDMP_EINVAL, me + ": sigma_stride must be 0 or nz");
    if (noise_stride != 0 && noise_stride != nz) return fail(ctx, KIDMP_EINVAL, me + ": noise_stride must be 0 or nz");
    SpecArgs<T> a{};
    T *const wanted[SP_NVAL] = {out->lost_below, out->lost_above, out->dbz, out->vm, out->sw, out->skew, out->kurt, out->v_lo, out->v_hi};
    bool any = out->spec != nullptr || out->nbins != nullptr;
    for (int v = 0; v < SP_NVAL; ++v) { a.val[v] = wanted[v]; any = any || wanted[v]; }
    if (!any) return fail(ctx, KIDMP_EINVAL, me + ": nothing requested: every member of out is null");
    if (ncol == 0) return KIDMP_OK;                                  // an empty batch has nothing to point at
    if (!spec) return fail(ctx, KIDMP_EINVAL, me + ": null argument (spec is required)");
    GUARD(ctx);
    const void *ptrs[] = {spec, sigma, noise, out->spec, out->lost_below, out->lost_above, out->dbz, out->vm, out->sw, out->skew, out->kurt,
                          out->v_lo, out->v_hi, out->nbins};
    const char *what[] = {"spec", "sigma", "noise", "out.spec", "out.lost_below", "out.lost_above", "out.dbz", "out.vm", "out.sw", "out.skew",
                          "out.kurt", "out.v_lo", "out.v_hi", "out.nbins"};
    for (int i = 0; i < 14; ++i)
        if (int rc = check_device_array(ctx, who, ptrs[i], what[i])) return rc;
    a.spec = spec; a.sigma = sigma; a.noise = noise; a.ospec = out->spec; a.nbins = out->nbins;
    a.v0 = v0; a.dv = dv; a.inv_dv = 1. / dv; a.cut = cfg->cut; a.snr_min = cfg->snr_min;
    a.nz = nz; a.nv = nv; a.sigma_stride = sigma_stride; a.noise_stride = noise_stride; a.add_noise = cfg->add_noise != 0; a.ngroup = ngroup;
    const dim3 grid((unsigned)(ncol * ngroup)), block(64);
    hipStream_t st = (hipStream_t)stream;
    if (out->lost_below || out->lost_above) hipLaunchKernelGGL((k_spectrum_process<T, true>), grid, block, 0, st, a);
    else                                    hipLaunchKernelGGL((k_spectrum_process<T, false>), grid, block, 0, st, a);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}
}  // namespace

extern "C" {
int kidmp_spectrum_process_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *spec, double v0, double dv, int32_t nv, const double *sigma,
                                  int32_t sigma_stride, const double *noise, int32_t noise_stride, const kidmp_specproc_cfg *cfg,
                                  const kidmp_specproc_out *out, void *stream)
{
    return specproc_device<double>(ctx, "kidmp_spectrum_process_device", ncol, nz, spec, v0, dv, nv, sigma, sigma_stride, noise, noise_stride, cfg,
                                   out, stream);
}
int kidmp32_spectrum_process_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *spec, double v0, double dv, int32_t nv, const float *sigma,
                                    int32_t sigma_stride, const float *noise, int32_t noise_stride, const kidmp_specproc_cfg *cfg,
                                    const kidmp32_specproc_out *out, void *stream)
{
    return specproc_device<float>(ctx, "kidmp32_spectrum_process_device", ncol, nz, spec, v0, dv, nv, sigma, sigma_stride, noise, noise_stride, cfg,
                                  out, stream);
}
}  // extern "C"
