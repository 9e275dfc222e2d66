// kidmp_dspectrum.hip -- the entries of include/kidmp_dspectrum.h: the Doppler spectrum of device arrays in one launch of
// k_doppler_spectrum (below), and of host arrays in chunks through the context's staging memory.
#include <cmath>
#include <cstddef>

#include "kidmp_ctx.h"
#include "../../include/kidmp_dspectrum.h"

#include "kidmp_dspectrum_slot.h"
#include "kidmp_column.h"

namespace kidmp {

// The Doppler spectrum (include/kidmp_dspectrum.h): the reflectivity of every level on a uniform velocity grid, from
// k_doppler_moments' load.  Null means: qs, qg -- zero; w -- zero; an output -- not wanted.  out: total, rain, snow,
// graupel [ncol][nv][nz], below, above [ncol][nz].  D, dD: device arrays of nb[x] doubles by species rain, snow, graupel.
// idv = 1/dv.  One launch; the velocity axis is walked in tiles of DSPECTRUM_TILE slots held in LDS.
// (-DKIDMP_DSPECTRUM_TILE=n builds another tile for tools/bench_doppler_spectrum.py --lib; the results do not depend on it)
#ifndef KIDMP_DSPECTRUM_TILE
#define KIDMP_DSPECTRUM_TILE 24
#endif
constexpr int DSPECTRUM_NOUT = 6, DSPECTRUM_NSPEC = 3, DSPECTRUM_TILE = KIDMP_DSPECTRUM_TILE, DSPECTRUM_MAX_NV = 256;
static_assert(DSPECTRUM_TILE >= 2 && DSPECTRUM_TILE <= 30, "four waves' tiles and the fastmath tables share 64 KiB of LDS");
template <class T> struct DSpectrumArgs {
    const T *t, *p, *qv, *qr, *nr, *qs, *qg, *w;
    T *out[DSPECTRUM_NOUT];
    const double *D[DSPECTRUM_NSPEC], *dD[DSPECTRUM_NSPEC];
    int32_t nb[DSPECTRUM_NSPEC];
    double v0, idv;
    int32_t nv;
};

// ---- the Doppler spectrum (include/kidmp_dspectrum.h) ----
// what a level keeps for its bins: the three species' factors of lvl::exp_echo / lvl::snow_echo_bin
struct EchoLevel {
    double rhof, w, n0r, lamr, n0g, lamg;
    lvl::SnowEcho s;
    bool pr, ps, pg;
};

// One species' bins of one level group into the slots [t0, t1) of the wave's tile, `acc` laid out [slot - t0][lane]:
// every lane owns a column of the tile, so no two lanes meet and the order of the additions to a slot is the order of
// the bins.  Slots are counted from `below` = 0: slot s holds velocity bin s - 1, slot nv + 1 is `above`.
// What depends on the bin alone is formed once per bin, 64 bins at a time and one per lane, and handed round with
// v_readlane.  Each of those lanes also bounds the slots its bin can reach at any level of the group, from the group's
// extremes of rhof and w: the position (rhof*vfac - w - v0)*idv is monotone in rhof and in w under rounding, so the bound
// holds exactly, and a bin that cannot reach the tile is passed over before its exponential.  The bound only prunes;
// whether a lane deposits is decided by its own slot, so the result does not depend on the tile.
template <int SP, class T>
__device__ __forceinline__ void deposit_species(double *__restrict__ acc, int t0, int t1, const EchoLevel &L, bool present,
                                                const DSpectrumArgs<T> &a, int lane)
{
    if (!__ballot(present)) return;
    const double inf = double(__builtin_inf());
    const bool wild = __ballot(present && !(fabs(L.rhof) < inf && fabs(L.w) < inf)) != 0;   // NaN or infinite: no bound
    const double rmin = wave_min(present ? L.rhof : inf), rmax = wave_max(present ? L.rhof : -inf);
    const double wmin = wave_min(present ? L.w : inf), wmax = wave_max(present ? L.w : -inf);
    const double *__restrict__ D = a.D[SP], *__restrict__ dD = a.dD[SP];
    const int nb = a.nb[SP], nv = a.nv, top = nv + 1;
    for (int bb = 0; bb < nb; bb += 64) {
        double mD = 0., mG = 0., mV = 0., mMu = 0.;
        bool reach = false;
        if (bb + lane < nb) {
            mD = D[bb + lane];
            const double dDb = dD[bb + lane];
            if (SP == 0) { mG = lvl::pw6_times(mD, dDb); mV = lvl::rain_bin_speed(mD); }
            if (SP == 1) { mG = lvl::pw4_times(mD, dDb); mV = lvl::snow_bin_speed(mD); mMu = fm::pow(mD, mu_s); }
            if (SP == 2) { mG = lvl::pw6_times(mD, dDb); mV = lvl::graupel_bin_speed(mD); }
            int lo = 0, hi = top;
            if (!wild && mV >= 0.) {
                lo = dspectrum_slot((rmin * mV - wmax - a.v0) * a.idv, nv).j + 1;
                hi = dspectrum_slot((rmax * mV - wmin - a.v0) * a.idv, nv).j + 2;
            }
            reach = hi >= t0 && lo < t1;
        }
        unsigned long long hit = __ballot(reach);
        while (hit) {
            const int b = __builtin_ctzll(hit);
            hit &= hit - 1;
            const double Db = readlane(mD, b), Gb = readlane(mG, b), Vb = readlane(mV, b);
            const double Dmu = SP == 1 ? readlane(mMu, b) : 0.;
            const DSpectrumSlot s = dspectrum_slot((L.rhof * Vb - L.w - a.v0) * a.idv, nv);
            const int s0 = s.j + 1, s1 = s.j + 2;                    // 0 .. nv, 1 .. nv + 1
            const bool in0 = s0 >= t0 && s0 < t1, in1 = s1 >= t0 && s1 < t1;
            if (present && (in0 || in1)) {
                double z = 0.;
                if (SP == 0) z = lvl::exp_echo(L.n0r, L.lamr, Db, Gb);
                if (SP == 1) z = lvl::snow_echo_bin(L.s, Db, Dmu, Gb);
                if (SP == 2) z = lvl::exp_echo(L.n0g, L.lamg, Db, Gb);
                if (in0) acc[(s0 - t0) * 64 + lane] += (1. - s.f) * z;
                if (in1) acc[(s1 - t0) * 64 + lane] += s.f * z;
            }
        }
    }
}

// One wavefront per column: the Doppler spectrum of every level (include/kidmp_dspectrum.h).  The load and the scan are
// k_doppler_moments' (radar_level, graupel_running_min); every level keeps the factors of its three species in registers.
// Then, per level group and per requested spectrum (total with below and above, rain, snow, graupel: one pass each), the
// nv + 2 slots are walked in tiles of DSPECTRUM_TILE: the tile's accumulators are a lane-private column in LDS, zeroed,
// filled species by species in the order rain, snow, graupel with the bins ascending, and written out as one row store
// per velocity bin.  No atomics; a slot's additions come in one order whatever the tile, the pass and the grid.
template <class T, int NJ>
__global__ void __launch_bounds__(REFL_THREADS)
k_doppler_spectrum(ReflConsts c, DopplerConsts dc, DSpectrumArgs<T> a, int64_t ncol, int nz)
{
    __shared__ double s_acc[REFL_WAVES][DSPECTRUM_TILE * 64];
    int lane;
    const int64_t col = enter_column(lane);
    if (col >= ncol) return;                                         // whole wavefronts only: the scans need every lane
    const int64_t base = col * int64_t(nz);
    double *__restrict__ acc = s_acc[int(threadIdx.x) >> 6];

    EchoLevel lv[NJ];
    double rg[NJ], n0[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 64 * j + lane;
        lv[j] = EchoLevel{};
        rg[j] = R1;
        n0[j] = double(__builtin_inf());                             // levels past kte do not enter the minimum
        if (k >= nz) continue;
        const int64_t i = base + k;
        const RadarLevel r = radar_level(c, a, i);
        lv[j].rhof = r.rhof;
        lv[j].pr = r.L_qr; lv[j].ps = r.L_qs; lv[j].pg = r.L_qg;
        if (r.L_qr || r.L_qs || r.L_qg) lv[j].w = a.w ? double(a.w[i]) : 0.;     // a level with no species: w is not read
        lv[j].n0r = r.N0_r; lv[j].lamr = r.lamr;
        if (r.L_qs) lv[j].s = lvl::snow_echo(dc, r.ze_snow, lvl::snow_mrat(c, dc, r.sl));
        rg[j] = r.rg;
        n0[j] = r.n0_exp;
    }
    graupel_running_min<NJ>(n0, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (!lv[j].pg) continue;
        double ilamg, N0_g;
        lvl::graupel_ze(c, n0[j], rg[j], ilamg, lv[j].lamg, N0_g);
        lv[j].n0g = lvl::ZE_GRAUPEL_FAC * N0_g;
    }

    const int nv = a.nv, nslot = nv + 2;
    for (int j = 0; j < NJ; ++j) {
        EchoLevel L = lv[0];
#pragma unroll
        for (int jj = 1; jj < NJ; ++jj)
            if (j == jj) L = lv[jj];
        const int k = 64 * j + lane;
        for (int pass = 0; pass < 4; ++pass) {
            const bool edges = pass == 0 && (a.out[4] || a.out[5]);
            T *__restrict__ spec = a.out[pass];
            if (!spec && !edges) continue;
            for (int t0 = 0; t0 < nslot; t0 += DSPECTRUM_TILE) {
                const int t1 = t0 + DSPECTRUM_TILE < nslot ? t0 + DSPECTRUM_TILE : nslot;
                if (!spec && t0 > 0 && t1 < nslot) continue;         // below and above alone: the first and the last tile
                for (int s = 0; s < t1 - t0; ++s) acc[s * 64 + lane] = 0.;
                if (pass == 0 || pass == 1) deposit_species<0, T>(acc, t0, t1, L, L.pr, a, lane);
                if (pass == 0 || pass == 2) deposit_species<1, T>(acc, t0, t1, L, L.ps, a, lane);
                if (pass == 0 || pass == 3) deposit_species<2, T>(acc, t0, t1, L, L.pg, a, lane);
                if (k < nz)
                    for (int s = t0; s < t1; ++s) {
                        const double v = acc[(s - t0) * 64 + lane];
                        if (s == 0) { if (edges && a.out[4]) a.out[4][base + k] = T(v); }
                        else if (s == nslot - 1) { if (edges && a.out[5]) a.out[5][base + k] = T(v); }
                        else if (spec) spec[(col * int64_t(nv) + (s - 1)) * int64_t(nz) + k] = T(v);
                    }
            }
        }
    }
}

namespace {
template <class T>
hipError_t launch_doppler_spectrum(const ReflConsts &c, const DopplerConsts &dc, int64_t ncol, int nz, const DSpectrumArgs<T> &a, hipStream_t s)
{
    if (ncol <= 0) return hipSuccess;                                // an empty batch is not looked at
    if (a.nv < 1 || a.nv > DSPECTRUM_MAX_NV) return hipErrorInvalidValue;
    return launch_level_groups(ncol, nz, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        hipLaunchKernelGGL((k_doppler_spectrum<T, NJ>), column_grid(ncol), dim3(REFL_THREADS), 0, s, c, dc, a, ncol, nz);
    });
}
}  // namespace

}  // namespace kidmp

using namespace kidmp;

static_assert(sizeof(kidmp_dspectrum_out) == DSPECTRUM_NOUT * sizeof(double *) && sizeof(kidmp32_dspectrum_out) == DSPECTRUM_NOUT * sizeof(float *)
                  && DSPECTRUM_NSPEC == KIDMP_DSPECTRUM_NSPECIES && DSPECTRUM_MAX_NV == KIDMP_DSPECTRUM_MAX_NV && nbins <= KIDMP_DSPECTRUM_MAX_BINS,
              "include/kidmp_dspectrum.h");

namespace {
constexpr int NIN = 8, NREQ = 5, NSPECTRA = 4;            // t, p, qv, qr, nr | qs, qg, w;  total, rain, snow, graupel | below, above
const char *const IN_NAMES[NIN] = {"t", "p", "qv", "qr", "nr", "qs", "qg", "w"};
const char *const OUT_NAMES[DSPECTRUM_NOUT] = {"total", "rain", "snow", "graupel", "below", "above"};
constexpr size_t MAX_STAGE = size_t(256) << 20;           // the host entries' staging: chunks are sized to stay below it

// the scheme's own grid of a species inside a Bins (host or device copy alike): rain, snow, graupel
const double *bins_D(const Bins *b, int x) { return x == 0 ? b->Dr : x == 1 ? b->Ds : b->Dg; }
const double *bins_dD(const Bins *b, int x) { return x == 0 ? b->dtr : x == 1 ? b->dts : b->dtg; }

template <class T> struct DSpectrumCall {
    const T *in[NIN];
    T *out[DSPECTRUM_NOUT];
    const double *D[DSPECTRUM_NSPEC], *dD[DSPECTRUM_NSPEC];   // the caller's; both null: the scheme's own
    int32_t nb[DSPECTRUM_NSPEC];
    double v0, dv;
    int32_t nv;
};
template <class T, class O>
DSpectrumCall<T> dspectrum_call(const T *t, const T *p, const T *qv, const T *qr, const T *nr, const T *qs, const T *qg, const T *w,
                                double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const O *out)
{
    DSpectrumCall<T> c{{t, p, qv, qr, nr, qs, qg, w}, {}, {}, {}, {}, v0, dv, nv};
    if (out) {
        T *const o[DSPECTRUM_NOUT] = {out->total, out->rain, out->snow, out->graupel, out->below, out->above};
        for (int v = 0; v < DSPECTRUM_NOUT; ++v) c.out[v] = o[v];
    }
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        c.nb[x] = nbins;
        if (grids && (grids->D[x] || grids->dD[x])) { c.D[x] = grids->D[x]; c.dD[x] = grids->dD[x]; c.nb[x] = grids->nb[x]; }
    }
    return c;
}

// what the device and the host entries check alike, before anything is touched
template <class T>
int check_dspectrum(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DSpectrumCall<T> &a)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (ncol < 0) return fail(ctx, KIDMP_EINVAL, w + ": ncol < 0");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (a.nv < 1 || a.nv > KIDMP_DSPECTRUM_MAX_NV) return fail(ctx, KIDMP_EINVAL, w + ": nv outside [1, KIDMP_DSPECTRUM_MAX_NV]");
    if (!(a.dv > 0.) || !std::isfinite(a.dv) || !std::isfinite(1. / a.dv)) return fail(ctx, KIDMP_EINVAL, w + ": dv must be finite and above 0");
    if (!std::isfinite(a.v0)) return fail(ctx, KIDMP_EINVAL, w + ": v0 must be finite");
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        if ((a.D[x] == nullptr) != (a.dD[x] == nullptr)) return fail(ctx, KIDMP_EINVAL, w + ": a grid needs both D and dD");
        if (a.nb[x] < 1 || a.nb[x] > KIDMP_DSPECTRUM_MAX_BINS) return fail(ctx, KIDMP_EINVAL, w + ": nb outside [1, KIDMP_DSPECTRUM_MAX_BINS]");
    }
    if (ncol == 0) return KIDMP_OK;                       // an empty batch has nothing to point at
    bool any = false;
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) any = any || a.out[v];
    if (!any) return fail(ctx, KIDMP_EINVAL, w + ": nothing requested: out is NULL or every member is");
    for (int v = 0; v < NREQ; ++v)
        if (!a.in[v]) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    if (!doppler_consts_supported(ctx->hc) || !spectra_consts_supported(ctx->hc))
        return fail(ctx, KIDMP_ESTATE, w + ": exponents differ from the kernel's");
    return KIDMP_OK;
}

// one launch over device pointers
template <class T>
hipError_t enqueue_dspectrum(kidmp_ctx *ctx, int64_t ncol, int nz, const DSpectrumCall<T> &a, hipStream_t s)
{
    const T *const *q = a.in;
    DSpectrumArgs<T> args{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], {}, {}, {}, {}, a.v0, 1. / a.dv, a.nv};
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) args.out[v] = a.out[v];
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        args.D[x] = a.D[x] ? a.D[x] : bins_D(ctx->d_bins, x);
        args.dD[x] = a.dD[x] ? a.dD[x] : bins_dD(ctx->d_bins, x);
        args.nb[x] = a.D[x] ? a.nb[x] : nbins;
    }
    return launch_doppler_spectrum<T>(refl_consts(ctx->hc), doppler_consts(ctx->hc), ncol, nz, args, s);
}

template <class T>
int dspectrum_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DSpectrumCall<T> &a, void *stream)
{
    if (int rc = check_dspectrum<T>(ctx, who, ncol, nz, a)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    for (int v = 0; v < NIN; ++v)
        if (int rc = check_device_array(ctx, who, a.in[v], IN_NAMES[v])) return rc;
    for (int v = 0; v < DSPECTRUM_NOUT; ++v)
        if (int rc = check_device_array(ctx, who, a.out[v], OUT_NAMES[v])) return rc;
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        if (int rc = check_device_array(ctx, who, a.D[x], "D")) return rc;
        if (int rc = check_device_array(ctx, who, a.dD[x], "dD")) return rc;
    }
    HIPTRY(ctx, enqueue_dspectrum<T>(ctx, ncol, nz, a, (hipStream_t)stream));
    return KIDMP_OK;
}

// host arrays: stage_run of kidmp_host.hip, the chunk narrowed to stay below MAX_STAGE.  The caller's grids go up once,
// only the inputs given go up per chunk and only what was asked for comes down.
template <class T>
int dspectrum_host(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const DSpectrumCall<T> &h)
{
    if (int rc = check_dspectrum<T>(ctx, who, ncol, nz, h)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    constexpr int A_D = 0, A_DD = DSPECTRUM_NSPEC, A_IN = 2 * DSPECTRUM_NSPEC, A_OUT = A_IN + NIN;
    StageArray a[A_OUT + DSPECTRUM_NOUT];
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        a[A_D + x] = stage_once(h.D[x], h.nb[x]);
        a[A_DD + x] = stage_once(h.dD[x], h.nb[x]);
    }
    for (int v = 0; v < NIN; ++v) a[A_IN + v] = stage_array(h.in[v], nz, STAGE_UP);
    for (int v = 0; v < DSPECTRUM_NOUT; ++v)                  // the spectra have nv profiles of nz values per column
        a[A_OUT + v] = stage_array(h.out[v], int64_t(v < NSPECTRA ? h.nv : 1) * nz, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol), MAX_STAGE);
    if (int rc = stage_open(ctx, plan)) return rc;
    DSpectrumCall<T> d{};
    d.v0 = h.v0; d.dv = h.dv; d.nv = h.nv;
    for (int x = 0; x < DSPECTRUM_NSPEC; ++x) {
        d.nb[x] = h.nb[x];
        d.D[x] = staged<double>(a[A_D + x]);
        d.dD[x] = staged<double>(a[A_DD + x]);
    }
    for (int v = 0; v < NIN; ++v) d.in[v] = staged<T>(a[A_IN + v]);
    for (int v = 0; v < DSPECTRUM_NOUT; ++v) d.out[v] = staged<T>(a[A_OUT + v]);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) { return enqueue_dspectrum<T>(ctx, n, nz, d, ctx->stream); });
}
}  // namespace

extern "C" {
int kidmp_doppler_spectrum_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                  const double *qr, const double *nr, const double *qs, const double *qg, const double *w,
                                  double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp_dspectrum_out *out,
                                  void *stream)
{
    return dspectrum_device<double>(ctx, "kidmp_doppler_spectrum_device", ncol, nz,
                                    dspectrum_call<double>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out), stream);
}
int kidmp32_doppler_spectrum_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                    const float *qr, const float *nr, const float *qs, const float *qg, const float *w,
                                    double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp32_dspectrum_out *out,
                                    void *stream)
{
    return dspectrum_device<float>(ctx, "kidmp32_doppler_spectrum_device", ncol, nz,
                                   dspectrum_call<float>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out), stream);
}
int kidmp_doppler_spectrum_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p, const double *qv,
                                const double *qr, const double *nr, const double *qs, const double *qg, const double *w,
                                double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp_dspectrum_out *out)
{
    return dspectrum_host<double>(ctx, "kidmp_doppler_spectrum_host", ncol, nz,
                                  dspectrum_call<double>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out));
}
int kidmp32_doppler_spectrum_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p, const float *qv,
                                  const float *qr, const float *nr, const float *qs, const float *qg, const float *w,
                                  double v0, double dv, int32_t nv, const kidmp_dspectrum_grids *grids, const kidmp32_dspectrum_out *out)
{
    return dspectrum_host<float>(ctx, "kidmp32_doppler_spectrum_host", ncol, nz,
                                 dspectrum_call<float>(t, p, qv, qr, nr, qs, qg, w, v0, dv, nv, grids, out));
}
}  // extern "C"
