// kidmp_stats.hip -- per-level ensemble statistics (include/kidmp_stats.h): the moments and histograms of [ncol][nz]
// device arrays over the columns, per level and per ensemble group.  Two launches on the caller's stream: a partial
// pass that writes one slab per column chunk into the workspace and a combine pass that reads the slabs in index
// order.  No global atomics, no float atomics, no hand-off between workgroups: the store-and-sum form, so that every
// result is reproducible bit for bit for a given (ncol, nz, grouping).
#include "kidmp_ctx.h"
#include "../../include/kidmp_stats.h"

#include <cfloat>
#include <cmath>

using namespace kidmp;

namespace {
constexpr int STATS_CHUNKS = 256;      // kidmp_stats_chunks: at most one chunk per compute unit
constexpr int STATS_TILE = 64;         // levels per workgroup = one wave: thread k owns level k0 + k
constexpr int STATS_UNROLL = 4;        // columns whose loads are in flight together
constexpr int STATS_HSTRIDE = (KIDMP_STATS_MAX_BINS + 3) | 1;   // widest histogram row in 32-bit words, odd
constexpr int64_t STATS_MAX_NCOL = int64_t(1) << 39;            // a chunk's 32-bit histogram counts cannot overflow below this
static_assert(STATS_TILE * STATS_HSTRIDE * 4 + (KIDMP_STATS_MAX_BINS + 1) * 8 <= 65536, "static LDS of k_stats_part");

struct Moments { double n, mean, m2, mn, mx; };
__host__ __device__ inline Moments empty_moments() { return {0., 0., 0., HUGE_VAL, -HUGE_VAL}; }

// Chan's pairwise update, a <- a + b; an empty side is the identity.  The one formula of the combine pass and of
// kidmp_stats_merge (this file is built without FMA contraction: host and device round alike).
__host__ __device__ inline void chan_merge(Moments &a, const Moments &b)
{
    if (b.n == 0.) return;
    if (a.n == 0.) { a = b; return; }
    const double n = a.n + b.n, d = b.mean - a.mean;
    a.mean = a.mean + d * (b.n / n);
    a.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / n);
    a.mn = fmin(a.mn, b.mn);
    a.mx = fmax(a.mx, b.mx);
    a.n = n;
}

struct StatsArgs {
    const void *field[KIDMP_STATS_MAX_FIELDS];
    int64_t stride[KIDMP_STATS_MAX_FIELDS];
    double floor[KIDMP_STATS_MAX_FIELDS];
    const int32_t *group;
    const double *edges;
    double *pm;                        // [chunk][cell][NMOM][nz]
    uint32_t *ph;                      // [chunk][cell][nz][nbin+3]
    int64_t ncol, per;                 // chunk j: columns [j*per, min((j+1)*per, ncol))
    int32_t nz, nfield, nbin;
};

// Partial pass.  grid = (chunks in use, ngroup*nfield, level tiles of STATS_TILE), one wave per workgroup.  Lanes run over
// the vertical (k fastest: a column is one contiguous run), the workgroup loops over the columns of its chunk and skips
// those of other groups (only the 4-byte ids are read by every group).  The running moments of a level live in its
// thread's registers (Welford); its histogram row lives in LDS and is touched by that thread alone, so the
// read-modify-write needs no atomic; rows are an odd number of words apart, which spreads the lanes over the banks.
template <class T, bool HIST>
__global__ __launch_bounds__(STATS_TILE) void k_stats_part(const StatsArgs a)
{
    __shared__ uint32_t s_hist[HIST ? STATS_TILE * STATS_HSTRIDE : 1];
    __shared__ double s_edge[HIST ? KIDMP_STATS_MAX_BINS + 1 : 1];
    const int lane = threadIdx.x, cell = blockIdx.y, g = cell / a.nfield, f = cell - g * a.nfield;
    const int k0 = blockIdx.z * STATS_TILE, k = k0 + lane;
    const bool live = k < a.nz;
    const int nb3 = a.nbin + 3, hs = nb3 | 1;                 // hs <= STATS_HSTRIDE
    int top = 1;                                              // the largest power of two <= nbin + 1
    if (HIST) {
        for (int i = lane; i < STATS_TILE * hs; i += STATS_TILE) s_hist[i] = 0u;
        for (int i = lane; i <= a.nbin; i += STATS_TILE) s_edge[i] = a.edges[int64_t(f) * (a.nbin + 1) + i];
        while (2 * top <= a.nbin + 1) top *= 2;
        __syncthreads();
    }
    const T *x = static_cast<const T *>(a.field[f]) + k;      // dereferenced by live lanes only
    const int64_t cs = a.stride[f];
    const double flo = a.floor[f];
    const int32_t *grp = a.group;
    const int64_t c0 = int64_t(blockIdx.x) * a.per;
    const int64_t c1 = (grp || g == 0) ? (c0 + a.per < a.ncol ? c0 + a.per : a.ncol) : c0;   // no ids: all in group 0
    Moments m = empty_moments();
    uint32_t *row = s_hist + (HIST ? lane * hs : 0);
    for (int64_t c = c0; c < c1; c += STATS_UNROLL) {
        double v[STATS_UNROLL];
        bool in[STATS_UNROLL];
#pragma unroll
        for (int u = 0; u < STATS_UNROLL; ++u) {
            const int64_t cc = c + u;
            const bool mine = cc < c1 && (!grp || grp[cc] == g);   // the same for every lane
            in[u] = mine && live;
            v[u] = in[u] ? double(x[cc * cs]) : 0.;
        }
#pragma unroll
        for (int u = 0; u < STATS_UNROLL; ++u) {
            if (!in[u]) continue;
            const double xv = v[u];
            if (HIST) {
                int slot = a.nbin + 2;                        // NaN
                if (xv == xv) {                               // slot = number of edges <= xv, in [0, nbin+1]
                    slot = 0;
                    for (int step = top; step >= 1; step >>= 1) {
                        const int j = slot + step;
                        if (j <= a.nbin + 1 && s_edge[j - 1] <= xv) slot = j;
                    }
                }
                row[slot] += 1u;
            }
            if (xv > flo && xv <= DBL_MAX) {                   // finite and above the floor
                m.n += 1.;
                const double d = xv - m.mean;
                m.mean += d / m.n;
                m.m2 += d * (xv - m.mean);
                m.mn = fmin(m.mn, xv);
                m.mx = fmax(m.mx, xv);
            }
        }
    }
    const int64_t slab = int64_t(blockIdx.x) * gridDim.y + cell;
    if (live) {
        double *o = a.pm + slab * KIDMP_STATS_NMOM * a.nz + k;
        o[0] = m.n;
        o[a.nz] = m.mean;
        o[2 * a.nz] = m.m2;
        o[3 * a.nz] = m.mn;
        o[4 * a.nz] = m.mx;
    }
    if (HIST) {
        __syncthreads();
        const int rows = a.nz - k0 < STATS_TILE ? a.nz - k0 : STATS_TILE;
        uint32_t *o = a.ph + (slab * a.nz + k0) * nb3;        // the tile's rows are contiguous: a coalesced copy
        for (int i = lane; i < rows * nb3; i += STATS_TILE) o[i] = s_hist[(i / nb3) * hs + i % nb3];
    }
}

// Combine pass: thread i < ncell*nz merges the chunks of cell-level i in index order (Chan); thread i < ncell*nz*(nbin+3)
// adds the chunks' counts of histogram slot i into int64.
__global__ void k_stats_combine(int nch, int64_t ncell, int nz, int nbin, const double *__restrict__ pm,
                                const uint32_t *__restrict__ ph, double *__restrict__ mom, int64_t *__restrict__ hist)
{
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < ncell * nz) {
        const int64_t cell = i / nz, k = i - cell * nz;
        Moments acc = empty_moments();
        for (int ch = 0; ch < nch; ++ch) {
            const double *p = pm + ((int64_t(ch) * ncell + cell) * KIDMP_STATS_NMOM) * nz + k;
            const Moments b = {p[0], p[nz], p[2 * int64_t(nz)], p[3 * int64_t(nz)], p[4 * int64_t(nz)]};
            chan_merge(acc, b);
        }
        double *o = mom + cell * KIDMP_STATS_NMOM * nz + k;
        o[0] = acc.n;
        o[nz] = acc.mean;
        o[2 * int64_t(nz)] = acc.m2;
        o[3 * int64_t(nz)] = acc.mn;
        o[4 * int64_t(nz)] = acc.mx;
    }
    const int64_t nh = nbin ? ncell * nz * (nbin + 3) : 0;
    if (i < nh) {
        int64_t s = 0;
        for (int ch = 0; ch < nch; ++ch) s += int64_t(ph[int64_t(ch) * nh + i]);
        hist[i] = s;
    }
}

bool stats_shape_ok(int64_t ncol, int32_t nz, int32_t nfield, int32_t ngroup, int32_t nbin)
{
    return ncol >= 0 && ncol <= STATS_MAX_NCOL && nz >= 2 && nz <= KIDMP_MAX_NZ && nfield >= 1 && nfield <= KIDMP_STATS_MAX_FIELDS &&
           ngroup >= 1 && ngroup <= KIDMP_STATS_MAX_GROUPS && nbin >= 0 && nbin <= KIDMP_STATS_MAX_BINS;
}

template <class T>
int level_stats_device(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, const kidmp_stats_request *req, double *mom,
                       int64_t *hist, void *work, size_t work_bytes, void *stream)
{
    const std::string w(who);
    if (int rc = require_ready(ctx)) return rc;
    if (!req) return fail(ctx, KIDMP_EINVAL, w + ": null request");
    if (ncol < 0 || ncol > STATS_MAX_NCOL) return fail(ctx, KIDMP_EINVAL, w + ": ncol outside [0, 2**39]");
    if (nz < 2 || nz > KIDMP_MAX_NZ) return fail(ctx, KIDMP_EINVAL, w + ": nz outside [2, KIDMP_MAX_NZ]");
    if (!stats_shape_ok(ncol, nz, req->nfield, req->ngroup, req->nbin))
        return fail(ctx, KIDMP_EINVAL, w + ": nfield, ngroup or nbin outside its range");
    if (!req->field || !mom || (req->nbin > 0 && (!hist || !req->edges))) return fail(ctx, KIDMP_EINVAL, w + ": null array argument");
    StatsArgs a{};
    for (int f = 0; f < req->nfield; ++f) {
        a.field[f] = req->field[f];
        a.stride[f] = req->col_stride ? req->col_stride[f] : nz;
        a.floor[f] = req->floor ? req->floor[f] : -HUGE_VAL;
        if (!a.field[f] && ncol > 0) return fail(                  // an empty batch has nothing to point at
ctx, KIDMP_EINVAL, w + ": null array argument");
        if (a.stride[f] < nz) return fail(ctx, KIDMP_EINVAL, w + ": col_stride < nz");
    }
    const size_t need = kidmp_stats_workspace_bytes(ncol, nz, req->nfield, req->ngroup, req->nbin);
    if (ncol > 0 && (!work || work_bytes < need || reinterpret_cast<uintptr_t>(work) % 8 != 0))
        return fail(ctx, KIDMP_EINVAL, w + ": the workspace is too small or misaligned (kidmp_stats_workspace_bytes)");
    GUARD(ctx);
    for (int f = 0; f < req->nfield; ++f)
        if (int rc = check_device_array(ctx, who, a.field[f], "a field")) return rc;
    const char *names[] = {"group", "edges", "mom", "hist", "work"};
    const void *ptrs[] = {req->group, req->nbin > 0 ? req->edges : nullptr, mom, req->nbin > 0 ? hist : nullptr, ncol > 0 ? work : nullptr};
    for (int i = 0; i < 5; ++i)
        if (int rc = check_device_array(ctx, who, ptrs[i], names[i])) return rc;

    hipStream_t s = (hipStream_t)stream;
    const int64_t ncell = int64_t(req->ngroup) * req->nfield;
    const int chunks = kidmp_stats_chunks(ncol);
    int used = 0;
    a.pm = static_cast<double *>(work);
    a.ph = reinterpret_cast<uint32_t *>(a.pm + int64_t(chunks) * ncell * KIDMP_STATS_NMOM * nz);
    if (ncol > 0) {
        a.group = req->group;
        a.edges = req->edges;
        a.ncol = ncol;
        a.per = (ncol + chunks - 1) / chunks;
        a.nz = nz;
        a.nfield = req->nfield;
        a.nbin = req->nbin;
        used = int((ncol + a.per - 1) / a.per);               // trailing chunks without a column are not launched
        const dim3 grid((unsigned)used, (unsigned)ncell, (unsigned)((nz + STATS_TILE - 1) / STATS_TILE)), block(STATS_TILE);
        if (req->nbin > 0) hipLaunchKernelGGL((k_stats_part<T, true>), grid, block, 0, s, a);
        else               hipLaunchKernelGGL((k_stats_part<T, false>), grid, block, 0, s, a);
        HIPTRY(ctx, hipGetLastError());
    }
    const int64_t nthread = ncell * nz * (req->nbin > 0 ? req->nbin + 3 : 1);
    hipLaunchKernelGGL(k_stats_combine, dim3((unsigned)((nthread + 255) / 256)), dim3(256), 0, s, used, ncell, nz, req->nbin, a.pm, a.ph,
                       mom, hist);
    HIPTRY(ctx, hipGetLastError());
    return KIDMP_OK;
}
}  // namespace

extern "C" {
int32_t kidmp_stats_chunks(int64_t ncol)
{
    return ncol <= 0 ? 0 : int32_t(ncol < STATS_CHUNKS ? ncol : STATS_CHUNKS);
}

size_t kidmp_stats_workspace_bytes(int64_t ncol, int32_t nz, int32_t nfield, int32_t ngroup, int32_t nbin)
{
    if (!stats_shape_ok(ncol, nz, nfield, ngroup, nbin)) return 0;
    const size_t per_level = KIDMP_STATS_NMOM * sizeof(double) + (nbin > 0 ? size_t(nbin + 3) * sizeof(uint32_t) : 0);
    const size_t bytes = size_t(kidmp_stats_chunks(ncol)) * size_t(ngroup) * size_t(nfield) * size_t(nz) * per_level;
    return (bytes + 255) / 256 * 256;
}

int kidmp_level_stats_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const kidmp_stats_request *req, double *mom,
                             int64_t *hist, void *work, size_t work_bytes, void *stream)
{
    return level_stats_device<double>(ctx, "kidmp_level_stats_device", ncol, nz, req, mom, hist, work, work_bytes, stream);
}
int kidmp32_level_stats_device(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const kidmp_stats_request *req, double *mom,
                               int64_t *hist, void *work, size_t work_bytes, void *stream)
{
    return level_stats_device<float>(ctx, "kidmp32_level_stats_device", ncol, nz, req, mom, hist, work, work_bytes, stream);
}

int kidmp_stats_merge(int64_t ncell, int32_t nz, int32_t nbin, double *mom_a, int64_t *hist_a, const double *mom_b,
                      const int64_t *hist_b)
{
    if (ncell < 0 || nz < 1 || nbin < 0 || nbin > KIDMP_STATS_MAX_BINS) return fail(nullptr, KIDMP_EINVAL, "kidmp_stats_merge: bad argument");
    if (!mom_a || !mom_b || (nbin > 0 && (!hist_a || !hist_b))) return fail(nullptr, KIDMP_EINVAL, "kidmp_stats_merge: null argument");
    for (int64_t cell = 0; cell < ncell; ++cell)
        for (int64_t k = 0; k < nz; ++k) {
            double *pa = mom_a + cell * KIDMP_STATS_NMOM * nz + k;
            const double *pb = mom_b + cell * KIDMP_STATS_NMOM * nz + k;
            Moments a = {pa[0], pa[nz], pa[2 * int64_t(nz)], pa[3 * int64_t(nz)], pa[4 * int64_t(nz)]};
            chan_merge(a, {pb[0], pb[nz], pb[2 * int64_t(nz)], pb[3 * int64_t(nz)], pb[4 * int64_t(nz)]});
            pa[0] = a.n;
            pa[nz] = a.mean;
            pa[2 * int64_t(nz)] = a.m2;
            pa[3 * int64_t(nz)] = a.mn;
            pa[4 * int64_t(nz)] = a.mx;
        }
    const int64_t nh = nbin > 0 ? ncell * nz * (nbin + 3) : 0;
    for (int64_t i = 0; i < nh; ++i) hist_a[i] += hist_b[i];
    return KIDMP_OK;
}
}  // extern "C"
