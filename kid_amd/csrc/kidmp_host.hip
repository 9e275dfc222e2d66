// kidmp_host.hip -- the entries of include/kidmp.h that take host arrays.
#include "kidmp_ctx.h"

using namespace kidmp;

// ---- the host-array entries (kidmp_batch_step_host*, kidmp32_batch_step_host): a three-stage pipeline over column chunks ----
// The batch is cut into chunks of CH columns; chunk i is uploaded on the context's H2D stream, stepped on its compute
// stream and downloaded on its D2H stream, through a ring of HOST_NBUF staging sets in HBM, so the two DMA directions
// (PCIe is full duplex) and the kernel work on three different chunks at once.  Host arrays that are page-locked
// (kidmp_host_alloc, or the caller's own hipHostMalloc / hipHostRegister) are moved by the DMA
// engines asynchronously; pageable arrays still work, but the runtime stages them through its own bounce buffer and
// the calling thread waits for each copy.  Per column-step the boundary moves 14 (15 with w) profiles in and 12 out
// (+36 for the rate diagnostics): about 25 KB in binary64.
int64_t kidmp::pick_host_chunk(const kidmp_ctx *ctx, int64_t ncol) { return stage_pick_chunk(ctx->host_chunk, ncol); }

// the context's staging memory only grows
int kidmp::ensure_stage(kidmp_ctx *ctx, size_t need)
{
    if (need <= ctx->stage_bytes) return KIDMP_OK;
    if (ctx->d_stage) (void)hipFree(ctx->d_stage);
    ctx->d_stage = nullptr;
    ctx->stage_bytes = 0;
    HIPTRY(ctx, hipMalloc((void **)&ctx->d_stage, need));
    ctx->stage_bytes = need;
    return KIDMP_OK;
}

// ---- the host-array entries of the diagnostics (reflectivity, radii, summary, fall speeds, Doppler moments and spectra,
// size spectra, lidar, bright band, cloud radar, radiometer, polarimetric and multichannel): ONE body ----
// The entry describes its arrays (kidmp_stage_plan.h); the batch goes through the context's staging memory in chunks of
// plan.chunk columns, strictly one after the other on the context's compute stream: the shared profiles and the caller's
// grids go up once, then per chunk what the kernel reads goes up, enqueue(c0, n) launches over the slots and what was asked
// for comes down.  A column's result does not depend on its batch, so any chunking gives the same bits.  Page-locked host
// arrays are moved asynchronously; the one synchronise at the end holds in every case, so that no copy is still in flight
// towards the caller's arrays when the entry returns, and the first error is the one reported.
int kidmp::stage_open(kidmp_ctx *ctx, const StagePlan &plan)
{
    if (int rc = ensure_stage(ctx, plan.total)) return rc;
    for (int i = 0; i < plan.na; ++i)
        if (plan.a[i].host) plan.a[i].dev = reinterpret_cast<char *>(ctx->d_stage) + plan.a[i].offset;
    return KIDMP_OK;
}

namespace {
// every slab of one array, up or down: the columns [c0, c0 + n)
hipError_t stage_move(kidmp_ctx *ctx, const StageArray &a, bool down, int64_t c0, int64_t n)
{
    hipError_t e = hipSuccess;
    for (int s = 0; s < a.nslab && e == hipSuccess; ++s) {
        const StageCopy c = stage_copy(a, s, c0, n);
        char *const host = const_cast<char *>(static_cast<const char *>(a.host)) + c.host_off;
        char *const dev = reinterpret_cast<char *>(ctx->d_stage) + c.stage_off;
        const hipMemcpyKind kind = down ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
        if (c.rows == 1) e = down ? hipMemcpyAsync(host, dev, c.row_bytes, kind, ctx->stream) : hipMemcpyAsync(dev, host, c.row_bytes, kind, ctx->stream);
        else e = down ? hipMemcpy2DAsync(host, c.host_pitch, dev, c.row_bytes, c.row_bytes, c.rows, kind, ctx->stream)
                      : hipMemcpy2DAsync(dev, c.row_bytes, host, c.host_pitch, c.row_bytes, c.rows, kind, ctx->stream);
    }
    return e;
}
}  // namespace

int kidmp::stage_run(kidmp_ctx *ctx, const StagePlan &plan, const std::function<hipError_t(int64_t, int64_t)> &enqueue)
{
    const StageArray *const a = plan.a;
    hipError_t e = hipSuccess;
    auto move = [&](bool down, bool before, int64_t c0, int64_t n) {
        for (int i = 0; i < plan.na && e == hipSuccess; ++i)
            if (a[i].host && (a[i].dir & (down ? STAGE_DOWN : STAGE_UP)) && stage_before_loop(a[i]) == before) e = stage_move(ctx, a[i], down, c0, n);
    };
    move(false, true, 0, 0);
    for (int64_t c0 = 0; c0 < plan.ncol && e == hipSuccess; c0 += plan.chunk) {
        const int64_t n = stage_chunk_cols(plan, c0);
        move(false, false, c0, n);
        if (e == hipSuccess) e = enqueue(c0, n);
        move(true, false, c0, n);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    HIPTRY(ctx, e);
    HIPTRY(ctx, es);
    return KIDMP_OK;
}

namespace {
// Leaving host_pipeline with an error must not leave DMA in flight towards the caller's arrays.
struct PipelineDrain {
    kidmp_ctx *c;
    bool armed = true;
    ~PipelineDrain()
    {
        if (!armed) return;
        (void)hipStreamSynchronize(c->s_h2d);
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->s_d2h);
    }
};

// calc_refl10cm on host arrays: stage_run above
template <class T>
int refl_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const T *t, const T *p, const T *qv, const T *qr, const T *nr,
              const T *qs, const T *qg, T *dbz)
{
    const void *req[] = {t, p, qv, qr, nr, dbz};
    if (int rc = check_refl_args(ctx, ncol, nz, req, 6, qs, qg)) return rc;
    if (ncol == 0) return KIDMP_OK;
    GUARD(ctx);
    const T *h[7] = {t, p, qv, qr, nr, qs, qg};
    StageArray a[8];                                          // every array keeps its slot
    for (int v = 0; v < 7; ++v) a[v] = stage_keep(stage_array(h[v], nz, STAGE_UP));
    a[7] = stage_array(dbz, nz, STAGE_DOWN);
    const StagePlan plan = stage_plan(a, ncol, pick_host_chunk(ctx, ncol));
    if (int rc = stage_open(ctx, plan)) return rc;
    T *d[8];
    for (int v = 0; v < 8; ++v) d[v] = staged<T>(a[v]);
    const ReflConsts c = refl_consts(ctx->hc);
    return stage_run(ctx, plan, [&](int64_t, int64_t n) {
        return launch_reflectivity<T>(c, n, nz, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], ctx->stream);
    });
}

// calc_effectRad (M:4834-4935) on host arrays of n elements, INOUT (stage_run): re_* go up as well as down.  The entry has
// no nz, so its n elements are columns of one element and a chunk is the context's chunk size in columns of a nominal 128
// levels.
template <class T>
int radii_host(kidmp_ctx *ctx, const char *who, int64_t n, const T *t, const T *p, const T *qv, const T *qc, const T *nc,
               const T *qi, const T *ni, const T *qs, T *re_qc, T *re_qi, T *re_qs)
{
    if (int rc = check_radii_args<T>(ctx, who, n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs)) return rc;
    if (n == 0) return KIDMP_OK;
    int64_t nz_col = 0;
    if (int rc = nc_levels_of(ctx, who, n, nz_col)) return rc;
    GUARD(ctx);
    const int64_t want = (ctx->host_chunk > 0 ? ctx->host_chunk : 8192) * 128;
    const T *h[11] = {t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs};
    StageArray a[11];                                         // every array keeps its slot
    for (int v = 0; v < 11; ++v) a[v] = stage_keep(stage_array(h[v], 1, v < 8 ? STAGE_UP : STAGE_BOTH));
    const StagePlan plan = stage_plan(a, n, want < n ? want : n);
    if (int rc = stage_open(ctx, plan)) return rc;
    T *d[11];
    for (int v = 0; v < 11; ++v) d[v] = staged<T>(a[v]);
    return stage_run(ctx, plan, [&](int64_t off, int64_t cnt) {
        return launch_radii_keep<T>(ctx, cnt, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], ctx->stream, nz_col, off);
    });
}
}  // namespace

// extra.out (optional, host arrays): calc_refl10cm (M:4946-5244) and calc_effectRad (M:4834-4935, the driver's preset form
// of M:1111-1116) of every chunk's post-step state, formed by ONE launch on the compute stream right after the step.  Only
// the requested profiles are staged and come back.
template <class T>
int kidmp::host_pipeline(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, T *const *io, const T *const *in, T *ppt,
                         double *rates, int32_t *nstep, int32_t arith, const PipelineExtras<T> &extra)
{
    const auto [exact_sums, scan_sanity, out] = extra;
    if (int rc = check_outputs_request<T>(ctx, "kidmp", out)) return rc;
    T *const hout[4] = {out.dbz, out.re_qc, out.re_qi, out.re_qs};
    const int n_out = (out.dbz != nullptr) + (out.re_qc != nullptr) + (out.re_qi != nullptr) + (out.re_qs != nullptr);
    // Arrays the caller may leave out (NULL), as KiD itself does (W:36 passes nc1d, nwfa1d, nifa1d unset; a warm run
    // never touches the frozen species, W:46-52): they then neither cross PCIe nor come back.
    //   nc, nwfa, nifa (all three)   non-aerosol contexts: the defaults of M:958-964, formed on the device
    //   qi, qs, qg, ni (all four)    iiwarm contexts: exactly zero (and they stay zero)
    const bool has_w = ctx->cfg.is_aerosol_aware != 0;
    const int n_aer = (io[8] != nullptr) + (io[9] != nullptr) + (io[10] != nullptr);
    const int n_frz = (io[2] != nullptr) + (io[4] != nullptr) + (io[5] != nullptr) + (io[6] != nullptr);
    const bool skip_aer = n_aer == 0 && ncol > 0, skip_frz = n_frz == 0 && ncol > 0;
    if (ncol > 0 && n_aer != 0 && n_aer != 3) return fail(ctx, KIDMP_EINVAL, "kidmp: nc, nwfa, nifa must be given or left out together");
    if (ncol > 0 && n_frz != 0 && n_frz != 4) return fail(ctx, KIDMP_EINVAL, "kidmp: qi, qs, qg, ni must be given or left out together");
    if (skip_aer && has_w) return fail(ctx, KIDMP_EINVAL, "kidmp: an aerosol-aware context needs nc, nwfa and nifa");
    if (skip_frz && !ctx->cfg.iiwarm) return fail(ctx, KIDMP_EINVAL, "kidmp: a mixed-phase context needs qi, qs, qg and ni");
    const void *ptrs[15];
    int np = 0;
    for (int v = 0; v < 12; ++v) {
        const bool optional_out = (skip_aer && v >= 8 && v <= 10) || (skip_frz && (v == 2 || v == 4 || v == 5 || v == 6));
        if (!optional_out) ptrs[np++] = io[v];
    }
    ptrs[np++] = in[0]; ptrs[np++] = in[1]; ptrs[np++] = ppt;
    if (int rc = check_step_args(ctx, ncol, nz, dt, ptrs, np)) return rc;
    if (int rc = check_nc_count(ctx, "kidmp_batch_step_host", ncol)) return rc;
    if (has_w && !in[2] && ncol > 0) return fail(ctx, KIDMP_EINVAL, "kidmp: an aerosol-aware context needs the updraft profile w");
    if (ncol == 0) {
        if (exact_sums || scan_sanity) {
            GUARD(ctx);
            if (exact_sums) HIPTRY(ctx, hipMemset(ctx->d_acc, 0, ACC_N * sizeof(unsigned long long)));
            if (scan_sanity) HIPTRY(ctx, hipMemset(ctx->d_sanity, 0, SANITY_N * sizeof(unsigned long long)));
        }
        return KIDMP_OK;
    }
    GUARD(ctx);
    const int64_t CH = pick_host_chunk(ctx, ncol);
    const int64_t nchunk = (ncol + CH - 1) / CH;
    const int nbuf = nchunk < HOST_NBUF ? int(nchunk) : HOST_NBUF;
    const size_t prof = size_t(CH) * size_t(nz);
    // one staging set: [rates (double)] [15 profiles + ppt (T)] [nstep (int32)], each part 256-byte aligned
    auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_rates = rates ? up256(size_t(KIDMP_NRATES) * prof * sizeof(double)) : 0;
    const size_t b_prof = up256(prof * sizeof(T));
    const size_t b_ppt = up256(4 * size_t(CH) * sizeof(T));
    const size_t b_nstep = nstep ? up256(4 * size_t(CH) * sizeof(int32_t)) : 0;
    const size_t b_set = b_rates + size_t(15 + n_out) * b_prof + b_ppt + b_nstep;
    if (int rc = ensure_stage(ctx, b_set * size_t(nbuf))) return rc;
    char *const base = reinterpret_cast<char *>(ctx->d_stage);
    PipelineDrain drain{ctx};
    if (exact_sums) HIPTRY(ctx, hipMemsetAsync(ctx->d_acc, 0, ACC_N * sizeof(unsigned long long), ctx->stream));
    if (scan_sanity) HIPTRY(ctx, hipMemsetAsync(ctx->d_sanity, 0, SANITY_N * sizeof(unsigned long long), ctx->stream));
    for (int64_t i = 0; i < nchunk; ++i) {
        const int b = int(i % nbuf);
        const int64_t c0 = i * CH, n = (c0 + CH <= ncol ? CH : ncol - c0);
        const size_t off = size_t(c0) * size_t(nz), cnt = size_t(n) * size_t(nz);
        char *set = base + size_t(b) * b_set;
        double *drates = rates ? reinterpret_cast<double *>(set) : nullptr;
        T *dio[12]; const T *din[3];
        char *q = set + b_rates;
        for (int v = 0; v < 12; ++v) { dio[v] = reinterpret_cast<T *>(q); q += b_prof; }
        T *dinw[3];
        for (int v = 0; v < 3; ++v) { dinw[v] = reinterpret_cast<T *>(q); din[v] = dinw[v]; q += b_prof; }
        T *dppt = reinterpret_cast<T *>(q); q += b_ppt;
        int32_t *dnstep = nstep ? reinterpret_cast<int32_t *>(q) : nullptr;
        q += b_nstep;
        T *dout[4] = {};
        for (int v = 0; v < 4; ++v)
            if (hout[v]) { dout[v] = reinterpret_cast<T *>(q); q += b_prof; }
        if (!has_w || !in[2]) din[2] = nullptr;
        // upload (the set is free once the download of the chunk that used it last has finished)
        if (i >= nbuf) HIPTRY(ctx, hipStreamWaitEvent(ctx->s_h2d, ctx->ev_down[b], 0));
        for (int v = 0; v < 12; ++v)
            if (io[v]) HIPTRY(ctx, hipMemcpyAsync(dio[v], io[v] + off, cnt * sizeof(T), hipMemcpyHostToDevice, ctx->s_h2d));
        for (int v = 0; v < (din[2] ? 3 : 2); ++v) HIPTRY(ctx, hipMemcpyAsync(dinw[v], in[v] + off, cnt * sizeof(T), hipMemcpyHostToDevice, ctx->s_h2d));
        HIPTRY(ctx, hipMemcpyAsync(dppt, ppt + 4 * c0, 4 * size_t(n) * sizeof(T), hipMemcpyHostToDevice, ctx->s_h2d));
        HIPTRY(ctx, hipEventRecord(ctx->ev_up[b], ctx->s_h2d));
        // step
        HIPTRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_up[b], 0));
        if (skip_frz)
            for (int v : {2, 4, 5, 6}) HIPTRY(ctx, hipMemsetAsync(dio[v], 0, cnt * sizeof(T), ctx->stream));
        if (skip_aer) {
            launch_default_aerosols<T>(int64_t(cnt), T(ctx->hc.Nt_c), dio[0], dio[11], din[0], dio[8], dio[9], dio[10], ctx->stream,
                                       ctx->d_nc_col ? ctx->d_nc_col + c0 : nullptr, nz);   // (the bound buffer: nothing extra crosses PCIe)
            HIPTRY(ctx, hipGetLastError());
        }
        if (int rc = step_device<T>(ctx, n, nz, T(dt), dio, din[0], din[2], din[1], dppt, drates, dnstep, arith, ctx->stream, c0)) return rc;
        if (n_out)                                            // the outputs of the chunk's post-step state
            HIPTRY(ctx, launch_outputs<T>(ctx, n, nz, {dio[11], din[0], dio[0], dio[1], dio[8], dio[2], dio[6], dio[3], dio[7],
                                                       dio[4], dio[5]}, {dout[0], dout[1], dout[2], dout[3]}, ctx->stream, c0));
        if (exact_sums) HIPTRY(ctx, launch_ppt_exact<T>(n, dppt, ctx->d_acc, ctx->stream));   // the chunk's share of the domain sums
        if constexpr (std::is_same<T, double>::value)
            if (scan_sanity) {                                // the scan of M:1025-1094 over the chunk's end state (exact integer atomics)
                launch_sanity(int64_t(cnt), {dio[1], dio[3], dio[7], dio[4], dio[2], dio[5], dio[6], dio[0]}, ctx->d_sanity, ctx->stream);
                HIPTRY(ctx, hipGetLastError());
            }
        HIPTRY(ctx, hipEventRecord(ctx->ev_step[b], ctx->stream));
        // download
        HIPTRY(ctx, hipStreamWaitEvent(ctx->s_d2h, ctx->ev_step[b], 0));
        for (int v = 0; v < 12; ++v)
            if (io[v]) HIPTRY(ctx, hipMemcpyAsync(io[v] + off, dio[v], cnt * sizeof(T), hipMemcpyDeviceToHost, ctx->s_d2h));
        HIPTRY(ctx, hipMemcpyAsync(ppt + 4 * c0, dppt, 4 * size_t(n) * sizeof(T), hipMemcpyDeviceToHost, ctx->s_d2h));
        if (rates) HIPTRY(ctx, hipMemcpyAsync(rates + size_t(KIDMP_NRATES) * off, drates, size_t(KIDMP_NRATES) * cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->s_d2h));
        if (nstep) HIPTRY(ctx, hipMemcpyAsync(nstep + 4 * c0, dnstep, 4 * size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->s_d2h));
        for (int v = 0; v < 4; ++v)
            if (hout[v]) HIPTRY(ctx, hipMemcpyAsync(hout[v] + off, dout[v], cnt * sizeof(T), hipMemcpyDeviceToHost, ctx->s_d2h));
        HIPTRY(ctx, hipEventRecord(ctx->ev_down[b], ctx->s_d2h));
    }
    HIPTRY(ctx, hipStreamSynchronize(ctx->s_d2h));           // everything else precedes it through the events
    drain.armed = false;
    return KIDMP_OK;
}
template int kidmp::host_pipeline<double>(kidmp_ctx *, int64_t, int32_t, double, double *const *, const double *const *, double *,
                                          double *, int32_t *, int32_t, const PipelineExtras<double> &);   // for kidmp_multi.hip


// mphys_thompson09_interfacen (W:28-310) on host arrays, inside the same ring: per chunk the present members of state,
// adv and div and exner go up (dz once, ahead of the first chunk), gather / step / outputs / back-out run on the compute
// stream (kid_enqueue, the body of the device entry), and mphys, ppt and what else was asked for come down.  One
// staging set: [rates] [workspace: 15 profiles] [state, adv, div: 9 each] [exner] [mphys: 9] [outputs] [ppt] [nstep].
template <class T>
int kidmp::kid_host(kidmp_ctx *ctx, const KidCall<T> &h)
{
    const int64_t ncol = h.ncol;
    const int32_t nz = h.nz;
    GUARD(ctx);
    const int64_t CH = pick_host_chunk(ctx, ncol);
    const int64_t nchunk = (ncol + CH - 1) / CH;
    const int nbuf = nchunk < HOST_NBUF ? int(nchunk) : HOST_NBUF;
    const size_t prof = size_t(CH) * size_t(nz);
    auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
    T *const hout[4] = {h.out.dbz, h.out.re_qc, h.out.re_qi, h.out.re_qs};
    int n_in = 1, n_out = 0;                                     // exner
    for (int m = 0; m < KID_NF; ++m) {
        n_in += (h.state.f[m] != nullptr) + (h.adv.f[m] != nullptr) + (h.div.f[m] != nullptr);
        n_out += h.mphys.f[m] != nullptr;
    }
    for (int v = 0; v < 4; ++v) n_out += hout[v] != nullptr;
    const size_t b_rates = h.rates ? up256(size_t(KIDMP_NRATES) * prof * sizeof(double)) : 0;
    const size_t b_prof = up256(prof * sizeof(T));
    const size_t b_ppt = up256(4 * size_t(CH) * sizeof(T));
    const size_t b_nstep = h.nstep ? up256(4 * size_t(CH) * sizeof(int32_t)) : 0;
    const size_t b_set = b_rates + size_t(KID_NWORK + n_in + n_out) * b_prof + b_ppt + b_nstep;
    const size_t b_dz = up256(size_t(nz) * sizeof(T));
    if (int rc = ensure_stage(ctx, b_dz + b_set * size_t(nbuf))) return rc;
    T *const ddz = reinterpret_cast<T *>(ctx->d_stage);
    char *const base = reinterpret_cast<char *>(ctx->d_stage) + b_dz;
    PipelineDrain drain{ctx};
    HIPTRY(ctx, hipMemcpyAsync(ddz, h.dz, size_t(nz) * sizeof(T), hipMemcpyHostToDevice, ctx->s_h2d));
    for (int64_t i = 0; i < nchunk; ++i) {
        const int b = int(i % nbuf);
        const int64_t c0 = i * CH, n = (c0 + CH <= ncol ? CH : ncol - c0);
        const size_t off = size_t(c0) * size_t(nz), cnt = size_t(n) * size_t(nz);
        char *q = base + size_t(b) * b_set;
        double *drates = h.rates ? reinterpret_cast<double *>(q) : nullptr;
        q += b_rates;
        // the chunk's workspace: profile strides of the CHUNK's own column count, so that kid_enqueue finds them
        char *const dwork = q;
        q += size_t(KID_NWORK) * b_prof;
        auto take = [&](const void *host) { T *d = nullptr; if (host) { d = reinterpret_cast<T *>(q); q += b_prof; } return d; };
        KidCall<T> d = h;
        d.ncol = n;
        for (int m = 0; m < KID_NF; ++m) { d.state.f[m] = take(h.state.f[m]); d.adv.f[m] = take(h.adv.f[m]); d.div.f[m] = take(h.div.f[m]); }
        T *const dex = take(h.exner);
        for (int m = 0; m < KID_NF; ++m) d.mphys.f[m] = take(h.mphys.f[m]);
        T *dout[4];
        for (int v = 0; v < 4; ++v) dout[v] = take(hout[v]);
        d.out = {dout[0], dout[1], dout[2], dout[3]};
        T *const dppt = reinterpret_cast<T *>(q); q += b_ppt;
        int32_t *const dnstep = h.nstep ? reinterpret_cast<int32_t *>(q) : nullptr;
        d.exner = dex; d.dz = ddz; d.ppt = dppt; d.rates = drates; d.nstep = dnstep;
        // upload (the set is free once the download of the chunk that used it last has finished)
        if (i >= nbuf) HIPTRY(ctx, hipStreamWaitEvent(ctx->s_h2d, ctx->ev_down[b], 0));
        for (int m = 0; m < KID_NF; ++m) {
            const T *const src[3] = {h.state.f[m], h.adv.f[m], h.div.f[m]};
            T *const dst[3] = {d.state.f[m], d.adv.f[m], d.div.f[m]};
            for (int a = 0; a < 3; ++a)
                if (src[a]) HIPTRY(ctx, hipMemcpyAsync(dst[a], src[a] + off, cnt * sizeof(T), hipMemcpyHostToDevice, ctx->s_h2d));
        }
        HIPTRY(ctx, hipMemcpyAsync(dex, h.exner + off, cnt * sizeof(T), hipMemcpyHostToDevice, ctx->s_h2d));
        HIPTRY(ctx, hipEventRecord(ctx->ev_up[b], ctx->s_h2d));
        // gather, step, outputs, back-out
        HIPTRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_up[b], 0));
        if (int rc = kid_enqueue<T>(ctx, d, dwork, ctx->stream, c0)) return rc;
        HIPTRY(ctx, hipEventRecord(ctx->ev_step[b], ctx->stream));
        // download
        HIPTRY(ctx, hipStreamWaitEvent(ctx->s_d2h, ctx->ev_step[b], 0));
        for (int m = 0; m < KID_NF; ++m)
            if (h.mphys.f[m]) HIPTRY(ctx, hipMemcpyAsync(h.mphys.f[m] + off, d.mphys.f[m], cnt * sizeof(T), hipMemcpyDeviceToHost, ctx->s_d2h));
        HIPTRY(ctx, hipMemcpyAsync(h.ppt + 4 * c0, dppt, 4 * size_t(n) * sizeof(T), hipMemcpyDeviceToHost, ctx->s_d2h));
        if (h.rates) HIPTRY(ctx, hipMemcpyAsync(h.rates + size_t(KIDMP_NRATES) * off, drates, size_t(KIDMP_NRATES) * cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->s_d2h));
        if (h.nstep) HIPTRY(ctx, hipMemcpyAsync(h.nstep + 4 * c0, dnstep, 4 * size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->s_d2h));
        for (int v = 0; v < 4; ++v)
            if (hout[v]) HIPTRY(ctx, hipMemcpyAsync(hout[v] + off, dout[v], cnt * sizeof(T), hipMemcpyDeviceToHost, ctx->s_d2h));
        HIPTRY(ctx, hipEventRecord(ctx->ev_down[b], ctx->s_d2h));
    }
    HIPTRY(ctx, hipStreamSynchronize(ctx->s_d2h));           // everything else precedes it through the events
    drain.armed = false;
    return KIDMP_OK;
}

namespace {
template <class T, class F, class O>
int kid_host_entry(kidmp_ctx *ctx, const char *who, int64_t ncol, int32_t nz, T dt, T p0, T r_on_cp, const F *state, const F *adv,
                   const F *div, const T *exner, const T *dz, const F *mphys, T *ppt, double *rates, int32_t *nstep, const O *out,
                   int32_t arith)
{
    KidCall<T> c{};
    ColumnOutputs<T> o{};
    if (out) o = {out->dbz, out->re_qc, out->re_qi, out->re_qs};
    if (int rc = kid_check<T, F>(ctx, who, ncol, nz, double(dt), state, adv, div, exner, dz, mphys, ppt, o, arith, c)) return rc;
    if (ncol == 0) return KIDMP_OK;
    c.dt = dt; c.p0 = p0; c.r_on_cp = r_on_cp; c.rates = rates; c.nstep = nstep;
    return kid_host<T>(ctx, c);
}
}  // namespace

extern "C" {
int kidmp_kid_interface_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt, double p0, double r_on_cp,
                             const kidmp_kid_fields *state, const kidmp_kid_fields *adv, const kidmp_kid_fields *div,
                             const double *exner, const double *dz, const kidmp_kid_fields *mphys, double *ppt,
                             double *rates, int32_t *nstep, const kidmp_outputs *out)
{
    return kid_host_entry<double>(ctx, "kidmp_kid_interface_host", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, ppt,
                                  rates, nstep, out, 0);
}
int kidmp32_kid_interface_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt, float p0, float r_on_cp,
                               const kidmp32_kid_fields *state, const kidmp32_kid_fields *adv, const kidmp32_kid_fields *div,
                               const float *exner, const float *dz, const kidmp32_kid_fields *mphys, float *ppt,
                               double *rates, int32_t *nstep, const kidmp32_outputs *out, int32_t arith)
{
    return kid_host_entry<float>(ctx, "kidmp32_kid_interface_host", ncol, nz, dt, p0, r_on_cp, state, adv, div, exner, dz, mphys, ppt,
                                 rates, nstep, out, arith);
}
void *kidmp_host_alloc(size_t bytes)
{
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) { g_err = std::string("kidmp_host_alloc: ") + hipGetErrorString(e); return nullptr; }
    return p;
}
void kidmp_host_free(void *p) { if (p) (void)hipHostFree(p); }
int kidmp_set_host_chunk(kidmp_ctx *ctx, int64_t ncol_per_chunk)
{
    if (int rc = require_ready(ctx)) return rc;
    if (ncol_per_chunk < 0) return fail(ctx, KIDMP_EINVAL, "kidmp_set_host_chunk: negative chunk size");
    ctx->host_chunk = ncol_per_chunk;
    return KIDMP_OK;
}

int kidmp_batch_step_host_out(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                              double *qv, double *qc, double *qi, double *qr, double *qs, double *qg,
                              double *ni, double *nr, double *nc, double *nwfa, double *nifa, double *t,
                              const double *p, const double *w, const double *dz, double *ppt, double *rates,
                              int32_t *nstep, const kidmp_outputs *out)
{
    double *io[12] = {qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t};
    const double *in[3] = {p, dz, w};
    PipelineExtras<double> extra;
    if (out) extra.out = {out->dbz, out->re_qc, out->re_qi, out->re_qs};   // nothing requested: the plain step (_diag)
    return host_pipeline<double>(ctx, ncol, nz, dt, io, in, ppt, rates, nstep, 0, extra);
}
int kidmp32_batch_step_host_out(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                                float *qv, float *qc, float *qi, float *qr, float *qs, float *qg,
                                float *ni, float *nr, float *nc, float *nwfa, float *nifa, float *t,
                                const float *p, const float *w, const float *dz, float *ppt, double *rates,
                                int32_t *nstep, int32_t arith, const kidmp32_outputs *out)
{
    float *io[12] = {qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t};
    const float *in[3] = {p, dz, w};
    if (!valid_arith(arith)) return fail(ctx, KIDMP_EINVAL, BAD_ARITH);
    PipelineExtras<float> extra;
    if (out) extra.out = {out->dbz, out->re_qc, out->re_qi, out->re_qs};
    return host_pipeline<float>(ctx, ncol, nz, double(dt), io, in, ppt, rates, nstep, arith, extra);
}

int kidmp_batch_step_host_refl(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                               double *qv, double *qc, double *qi, double *qr, double *qs, double *qg,
                               double *ni, double *nr, double *nc, double *nwfa, double *nifa, double *t,
                               const double *p, const double *w, const double *dz, double *ppt, double *rates,
                               int32_t *nstep, double *dbz)
{
    const kidmp_outputs out = {dbz, nullptr, nullptr, nullptr};
    return kidmp_batch_step_host_out(ctx, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, &out);
}
int kidmp32_batch_step_host_refl(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                                 float *qv, float *qc, float *qi, float *qr, float *qs, float *qg,
                                 float *ni, float *nr, float *nc, float *nwfa, float *nifa, float *t,
                                 const float *p, const float *w, const float *dz, float *ppt, double *rates,
                                 int32_t *nstep, int32_t arith, float *dbz)
{
    const kidmp32_outputs out = {dbz, nullptr, nullptr, nullptr};
    return kidmp32_batch_step_host_out(ctx, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, arith, &out);
}

int kidmp_batch_step_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                          double *qv, double *qc, double *qi, double *qr, double *qs, double *qg,
                          double *ni, double *nr, double *nc, double *nwfa, double *nifa, double *t,
                          const double *p, const double *w, const double *dz, double *ppt, double *rates)
{
    return kidmp_batch_step_host_diag(ctx, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz,
                                      ppt, rates, nullptr);
}

int kidmp_batch_step_host_diag(kidmp_ctx *ctx, int64_t ncol, int32_t nz, double dt,
                               double *qv, double *qc, double *qi, double *qr, double *qs, double *qg,
                               double *ni, double *nr, double *nc, double *nwfa, double *nifa, double *t,
                               const double *p, const double *w, const double *dz, double *ppt, double *rates,
                               int32_t *nstep)
{
    return kidmp_batch_step_host_refl(ctx, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, nullptr);
}

int kidmp_column_step(kidmp_ctx *ctx, int32_t nz, double dt,
                      double *qv1d, double *qc1d, double *qi1d, double *qr1d, double *qs1d, double *qg1d,
                      double *ni1d, double *nr1d, double *nc1d, double *nwfa1d, double *nifa1d, double *t1d,
                      const double *p1d, const double *w1d, const double *dzq, double *ppt)
{
    return kidmp_batch_step_host(ctx, 1, nz, dt, qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, nr1d, nc1d, nwfa1d, nifa1d, t1d, p1d, w1d, dzq, ppt, nullptr);
}

int kidmp32_batch_step_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, float dt,
                            float *qv, float *qc, float *qi, float *qr, float *qs, float *qg,
                            float *ni, float *nr, float *nc, float *nwfa, float *nifa, float *t,
                            const float *p, const float *w, const float *dz, float *ppt, double *rates,
                            int32_t *nstep, int32_t arith)
{
    return kidmp32_batch_step_host_refl(ctx, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, arith, nullptr);
}
int kidmp32_column_step(kidmp_ctx *ctx, int32_t nz, float dt,
                        float *qv1d, float *qc1d, float *qi1d, float *qr1d, float *qs1d, float *qg1d,
                        float *ni1d, float *nr1d, float *nc1d, float *nwfa1d, float *nifa1d, float *t1d,
                        const float *p1d, const float *w1d, const float *dzq, float *ppt, int32_t arith)
{
    return kidmp32_batch_step_host(ctx, 1, nz, dt, qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, nr1d, nc1d, nwfa1d, nifa1d, t1d, p1d, w1d, dzq, ppt, nullptr, nullptr, arith);
}

int kidmp_reflectivity_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const double *t, const double *p,
                            const double *qv, const double *qr, const double *nr, const double *qs, const double *qg,
                            double *dbz)
{
    return refl_host<double>(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz);
}
int kidmp32_reflectivity_host(kidmp_ctx *ctx, int64_t ncol, int32_t nz, const float *t, const float *p,
                              const float *qv, const float *qr, const float *nr, const float *qs, const float *qg,
                              float *dbz)
{
    return refl_host<float>(ctx, ncol, nz, t, p, qv, qr, nr, qs, qg, dbz);
}

int kidmp_effective_radii_host(kidmp_ctx *ctx, int64_t n, const double *t, const double *p, const double *qv,
                               const double *qc, const double *nc, const double *qi, const double *ni, const double *qs,
                               double *re_qc, double *re_qi, double *re_qs)
{
    return radii_host<double>(ctx, "kidmp_effective_radii_host", n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs);
}
int kidmp32_effective_radii_host(kidmp_ctx *ctx, int64_t n, const float *t, const float *p, const float *qv,
                                 const float *qc, const float *nc, const float *qi, const float *ni, const float *qs,
                                 float *re_qc, float *re_qi, float *re_qs)
{
    return radii_host<float>(ctx, "kidmp32_effective_radii_host", n, t, p, qv, qc, nc, qi, ni, qs, re_qc, re_qi, re_qs);
}
}  // extern "C"
