// kidmp_multi.hip -- several GPUs behind one call: what a Fortran / C host (KiD's `do i=1,nx`, W:54-246, with nx in the millions) reaches
// without MPI.  Columns are independent and the tables read-only, so the batch is cut into contiguous ranges, one per
// context (= per device), each range goes through that context's own upload / step / download pipeline on its own host
// thread, and the ONE exchange of the path -- the domain sums of the surface precipitation, the nx-means of W:248-303
// -- is an RCCL all-reduce over the devices of the exact integer accumulators (k_ppt_exact): 24 int64, SUM.
#include <rccl/rccl.h>              // types only: the library is dlopen'ed by kidmp_init_multi (a one-GPU host needs no RCCL)
#include <dlfcn.h>

#include <mutex>
#include <new>
#include <thread>

#include "kidmp_ctx.h"

using namespace kidmp;

struct kidmp_multi {
    std::vector<kidmp_ctx *> ctx;            // one per entry of the device list, in list order
    std::vector<int> leader;                 // contexts that lead a distinct device (entries may repeat a device)
    std::vector<int> leader_of;              // ctx index -> index into `leader`
    std::vector<ncclComm_t> comm;            // one RCCL communicator per distinct device
    std::string err;
};

namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
std::mutex g_rccl_mu;
RcclApi g_rccl;

const char *load_rccl()       // nullptr on success, else what failed
{
    std::lock_guard<std::mutex> g(g_rccl_mu);
    if (g_rccl.lib) return nullptr;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return "librccl.so not found (dlopen)";
    RcclApi a;
    a.CommInitAll = (decltype(a.CommInitAll))dlsym(h, "ncclCommInitAll");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
    a.GroupStart = (decltype(a.GroupStart))dlsym(h, "ncclGroupStart");
    a.GroupEnd = (decltype(a.GroupEnd))dlsym(h, "ncclGroupEnd");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!a.CommInitAll || !a.CommDestroy || !a.AllReduce || !a.GroupStart || !a.GroupEnd || !a.GetErrorString)
        return "librccl.so lacks an expected symbol";
    a.lib = h;
    g_rccl = a;
    return nullptr;
}
}  // namespace

extern "C" {
int kidmp_shard_bounds(int64_t ncol, int32_t nshard, int32_t shard, int64_t *lo, int64_t *hi)
{
    if (ncol < 0 || nshard < 1 || shard < 0 || shard >= nshard || !lo || !hi) return fail(nullptr, KIDMP_EINVAL, "kidmp_shard_bounds: bad argument");
    const int64_t base = ncol / nshard, rem = ncol % nshard;               // contiguous ranges, sizes differ by at most one
    *lo = shard * base + (shard < rem ? shard : rem);
    *hi = *lo + base + (shard < rem ? 1 : 0);
    return KIDMP_OK;
}

void kidmp_finalize_multi(kidmp_multi *m)
{
    if (!m) return;
    for (ncclComm_t c : m->comm)
        if (c && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c);
    for (kidmp_ctx *c : m->ctx) kidmp_finalize(c);
    delete m;
}

int kidmp_init_multi(const kidmp_cfg *cfg, int32_t ndev, const int32_t *devices, kidmp_multi **out)
{
    if (!cfg || !out || !devices || ndev < 1 || ndev > KIDMP_MAX_DEVICE_LIST) return fail(nullptr, KIDMP_EINVAL, "kidmp_init_multi: bad argument (1..16 devices)");
    *out = nullptr;
    kidmp_multi *m = new (std::nothrow) kidmp_multi;
    if (!m) return fail(nullptr, KIDMP_ENOMEM, "kidmp_init_multi: out of host memory");
    for (int i = 0; i < ndev; ++i) {
        kidmp_cfg c = *cfg;
        c.device = devices[i];
        kidmp_ctx *x = nullptr;
        const int rc = kidmp_init(&c, &x);
        if (rc != KIDMP_OK) { kidmp_finalize_multi(m); return rc; }          // message already in g_err
        m->ctx.push_back(x);
        int l = -1;
        for (size_t q = 0; q < m->leader.size(); ++q)
            if (m->ctx[m->leader[q]]->cfg.device == devices[i]) l = int(q);
        if (l < 0) { m->leader.push_back(i); l = int(m->leader.size()) - 1; }
        m->leader_of.push_back(l);
    }
    // RCCL: one communicator per DISTINCT device (a list may name a device twice -- two contexts sharing a card, which
    // is how a one-GPU box exercises this path; their accumulators are added before the collective)
    if (const char *why = load_rccl()) { kidmp_finalize_multi(m); return fail(nullptr, KIDMP_ENODEV, std::string("kidmp_init_multi: ") + why); }
    std::vector<int> devs;
    for (int l : m->leader) devs.push_back(m->ctx[l]->cfg.device);
    m->comm.assign(devs.size(), nullptr);
    const ncclResult_t r = g_rccl.CommInitAll(m->comm.data(), int(devs.size()), devs.data());
    if (r != ncclSuccess) {
        const std::string msg = std::string("kidmp_init_multi: ncclCommInitAll: ") + g_rccl.GetErrorString(r);
        for (auto &c : m->comm) c = nullptr;
        kidmp_finalize_multi(m);
        return fail(nullptr, KIDMP_EHIP, msg);
    }
    *out = m;
    return KIDMP_OK;
}

int32_t kidmp_multi_size(const kidmp_multi *m) { return m ? int32_t(m->ctx.size()) : 0; }
kidmp_ctx *kidmp_multi_context(kidmp_multi *m, int32_t i) { return m && i >= 0 && size_t(i) < m->ctx.size() ? m->ctx[size_t(i)] : nullptr; }
const char *kidmp_multi_last_error(const kidmp_multi *m) { return m && !m->err.empty() ? m->err.c_str() : g_err.c_str(); }

int kidmp_batch_step_host_multi_diag(kidmp_multi *m, int64_t ncol, int32_t nz, double dt,
                                     double *qv, double *qc, double *qi, double *qr, double *qs, double *qg,
                                     double *ni, double *nr, double *nc, double *nwfa, double *nifa, double *t,
                                     const double *p, const double *w, const double *dz, double *ppt, double *rates,
                                     int32_t *nstep, double *precip_sums, double *sanity15)
{
    if (!m || m->ctx.empty()) return fail(m, KIDMP_ESTATE, "kidmp_batch_step_host_multi: not initialised");
    if (ncol < 0 || nz < 2 || nz > KIDMP_MAX_NZ) return fail(m, KIDMP_EINVAL, "kidmp_batch_step_host_multi: bad ncol / nz");
    const int nctx = int(m->ctx.size());
    for (kidmp_ctx *c : m->ctx)                                // sharding a per-column droplet number is not implemented
        if (c && c->d_nc_col) return fail(m, KIDMP_EINVAL, "kidmp_batch_step_host_multi: a member context holds a kidmp_set_column_nc binding");
    // Nothing below may throw through the C boundary: allocation failures (std::bad_alloc from the vectors, std::system_error
    // from std::thread) are mapped to a status code, and threads that did start are joined before the function returns.
    std::vector<int> rc;
    std::vector<std::string> msg;
    std::vector<int64_t> limbs, lead;
    std::vector<unsigned long long> san, san_lead;
    std::vector<std::thread> th;
    try {
        rc.assign(size_t(nctx), KIDMP_OK);
        msg.resize(size_t(nctx));
        limbs.resize(size_t(nctx) * ACC_N);
        lead.assign(m->leader.size() * ACC_N, 0);
        san.resize(size_t(nctx) * SANITY_N);
        san_lead.assign(m->leader.size() * SANITY_N, 0ull);
        th.reserve(size_t(nctx));
    } catch (const std::exception &) {
        return fail(m, KIDMP_ENOMEM, "kidmp_batch_step_host_multi: out of host memory");
    }
    auto work = [&](int i) noexcept {
        try {
            int64_t lo = 0, hi = 0;
            kidmp_shard_bounds(ncol, nctx, i, &lo, &hi);
            const size_t o = size_t(lo) * size_t(nz);
            auto at = [o](auto *a) { return a ? a + o : nullptr; };
            kidmp_ctx *c = m->ctx[size_t(i)];
            double *io[12] = {at(qv), at(qc), at(qi), at(qr), at(qs), at(qg), at(ni), at(nr), at(nc), at(nwfa), at(nifa), at(t)};
            const double *in[3] = {at(p), at(dz), at(w)};
            PipelineExtras<double> extra;
            extra.exact_sums = true;
            extra.scan_sanity = sanity15 != nullptr;
            rc[size_t(i)] = host_pipeline<double>(c, hi - lo, nz, dt, io, in, ppt ? ppt + 4 * lo : nullptr,
                rates ? rates + size_t(KIDMP_NRATES) * o : nullptr, nstep ? nstep + 4 * lo : nullptr, 0, extra);
            if (rc[size_t(i)] != KIDMP_OK) msg[size_t(i)] = kidmp_last_error(c);
        } catch (const std::bad_alloc &) {
            rc[size_t(i)] = KIDMP_ENOMEM;
        } catch (...) {
            rc[size_t(i)] = KIDMP_EHIP;
        }
    };
    // one host thread per context: HIP's current device and the pipeline's blocking waits are per thread
    int started = 0;
    bool thread_failure = false;
    for (int i = 1; i < nctx; ++i) {
        try {
            th.emplace_back(work, i);
            ++started;
        } catch (const std::exception &) {                     // std::system_error: no more threads
            thread_failure = true;
            break;
        }
    }
    if (!thread_failure) work(0);
    for (auto &x : th) x.join();
    if (thread_failure)
        return fail(m, KIDMP_ENOMEM, "kidmp_batch_step_host_multi: could not start a host thread per context (" +
                                      std::to_string(started) + " of " + std::to_string(nctx - 1) + " started, joined; nothing was stepped on the others)");
    for (int i = 0; i < nctx; ++i)
        if (rc[size_t(i)] != KIDMP_OK)
            return fail(m, rc[size_t(i)], "device " + std::to_string(m->ctx[size_t(i)]->cfg.device) + ": " +
                                           (msg[size_t(i)].empty() ? std::string("host-side failure in the context's worker thread") : msg[size_t(i)]));
    if (!precip_sums && !sanity15) return KIDMP_OK;
    // ---- the domain diagnostics: contexts that share a device combine their accumulators on the host, then the devices
    //      exchange them: all-reduce(int64, SUM) of the 24 precipitation limbs and -- on request, the analogue of the scan
    //      of M:1025-1094 -- all-reduce(uint64, MAX) of the 7 maxima (bit patterns of non-negative doubles order like the
    //      values) and all-reduce(uint64, SUM) of the 8 negative-entry counts, in ONE RCCL group ----
    // A leader's stream must be idle before this function returns on ANY path (queued collectives / copies).
    struct DrainLeaders {
        kidmp_multi *m;
        ~DrainLeaders()
        {
            for (int l : m->leader) {
                kidmp_ctx *c = m->ctx[size_t(l)];
                DeviceGuard g(c->cfg.device);
                (void)hipStreamSynchronize(c->stream);
            }
        }
    } drain_leaders{m};
    for (int i = 0; i < nctx; ++i) {
        kidmp_ctx *c = m->ctx[size_t(i)];
        DeviceGuard g(c->cfg.device);
        hipError_t e = hipMemcpy(&limbs[size_t(i) * ACC_N], c->d_acc, ACC_N * sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && sanity15) e = hipMemcpy(&san[size_t(i) * SANITY_N], c->d_sanity, SANITY_N * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(m, KIDMP_EHIP, std::string("hipMemcpy(accumulators): ") + hipGetErrorString(e));
        const size_t L = size_t(m->leader_of[size_t(i)]);
        for (int q = 0; q < ACC_N; ++q)                                    // wrap-around addition == two's complement sum
            lead[L * ACC_N + q] = int64_t(uint64_t(lead[L * ACC_N + q]) + uint64_t(limbs[size_t(i) * ACC_N + q]));
        if (sanity15)
            for (int q = 0; q < SANITY_N; ++q) {
                unsigned long long &sl = san_lead[L * SANITY_N + q];
                const unsigned long long v = san[size_t(i) * SANITY_N + q];
                sl = q < SANITY_MAX ? (v > sl ? v : sl) : sl + v;
            }
    }
    for (size_t l = 0; l < m->leader.size(); ++l) {                        // 192 + 120 bytes per device: synchronous copies,
        kidmp_ctx *c = m->ctx[size_t(m->leader[l])];                       // so that no DMA ever reads a host buffer after this scope
        DeviceGuard g(c->cfg.device);
        hipError_t e = hipMemcpy(c->d_acc, &lead[l * ACC_N], ACC_N * sizeof(int64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && sanity15) e = hipMemcpy(c->d_sanity, &san_lead[l * SANITY_N], SANITY_N * sizeof(unsigned long long), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(m, KIDMP_EHIP, std::string("hipMemcpy(accumulators, to device): ") + hipGetErrorString(e));
    }
    ncclResult_t r = g_rccl.GroupStart();
    for (size_t l = 0; l < m->leader.size() && r == ncclSuccess; ++l) {
        kidmp_ctx *c = m->ctx[size_t(m->leader[l])];
        DeviceGuard g(c->cfg.device);
        r = g_rccl.AllReduce(c->d_acc, c->d_acc, ACC_N, ncclInt64, ncclSum, m->comm[l], c->stream);
        if (r == ncclSuccess && sanity15) r = g_rccl.AllReduce(c->d_sanity, c->d_sanity, SANITY_MAX, ncclUint64, ncclMax, m->comm[l], c->stream);
        if (r == ncclSuccess && sanity15) r = g_rccl.AllReduce(c->d_sanity + SANITY_MAX, c->d_sanity + SANITY_MAX, SANITY_NEG, ncclUint64, ncclSum, m->comm[l], c->stream);
    }
    const ncclResult_t r2 = g_rccl.GroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess) return fail(m, KIDMP_EHIP, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r));
    int64_t total[ACC_N];
    unsigned long long stot[SANITY_N];
    for (size_t l = 0; l < m->leader.size(); ++l) {                        // every device holds the same results; all are drained
        kidmp_ctx *c = m->ctx[size_t(m->leader[l])];
        DeviceGuard g(c->cfg.device);
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && l == 0) e = hipMemcpy(total, c->d_acc, sizeof(total), hipMemcpyDeviceToHost);
        if (e == hipSuccess && l == 0 && sanity15) e = hipMemcpy(stot, c->d_sanity, sizeof(stot), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(m, KIDMP_EHIP, std::string("all-reduce of the domain diagnostics: ") + hipGetErrorString(e));
    }
    if (precip_sums) (void)kidmp_ppt_limbs_to_sums(total, precip_sums);
    if (sanity15)
        for (int q = 0; q < SANITY_N; ++q) {
            double v;
            if (q < SANITY_MAX) memcpy(&v, &stot[q], sizeof(v)); else v = double(stot[q]);
            sanity15[q] = v;
        }
    return KIDMP_OK;
}

int kidmp_batch_step_host_multi(kidmp_multi *m, int64_t ncol, int32_t nz, double dt,
                                double *qv, double *qc, double *qi, double *qr, double *qs, double *qg,
                                double *ni, double *nr, double *nc, double *nwfa, double *nifa, double *t,
                                const double *p, const double *w, const double *dz, double *ppt, double *rates,
                                int32_t *nstep, double *precip_sums)
{
    return kidmp_batch_step_host_multi_diag(m, ncol, nz, dt, qv, qc, qi, qr, qs, qg, ni, nr, nc, nwfa, nifa, t, p, w, dz, ppt, rates, nstep, precip_sums, nullptr);
}
}  // extern "C"
