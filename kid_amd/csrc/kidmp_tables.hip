// kidmp_tables.hip -- read-back of the lookup tables and scheme constants by name, and the table-cache files of
// thompson_init (qr_acr_qg / qr_acr_qs): save, load, and the reference's reuse-or-build policy.
#include <sys/stat.h>
#include <cstdio>

#include "kidmp_ctx.h"
#include "table_cache.h"

using namespace kidmp;

namespace {
struct Named { const char *name; const double *ptr; int64_t n; };
std::vector<Named> table_dir(const Tables &t)
{
    return {
        {"tcg_racg", t.tcg_racg, N_RACG}, {"tmr_racg", t.tmr_racg, N_RACG}, {"tcr_gacr", t.tcr_gacr, N_RACG},
        {"tmg_gacr", t.tmg_gacr, N_RACG}, {"tnr_racg", t.tnr_racg, N_RACG}, {"tnr_gacr", t.tnr_gacr, N_RACG},
        {"tcs_racs1", t.tcs_racs1, N_RACS}, {"tmr_racs1", t.tmr_racs1, N_RACS}, {"tcs_racs2", t.tcs_racs2, N_RACS},
        {"tmr_racs2", t.tmr_racs2, N_RACS}, {"tcr_sacr1", t.tcr_sacr1, N_RACS}, {"tms_sacr1", t.tms_sacr1, N_RACS},
        {"tcr_sacr2", t.tcr_sacr2, N_RACS}, {"tms_sacr2", t.tms_sacr2, N_RACS}, {"tnr_racs1", t.tnr_racs1, N_RACS},
        {"tnr_racs2", t.tnr_racs2, N_RACS}, {"tnr_sacr1", t.tnr_sacr1, N_RACS}, {"tnr_sacr2", t.tnr_sacr2, N_RACS},
        {"tpi_qcfz", t.tpi_qcfz, N_QCFZ}, {"tni_qcfz", t.tni_qcfz, N_QCFZ},
        {"tpi_qrfz", t.tpi_qrfz, N_QRFZ}, {"tpg_qrfz", t.tpg_qrfz, N_QRFZ}, {"tni_qrfz", t.tni_qrfz, N_QRFZ},
        {"tnr_qrfz", t.tnr_qrfz, N_QRFZ},
        {"tps_iaus", t.tps_iaus, N_IAUS}, {"tni_iaus", t.tni_iaus, N_IAUS}, {"tpi_ide", t.tpi_ide, N_IAUS},
        {"t_Efrw", t.t_Efrw, N_EF}, {"t_Efsw", t.t_Efsw, N_EF}, {"tnc_wev", t.tnc_wev, N_WEV},
        {"racs_rec", t.racs_rec, N_RACS * RACS_REC}, {"racg_rec", t.racg_rec, N_RACG * RACG_REC},
        {"qrfz_rec", t.qrfz_rec, N_QRFZ * QRFZ_REC},
    };
}

std::vector<Named> const_dir(const kidmp_ctx *c)
{
    const Consts &h = c->hc;
    const Bins &b = c->hb;
    return {
        {"Nt_c", &h.Nt_c, 1}, {"Sc3", &h.Sc3, 1}, {"D0i", &h.D0i, 1}, {"xm0s", &h.xm0s, 1}, {"xm0g", &h.xm0g, 1},
        {"cce1", h.cce[0], 15}, {"cce2", h.cce[1], 15}, {"cce3", h.cce[2], 15}, {"cce4", h.cce[3], 15}, {"cce5", h.cce[4], 15},
        {"ccg1", h.ccg[0], 15}, {"ccg2", h.ccg[1], 15}, {"ccg3", h.ccg[2], 15}, {"ccg4", h.ccg[3], 15}, {"ccg5", h.ccg[4], 15},
        {"ocg1", h.ocg1, 15}, {"ocg2", h.ocg2, 15},
        {"cie", h.cie, 7}, {"cig", h.cig, 7}, {"oig1", &h.oig1, 1}, {"oig2", &h.oig2, 1}, {"obmi", &h.obmi, 1},
        {"cre", h.cre, 13}, {"crg", h.crg, 13}, {"ore1", &h.ore1, 1}, {"org1", &h.org1, 1}, {"org2", &h.org2, 1},
        {"org3", &h.org3, 1}, {"obmr", &h.obmr, 1},
        {"cse", h.cse, 18}, {"csg", h.csg, 18}, {"oams", &h.oams, 1}, {"obms", &h.obms, 1}, {"ocms", &h.ocms, 1},
        {"cge", h.cge, 12}, {"cgg", h.cgg, 12}, {"oge1", &h.oge1, 1}, {"ogg1", &h.ogg1, 1}, {"ogg2", &h.ogg2, 1},
        {"ogg3", &h.ogg3, 1}, {"oamg", &h.oamg, 1}, {"obmg", &h.obmg, 1}, {"ocmg", &h.ocmg, 1},
        {"t1_qr_qc", &h.t1_qr_qc, 1}, {"t1_qr_qi", &h.t1_qr_qi, 1}, {"t2_qr_qi", &h.t2_qr_qi, 1},
        {"t1_qg_qc", &h.t1_qg_qc, 1}, {"t1_qs_qc", &h.t1_qs_qc, 1}, {"t1_qs_qi", &h.t1_qs_qi, 1},
        {"t1_qr_ev", &h.t1_qr_ev, 1}, {"t2_qr_ev", &h.t2_qr_ev, 1}, {"t1_qs_sd", &h.t1_qs_sd, 1},
        {"t2_qs_sd", &h.t2_qs_sd, 1}, {"t1_qg_sd", &h.t1_qg_sd, 1}, {"t2_qg_sd", &h.t2_qg_sd, 1},
        {"t1_qs_me", &h.t1_qs_me, 1}, {"t2_qs_me", &h.t2_qs_me, 1}, {"t1_qg_me", &h.t1_qg_me, 1},
        {"t2_qg_me", &h.t2_qg_me, 1},
        {"Dc", b.Dc, nbins}, {"dtc", b.dtc, nbins}, {"Di", b.Di, nbins}, {"dti", b.dti, nbins},
        {"Dr", b.Dr, nbins}, {"dtr", b.dtr, nbins}, {"Ds", b.Ds, nbins}, {"dts", b.dts, nbins},
        {"Dg", b.Dg, nbins}, {"dtg", b.dtg, nbins}, {"t_Nc", b.t_Nc, nbins},
        {"r_c", b.r_c, ntb_c}, {"r_i", b.r_i, ntb_i}, {"r_r", b.r_r, ntb_r}, {"r_g", b.r_g, ntb_g},
        {"r_s", b.r_s, ntb_s}, {"N0r_exp", b.N0r_exp, ntb_r1}, {"N0g_exp", b.N0g_exp, ntb_g1}, {"Nt_i", b.Nt_i, ntb_i1},
    };
}

struct CacheFamily { const char *file; std::vector<double *> dev; int64_t n; };
std::vector<CacheFamily> cache_families(Tables &t)
{
    return {
        {"racg_thompson09.data", {t.tcg_racg, t.tmr_racg, t.tcr_gacr, t.tmg_gacr, t.tnr_racg, t.tnr_gacr}, N_RACG},   // M:3823-3828
        {"racs_thompson09.data", {t.tcs_racs1, t.tmr_racs1, t.tcs_racs2, t.tmr_racs2, t.tcr_sacr1, t.tms_sacr1,
                                  t.tcr_sacr2, t.tms_sacr2, t.tnr_racs1, t.tnr_racs2, t.tnr_sacr1, t.tnr_sacr2}, N_RACS},   // M:4066-4077
    };
}

// device -> host -> file
int save_family(kidmp_ctx *ctx, const CacheFamily &fam, const std::string &path)
{
    std::vector<std::vector<double>> host(fam.dev.size(), std::vector<double>(size_t(fam.n)));
    std::vector<const double *> ptr;
    for (size_t i = 0; i < fam.dev.size(); ++i) {
        HIPTRY(ctx, hipMemcpy(host[i].data(), fam.dev[i], size_t(fam.n) * sizeof(double), hipMemcpyDeviceToHost));
        ptr.push_back(host[i].data());
    }
    if (cache_write(path.c_str(), int(ptr.size()), ptr.data(), fam.n) != 0) return fail(ctx, KIDMP_EIO, "cannot write " + path);
    return KIDMP_OK;
}

// file -> host -> device; the caller runs repack_records once its families are in
int load_family(kidmp_ctx *ctx, const CacheFamily &fam, const std::string &path)
{
    std::vector<std::vector<double>> host(fam.dev.size(), std::vector<double>(size_t(fam.n)));
    std::vector<double *> ptr;
    for (auto &h : host) ptr.push_back(h.data());
    const int rc = cache_read(path.c_str(), int(ptr.size()), ptr.data(), fam.n);
    if (rc != 0) return fail(ctx, KIDMP_EIO, (rc == -1 ? "cannot open " : "malformed or short table cache ") + path);
    for (size_t i = 0; i < fam.dev.size(); ++i)
        HIPTRY(ctx, hipMemcpy(fam.dev[i], host[i].data(), size_t(fam.n) * sizeof(double), hipMemcpyHostToDevice));
    return KIDMP_OK;
}
}  // namespace

extern "C" {
int64_t kidmp_get_table(kidmp_ctx *ctx, const char *name, double *out, int64_t cap)
{
    if (int rc = require_ready(ctx, "kidmp_get_table: bad context", name != nullptr)) return rc;
    GUARD(ctx);
    for (const Named &e : table_dir(ctx->tables))
        if (!strcmp(e.name, name)) {
            if (!out) return e.n;
            if (cap < e.n) return fail(ctx, KIDMP_EINVAL, "kidmp_get_table: buffer too small");
            HIPTRY(ctx, hipMemcpy(out, e.ptr, size_t(e.n) * sizeof(double), hipMemcpyDeviceToHost));
            return e.n;
        }
    return fail(ctx, KIDMP_EINVAL, std::string("kidmp_get_table: unknown table ") + name);
}
int64_t kidmp_get_const(kidmp_ctx *ctx, const char *name, double *out, int64_t cap)
{
    if (int rc = require_ready(ctx, "kidmp_get_const: bad context", name != nullptr)) return rc;
    for (const Named &e : const_dir(ctx))
        if (!strcmp(e.name, name)) {
            if (!out) return e.n;
            if (cap < e.n) return fail(ctx, KIDMP_EINVAL, "kidmp_get_const: buffer too small");
            memcpy(out, e.ptr, size_t(e.n) * sizeof(double));
            return e.n;
        }
    return fail(ctx, KIDMP_EINVAL, std::string("kidmp_get_const: unknown constant ") + name);
}

int kidmp_cache_write_file(const char *path, int32_t ntab, const double *const *tabs, int64_t n_each)
{
    if (!path || !tabs || ntab <= 0 || n_each <= 0) return fail(nullptr, KIDMP_EINVAL, "kidmp_cache_write_file: bad argument");
    return cache_write(path, ntab, tabs, n_each) == 0 ? KIDMP_OK : fail(nullptr, KIDMP_EIO, std::string("cannot write ") + path);
}
int kidmp_cache_read_file(const char *path, int32_t ntab, double *const *tabs, int64_t n_each)
{
    if (!path || !tabs || ntab <= 0 || n_each <= 0) return fail(nullptr, KIDMP_EINVAL, "kidmp_cache_read_file: bad argument");
    const int rc = cache_read(path, ntab, tabs, n_each);
    if (rc != 0) return fail(nullptr, KIDMP_EIO, std::string(rc == -1 ? "cannot open " : "malformed or short table cache ") + path);
    return KIDMP_OK;
}

int kidmp_save_table_cache(kidmp_ctx *ctx, const char *dir)
{
    if (int rc = require_ready(ctx, "kidmp_save_table_cache: bad context", dir != nullptr)) return rc;
    if (ctx->hc.iiwarm) return fail(ctx, KIDMP_ESTATE, "kidmp_save_table_cache: iiwarm context has no mixed-phase tables");
    GUARD(ctx);
    for (const CacheFamily &fam : cache_families(ctx->tables))
        if (int rc = save_family(ctx, fam, std::string(dir) + "/" + fam.file)) return rc;
    return KIDMP_OK;
}

// thompson_init's use of the cache files, per file as in the reference: qr_acr_qg (M:3717-3729, M:3822-3829) and
// qr_acr_qs (M:3864-3895, M:4065-4078) each do
//     inquire(file=..., exist=fexist);  fexist = fexist .and. l_reuse_thompson_lookup
//     if (fexist) then  read the 6 (12) tables  else  compute them and write(12,*) / write(13,*) them
int kidmp_table_cache_reuse(kidmp_ctx *ctx, const char *dir, int32_t l_reuse, int32_t write_if_built, int32_t *status)
{
    if (status) *status = 0;
    if (int rc = require_ready(ctx, "kidmp_table_cache_reuse: bad context", dir != nullptr)) return rc;
    if (ctx->hc.iiwarm) return KIDMP_OK;                     // thompson_init builds these tables only if .not. iiwarm (M:773)
    GUARD(ctx);
    struct stat sb;
    const bool have_dir = stat(dir, &sb) == 0 && S_ISDIR(sb.st_mode);
    bool loaded = false;
    int fam_no = 0;
    for (const CacheFamily &fam : cache_families(ctx->tables)) {
        const std::string path = std::string(dir) + "/" + fam.file;
        bool fexist = false;
        if (FILE *f = std::fopen(path.c_str(), "r")) { fexist = true; std::fclose(f); }
        if (fexist && l_reuse) {
            if (int rc = load_family(ctx, fam, path)) return rc;
            loaded = true;
            if (status) *status |= 1 << fam_no;
        } else if (write_if_built && have_dir) {
            // the reference opens the file unconditionally and aborts without the directory (M:3718); here a missing
            // directory just means nothing is written (reported through *status)
            if (int rc = save_family(ctx, fam, path)) return rc;
            if (status) *status |= 4 << fam_no;
        }
        ++fam_no;
    }
    if (loaded) HIPTRY(ctx, repack_records(ctx->tables, ctx->stream));   // the solver reads the interleaved records
    return KIDMP_OK;
}

int kidmp_load_table_cache(kidmp_ctx *ctx, const char *dir)
{
    if (int rc = require_ready(ctx, "kidmp_load_table_cache: bad context", dir != nullptr)) return rc;
    if (ctx->hc.iiwarm) return fail(ctx, KIDMP_ESTATE, "kidmp_load_table_cache: iiwarm context has no mixed-phase tables");
    GUARD(ctx);
    for (const CacheFamily &fam : cache_families(ctx->tables))
        if (int rc = load_family(ctx, fam, std::string(dir) + "/" + fam.file)) return rc;
    HIPTRY(ctx, repack_records(ctx->tables, ctx->stream));       // the solver reads the interleaved records
    return KIDMP_OK;
}
}  // extern "C"
