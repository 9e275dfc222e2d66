// stage_plan_check.cpp -- kid_amd/csrc/kidmp_stage_plan.h as a host program: the arithmetic that cuts a host-array call of
// the diagnostics into column chunks and the staging memory into slots, enumerated directly.
//   1. properties over a sweep of shapes, chunk settings, element sizes, strides and present/absent arrays: slots aligned,
//      disjoint and inside the planned total; chunks tiling [0, ncol) once and in order; every copy's host range inside the
//      array and its staged range inside its slot.  The copies are carried out with memcpy on buffers of exactly the arrays'
//      extents (so that a sanitizer sees any overrun) and the bytes that arrive are compared on both sides.
//   2. per entry, one representative call: chunk and staging bytes equal the formula the entry had before it was moved onto
//      the plan, written out longhand here.
//   3. the caps: a call too large for its entry's cap gets the largest chunk, at least 1, that fits.
// Prints "stage plan ok" and returns 0, or says what failed and returns 1.
#include "kidmp_stage_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace kidmp;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                                                                      std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// ---- 1. properties ----
// the host extent of an array in bytes, as the C ABI states it
static size_t extent(const StageArray &a, int64_t ncol)
{
    if (a.once) return size_t(a.per_col) * a.elem;
    const size_t slab = a.col_stride == 0 ? size_t(a.per_col) : size_t(ncol - 1) * size_t(a.col_stride) + size_t(a.per_col);
    return (size_t(a.nslab - 1) * size_t(a.slab_stride) + slab) * a.elem;
}
static unsigned char host_byte(int i, size_t off) { return (unsigned char)(17 * i + 31 * off + 7); }
static unsigned char dev_byte(int i, int slab, int64_t col, size_t b) { return (unsigned char)(13 * i + 5 * slab + 3 * col + 11 * b + 1); }

static void run_case(StageArray *a, int na, int64_t ncol, int64_t chunk_setting, const char *what)
{
    const StagePlan plan = stage_plan(a, na, ncol, stage_pick_chunk(chunk_setting, ncol));
    CHECK(plan.chunk >= 1 && plan.chunk <= ncol, "%s: chunk %lld of %lld", what, (long long)plan.chunk, (long long)ncol);
    if (chunk_setting > 0) CHECK(plan.chunk == (chunk_setting < ncol ? chunk_setting : ncol), "%s: chunk setting", what);
    // slots: aligned, pairwise disjoint, inside the total
    for (int i = 0; i < na; ++i) {
        if (!stage_has_slot(a[i])) { CHECK(!a[i].host, "%s: array %d present without a slot", what, i); continue; }
        const size_t end = a[i].offset + size_t(a[i].nslab) * a[i].slab_bytes;
        CHECK(a[i].offset % 256 == 0 && a[i].slab_bytes % 256 == 0, "%s: slot %d not aligned", what, i);
        CHECK(end <= plan.total, "%s: slot %d ends at %zu past %zu", what, i, end, plan.total);
        for (int j = 0; j < i; ++j) {
            if (!stage_has_slot(a[j])) continue;
            const size_t endj = a[j].offset + size_t(a[j].nslab) * a[j].slab_bytes;
            CHECK(end <= a[j].offset || endj <= a[i].offset, "%s: slots %d and %d overlap", what, i, j);
        }
    }
    // the arrays and the staging memory, of exactly their sizes
    std::vector<std::vector<unsigned char>> host(na);
    for (int i = 0; i < na; ++i) {
        if (!a[i].host) continue;
        host[i].resize(extent(a[i], ncol));
        for (size_t b = 0; b < host[i].size(); ++b) host[i][b] = host_byte(i, b);
    }
    std::vector<unsigned char> stage(plan.total, 0);
    std::vector<int> visits(size_t(ncol), 0);
    // one copy, range-checked, then carried out
    auto move = [&](int i, int s, bool down, int64_t c0, int64_t n) {
        const StageCopy c = stage_copy(a[i], s, c0, n);
        const size_t slot0 = a[i].offset + size_t(s) * a[i].slab_bytes;
        CHECK(c.rows >= 1 && c.host_off + (c.rows - 1) * c.host_pitch + c.row_bytes <= host[i].size(), "%s: array %d slab %d chunk %lld: host range", what,
              i, s, (long long)c0);
        CHECK(c.stage_off >= slot0 && c.stage_off + c.rows * c.row_bytes <= slot0 + a[i].slab_bytes, "%s: array %d slab %d chunk %lld: staged range",
              what, i, s, (long long)c0);
        if (failures) return;
        for (size_t r = 0; r < c.rows; ++r) {
            unsigned char *h = host[i].data() + c.host_off + r * c.host_pitch, *d = stage.data() + c.stage_off + r * c.row_bytes;
            if (down) std::memcpy(h, d, c.row_bytes);
            else std::memcpy(d, h, c.row_bytes);
        }
    };
    auto moves = [&](bool down, bool before, int64_t c0, int64_t n) {
        for (int i = 0; i < na; ++i)
            if (a[i].host && (a[i].dir & (down ? STAGE_DOWN : STAGE_UP)) && stage_before_loop(a[i]) == before)
                for (int s = 0; s < a[i].nslab; ++s) move(i, s, down, c0, n);
    };
    moves(false, true, 0, 0);
    int64_t expect_c0 = 0;
    for (int64_t c0 = 0; c0 < plan.ncol; c0 += plan.chunk) {
        const int64_t n = stage_chunk_cols(plan, c0);
        CHECK(c0 == expect_c0 && n >= 1 && n <= plan.chunk && c0 + n <= ncol, "%s: chunk [%lld, +%lld)", what, (long long)c0, (long long)n);
        expect_c0 = c0 + n;
        for (int64_t c = c0; c < c0 + n; ++c) ++visits[size_t(c)];
        moves(false, false, c0, n);
        if (failures) return;
        for (int i = 0; i < na; ++i) {
            if (!a[i].host) continue;
            const size_t row = size_t(a[i].per_col) * a[i].elem;
            for (int s = 0; s < a[i].nslab; ++s) {
                unsigned char *slab = stage.data() + a[i].offset + size_t(s) * a[i].slab_bytes;
                const size_t hbase = size_t(s) * size_t(a[i].slab_stride) * a[i].elem;
                // what went up is the chunk's rows, packed (one row for all columns where the array is shared or `once`)
                if (a[i].dir & STAGE_UP)
                    for (int64_t j = 0; j < (stage_before_loop(a[i]) ? 1 : n); ++j)
                        for (size_t b = 0; b < row; ++b) {
                            const size_t hoff = hbase + (stage_before_loop(a[i]) ? 0 : size_t(c0 + j) * size_t(a[i].col_stride) * a[i].elem) + b;
                            CHECK(slab[size_t(j) * row + b] == host_byte(i, hoff), "%s: array %d slab %d column %lld: staged bytes", what, i, s,
                                  (long long)(c0 + j));
                            if (failures) return;
                        }
                // the kernel's stand-in fills what comes down
                if (a[i].dir & STAGE_DOWN)
                    for (int64_t j = 0; j < n; ++j)
                        for (size_t b = 0; b < row; ++b) slab[size_t(j) * row + b] = dev_byte(i, s, c0 + j, b);
            }
        }
        moves(true, false, c0, n);
    }
    CHECK(expect_c0 == ncol, "%s: the chunks end at %lld", what, (long long)expect_c0);
    for (int64_t c = 0; c < ncol; ++c) CHECK(visits[size_t(c)] == 1, "%s: column %lld visited %d times", what, (long long)c, visits[size_t(c)]);
    for (int i = 0; i < na; ++i) {
        if (!a[i].host || !(a[i].dir & STAGE_DOWN)) continue;
        const size_t row = size_t(a[i].per_col) * a[i].elem;
        for (int s = 0; s < a[i].nslab; ++s)
            for (int64_t c = 0; c < ncol; ++c)
                for (size_t b = 0; b < row; ++b) {
                    const size_t hoff = (size_t(s) * size_t(a[i].slab_stride) + size_t(c) * size_t(a[i].col_stride)) * a[i].elem + b;
                    CHECK(host[i][hoff] == dev_byte(i, s, c, b), "%s: array %d slab %d column %lld: bytes that came down", what, i, s, (long long)c);
                    if (failures) return;
                }
    }
}

template <class T> static void sweep()
{
    static const T dummy = T(0);                              // presence is all a host pointer means to the plan
    const int64_t ncols[] = {1, 2, 7, 100}, nzs[] = {2, 5, 100};
    constexpr int NA = 11, NB = 3, NCH = 3;
    for (int64_t ncol : ncols)
        for (int64_t nz : nzs)
            for (int64_t setting : {int64_t(0), int64_t(1), int64_t(2), int64_t(3), int64_t(7), int64_t(16), ncol})
                for (int variant = 0; variant < 3; ++variant)
                    for (int absent = -1; absent <= NA; ++absent) {   // -1: all present; 1 .. NA-1: that one absent; NA: every optional one
                        if (absent == 0) continue;                    // array 0 is required
                        const int64_t dz_stride = variant == 0 ? 0 : variant == 1 ? nz : nz + 5, kg_stride = variant == 0 ? nz + 5 : variant == 1 ? 0 : nz;
                        const int64_t kg_slab = kg_stride ? (ncol - 1) * kg_stride + nz + 3 : nz;   // (a channel stride may exceed the slab)
                        static const double grid = 0.;
                        static const int32_t steps = 0;
                        StageArray a[NA] = {
                            stage_array(&dummy, nz, STAGE_UP),
                            stage_array(&dummy, nz, STAGE_UP),
                            stage_rows(&dummy, nz, dz_stride),
                            stage_slabs(stage_rows(&dummy, nz, kg_stride), NCH, kg_slab),
                            stage_once(&grid, NB),
                            stage_slabs(stage_array(&dummy, nz, STAGE_DOWN), NCH, ncol * nz),
                            stage_slabs(stage_array(&dummy, 1, STAGE_DOWN), NCH, ncol),
                            stage_array(&steps, 4, STAGE_DOWN),
                            stage_array(&grid, 6, STAGE_DOWN),
                            stage_array(&dummy, NB * nz, STAGE_DOWN),
                            stage_keep(stage_array(&dummy, nz, STAGE_BOTH)),
                        };
                        for (int i = 1; i < NA; ++i)
                            if (i == absent || absent == NA) a[i].host = nullptr;
                        char what[160];
                        std::snprintf(what, sizeof(what), "elem %zu ncol %lld nz %lld chunk %lld variant %d absent %d", sizeof(T), (long long)ncol,
                                      (long long)nz, (long long)setting, variant, absent);
                        run_case(a, NA, ncol, setting, what);
                        if (failures) return;
                    }
}

// ---- 2. the entries' former arithmetic, longhand ----
constexpr int64_t NCOL = 7, NZ = 5;
constexpr int SUMMARY_N = 16, LIDAR_SUMMARY_N = 8, NBINS = 100;        // KIDMP_SUMMARY_N, KIDMP_LIDAR_SUMMARY_N, the scheme's own bins
constexpr size_t MiB256 = size_t(256) << 20, GiB1 = size_t(1) << 30;
static const int32_t I32 = 0;
static const double F64 = 0.;

static int64_t old_pick(int64_t host_chunk, int64_t ncol)
{
    if (host_chunk > 0) return host_chunk < ncol ? host_chunk : ncol;
    if (ncol <= 2048) return ncol;
    int64_t ch = (ncol + 3) / 4;
    ch = (ch + 255) / 256 * 256;
    return ch > 8192 ? 8192 : ch;
}
static void same(const char *entry, int64_t setting, size_t elem, const StagePlan &plan, int64_t old_ch, size_t old_bytes)
{
    CHECK(plan.chunk == old_ch && plan.total == old_bytes, "%s, chunk setting %lld, %zu-byte elements: chunk %lld (was %lld), %zu bytes (was %zu)", entry,
          (long long)setting, elem, (long long)plan.chunk, (long long)old_ch, plan.total, old_bytes);
}

template <class T> static void parent_equality(int64_t setting)
{
    static const T X = T(0);
    const T *const x = &X;
    const size_t E = sizeof(T);
    const int64_t CH = old_pick(setting, NCOL);
    const size_t b_prof = up256(size_t(CH) * size_t(NZ) * E), b_col = up256(size_t(CH) * E);
    auto ups = [&](StageArray *a, int n) { for (int v = 0; v < n; ++v) a[v] = stage_array(x, NZ, STAGE_UP); };
    auto downs = [&](StageArray *a, int n) { for (int v = 0; v < n; ++v) a[v] = stage_array(x, NZ, STAGE_DOWN); };
    {   // refl_host: eight slots whatever is given; qs and qg left out
        StageArray a[8];
        ups(a, 7);
        for (int v = 0; v < 7; ++v) a[v] = stage_keep(a[v]);
        a[5].host = a[6].host = nullptr;
        downs(a + 7, 1);
        same("reflectivity", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL)), CH, 8 * b_prof);
    }
    {   // radii_host: n = NCOL*NZ elements, the context's chunk, else 8192, times 128; eleven slots whatever is given
        const int64_t n = NCOL * NZ, want = (setting > 0 ? setting : 8192) * 128, ch = want < n ? want : n;
        StageArray a[11];
        for (int v = 0; v < 11; ++v) a[v] = stage_keep(stage_array(v == 4 || v == 9 ? nullptr : x, 1, v < 8 ? STAGE_UP : STAGE_BOTH));
        same("effective radii", setting, E, stage_plan(a, n, ch), ch, 11 * up256(size_t(ch) * E));
    }
    {   // summary_host: ten profile slots whatever is given, dz (per column, padded), the summary
        StageArray a[12];
        ups(a, 10);
        for (int v = 0; v < 10; ++v) a[v] = stage_keep(a[v]);
        a[4].host = nullptr;
        a[10] = stage_rows(x, NZ, NZ + 5);
        a[11] = stage_array(&F64, SUMMARY_N, STAGE_DOWN);
        same("column summary", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL)), CH,
             11 * b_prof + up256(size_t(CH) * SUMMARY_N * sizeof(double)));
    }
    {   // fall_host with nstep: ten inputs, dz, eleven outputs, nstep
        StageArray a[23];
        ups(a, 10);
        a[10] = stage_rows(x, NZ, 0);
        downs(a + 11, 11);
        a[22] = stage_array(&I32, 4, STAGE_DOWN);
        same("fall speeds", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL)), CH, 22 * b_prof + up256(size_t(CH) * 4 * sizeof(int32_t)));
    }
    {   // doppler_host: eight inputs, nine outputs
        StageArray a[17];
        ups(a, 8);
        downs(a + 8, 9);
        same("doppler moments", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL)), CH, 17 * b_prof);
    }
    {   // spectra_host: eleven inputs, eleven parameters, five spectra, the caller's grids of 7 and 12 bins for two of them
        const int nb[5] = {NBINS, 7, NBINS, 12, NBINS};
        const bool own[5] = {false, true, false, true, false};
        StageArray a[37];
        size_t per_col = 22 * size_t(NZ) * E, b_grids = 0;
        for (int s = 0; s < 5; ++s) {
            a[s] = stage_once(own[s] ? &F64 : nullptr, nb[s]);
            a[5 + s] = stage_once(own[s] ? &F64 : nullptr, nb[s]);
            a[32 + s] = stage_array(x, int64_t(nb[s]) * NZ, STAGE_DOWN);
            per_col += size_t(nb[s]) * size_t(NZ) * E;
            if (own[s]) b_grids += 2 * up256(size_t(nb[s]) * sizeof(double));
        }
        ups(a + 10, 11);
        downs(a + 21, 11);
        int64_t ch = CH;
        const int64_t fit = int64_t(MiB256 / per_col);
        if (ch > fit) ch = fit > 0 ? fit : 1;
        size_t need = b_grids + 22 * up256(size_t(ch) * size_t(NZ) * E);
        for (int s = 0; s < 5; ++s) need += up256(size_t(ch) * size_t(nb[s]) * size_t(NZ) * E);
        same("size spectra", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL), MiB256), ch, need);
    }
    {   // dspectrum_host: eight inputs, four spectra of nv bins and two profiles, the caller's grids of 7 and 12 bins
        const int nv = 9, nb[3] = {7, NBINS, 12};
        const bool own[3] = {true, false, true};
        StageArray a[20];
        size_t per_col = 8 * size_t(NZ) * E + (4 * size_t(nv) + 2) * size_t(NZ) * E, b_grids = 0;
        for (int s = 0; s < 3; ++s) {
            a[s] = stage_once(own[s] ? &F64 : nullptr, nb[s]);
            a[3 + s] = stage_once(own[s] ? &F64 : nullptr, nb[s]);
            if (own[s]) b_grids += 2 * up256(size_t(nb[s]) * sizeof(double));
        }
        ups(a + 6, 8);
        for (int v = 0; v < 6; ++v) a[14 + v] = stage_array(x, int64_t(v < 4 ? nv : 1) * NZ, STAGE_DOWN);
        int64_t ch = CH;
        const int64_t fit = int64_t((MiB256 - b_grids - 256 * size_t(8 + 6)) / per_col);
        if (ch > fit) ch = fit > 0 ? fit : 1;
        const size_t need = b_grids + 8 * up256(size_t(ch) * size_t(NZ) * E) + 4 * up256(size_t(ch) * size_t(nv) * size_t(NZ) * E)
                            + 2 * up256(size_t(ch) * size_t(NZ) * E);
        same("doppler spectrum", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL), MiB256), ch, need);
    }
    {   // lidar_host with the summary and a per-column dz: eleven inputs, dz, fourteen profiles, the summary
        StageArray a[27];
        ups(a, 11);
        a[11] = stage_rows(x, NZ, NZ + 5);
        downs(a + 12, 14);
        a[26] = stage_array(&F64, LIDAR_SUMMARY_N, STAGE_DOWN);
        same("lidar", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL)), CH,
             26 * b_prof + up256(size_t(CH) * LIDAR_SUMMARY_N * sizeof(double)));
    }
    {   // brightband_host with k0 and the caller's grids (9 and 14 bins): seven inputs, seven outputs, k0
        const int nb[2] = {9, 14};
        StageArray a[19];
        for (int s = 0; s < 2; ++s) { a[s] = stage_once(&F64, nb[s]); a[2 + s] = stage_once(&F64, nb[s]); }
        ups(a + 4, 7);
        downs(a + 11, 7);
        a[18] = stage_array(&I32, 1, STAGE_DOWN);
        same("bright band", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL)), CH,
             up256(size_t(CH) * sizeof(int32_t)) + 14 * b_prof + 2 * up256(9 * sizeof(double)) + 2 * up256(14 * sizeof(double)));
    }
    {   // pol_host: seven inputs, thirteen outputs
        StageArray a[20];
        ups(a, 7);
        downs(a + 7, 13);
        same("polarimetric", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL)), CH, 20 * b_prof);
    }
    // the channel entries, one channel and three: inputs, dz, (w,) k_gas per column (and per channel), the outputs' slabs
    for (int nch : {1, 3}) {
        const int64_t kg_slab = (NCOL - 1) * (NZ + 5) + NZ;
        {   // mie_host / mie_multi_host: eight inputs, dz, w, k_gas, thirteen profiles, pia_total
            StageArray a[25];
            ups(a, 8);
            a[8] = stage_rows(x, NZ, 0);
            a[9] = stage_array(x, NZ, STAGE_UP);
            a[10] = stage_slabs(stage_rows(x, NZ, NZ + 5), nch, nch > 1 ? kg_slab : 0);
            for (int v = 0; v < 13; ++v) a[11 + v] = stage_slabs(stage_array(x, NZ, STAGE_DOWN), nch, NCOL * NZ);
            a[24] = stage_slabs(stage_array(x, 1, STAGE_DOWN), nch, NCOL);
            const size_t profs = 1 + 1 + size_t(nch) + 8 + 13 * size_t(nch), cols = size_t(nch);
            int64_t ch = CH;                                  // (Stager::open: halve until it fits)
            size_t bp, bc;
            for (;;) {
                bp = up256(size_t(ch) * size_t(NZ) * E);
                bc = up256(size_t(ch) * E);
                if (profs * bp + cols * bc <= GiB1 || ch == 1) break;
                ch = (ch + 1) / 2;
            }
            same(nch > 1 ? "cloud radar, 3 channels" : "cloud radar", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL), nch > 1 ? GiB1 : 0), ch,
                 profs * bp + cols * bc);
        }
        {   // rad_host / rad_multi_host: eight inputs, dz, k_gas, six profiles, t_sfc, the three column outputs
            StageArray a[20];
            ups(a, 8);
            a[8] = stage_rows(x, NZ, NZ + 5);
            a[9] = stage_slabs(stage_rows(x, NZ, NZ + 5), nch, nch > 1 ? kg_slab : 0);
            for (int v = 0; v < 6; ++v) a[10 + v] = stage_slabs(stage_array(x, NZ, STAGE_DOWN), nch, NCOL * NZ);
            a[16] = stage_array(x, 1, STAGE_UP);
            for (int v = 0; v < 3; ++v) a[17 + v] = stage_slabs(stage_array(x, 1, STAGE_DOWN), nch, NCOL);
            const size_t profs = 1 + size_t(nch) + 8 + 6 * size_t(nch), cols = 1 + 3 * size_t(nch);
            same(nch > 1 ? "radiometer, 3 channels" : "radiometer", setting, E, stage_plan(a, NCOL, stage_pick_chunk(setting, NCOL), nch > 1 ? GiB1 : 0), CH,
                 profs * b_prof + cols * b_col);
        }
    }
}

// ---- 3. the caps ----
static void capped(const char *entry, StageArray *a, int na, int64_t ncol, size_t cap)
{
    const int64_t pick = stage_pick_chunk(0, ncol);
    CHECK(stage_total(a, na, pick) > cap, "%s: the call does not exceed its cap", entry);
    const StagePlan plan = stage_plan(a, na, ncol, pick, cap);
    CHECK(plan.chunk >= 1 && plan.chunk < pick, "%s: chunk %lld", entry, (long long)plan.chunk);
    CHECK(plan.total <= cap && plan.total == stage_total(a, na, plan.chunk), "%s: %zu bytes planned above the cap", entry, plan.total);
    CHECK(stage_total(a, na, plan.chunk + 1) > cap, "%s: chunk %lld + 1 would fit", entry, (long long)plan.chunk);
}
static void caps()
{
    const int64_t ncol = int64_t(1) << 20, nz = 256;
    {   // spectra: five spectra of 256 bins in binary64, two grids
        StageArray a[37];
        for (int s = 0; s < 5; ++s) {
            a[s] = stage_once(s < 2 ? &F64 : nullptr, 256);
            a[5 + s] = stage_once(s < 2 ? &F64 : nullptr, 256);
            a[32 + s] = stage_array(&F64, 256 * nz, STAGE_DOWN);
        }
        for (int v = 0; v < 11; ++v) { a[10 + v] = stage_array(&F64, nz, STAGE_UP); a[21 + v] = stage_array(&F64, nz, STAGE_DOWN); }
        capped("size spectra", a, 37, ncol, MiB256);
    }
    {   // dspectrum: four spectra of 256 velocity bins in binary64
        StageArray a[20];
        for (int s = 0; s < 3; ++s) { a[s] = stage_once(&F64, 100); a[3 + s] = stage_once(&F64, 100); }
        for (int v = 0; v < 8; ++v) a[6 + v] = stage_array(&F64, nz, STAGE_UP);
        for (int v = 0; v < 6; ++v) a[14 + v] = stage_array(&F64, (v < 4 ? 256 : 1) * nz, STAGE_DOWN);
        capped("doppler spectrum", a, 20, ncol, MiB256);
    }
    {   // the multichannel radiometer: sixteen channels in binary64
        StageArray a[20];
        for (int v = 0; v < 8; ++v) a[v] = stage_array(&F64, nz, STAGE_UP);
        a[8] = stage_rows(&F64, nz, nz);
        a[9] = stage_slabs(stage_rows(&F64, nz, nz), 16, ncol * nz);
        for (int v = 0; v < 6; ++v) a[10 + v] = stage_slabs(stage_array(&F64, nz, STAGE_DOWN), 16, ncol * nz);
        a[16] = stage_array(&F64, 1, STAGE_UP);
        for (int v = 0; v < 3; ++v) a[17 + v] = stage_slabs(stage_array(&F64, 1, STAGE_DOWN), 16, ncol);
        capped("radiometer, 16 channels", a, 20, ncol, GiB1);
        // a cap that nothing fits below: one column per chunk, the least there is
        CHECK(stage_plan(a, 20, ncol, stage_pick_chunk(0, ncol), 1000).chunk == 1, "a cap below one column's slots");
    }
    {   // the multichannel cloud radar: sixteen channels in binary64
        StageArray a[25];
        for (int v = 0; v < 8; ++v) a[v] = stage_array(&F64, nz, STAGE_UP);
        a[8] = stage_rows(&F64, nz, 0);
        a[9] = stage_array(&F64, nz, STAGE_UP);
        a[10] = stage_slabs(stage_rows(&F64, nz, 0), 16, nz);
        for (int v = 0; v < 13; ++v) a[11 + v] = stage_slabs(stage_array(&F64, nz, STAGE_DOWN), 16, ncol * nz);
        a[24] = stage_slabs(stage_array(&F64, 1, STAGE_DOWN), 16, ncol);
        capped("cloud radar, 16 channels", a, 25, ncol, GiB1);
    }
}

int main()
{
    sweep<float>();
    sweep<double>();
    for (int64_t setting : {int64_t(0), int64_t(3)}) {
        parent_equality<float>(setting);
        parent_equality<double>(setting);
    }
    caps();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("stage plan ok\n");
    return 0;
}
