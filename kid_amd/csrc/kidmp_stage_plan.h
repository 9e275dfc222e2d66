// kidmp_stage_plan.h -- how a host-array entry of the diagnostics cuts its batch into column chunks and the context's
// staging memory into slots: the call as a short list of array descriptors, and from it, in plain host arithmetic, the
// chunk size, every slot's offset, the bytes of staging needed and every copy's two ranges.  Nothing of HIP in it, so that
// the arithmetic the executor (stage_run of kidmp_host.hip) follows is the arithmetic a host program can enumerate
// (tests/native/stage_plan_check.cpp).
//
// A slot holds one chunk of one array, rows packed, and starts on a multiple of 256 bytes; an array of nslab slabs (the
// channels of the multichannel entries) has nslab such pieces one after the other, each 256-byte aligned.  An array whose
// host pointer is null takes no slot and moves no bytes, unless it keeps its slot (the entries that always laid out every
// array).  Slots follow one another in the order of the list.
#pragma once

#include <cstddef>
#include <cstdint>

namespace kidmp {
enum : int { STAGE_UP = 1, STAGE_DOWN = 2, STAGE_BOTH = STAGE_UP | STAGE_DOWN };

struct StageArray {
    const void *host;          // the caller's array; null: absent
    size_t elem;               // bytes per element
    int64_t per_col;           // elements per column; of a `once` array: elements in all
    int dir;                   // STAGE_UP, STAGE_DOWN or STAGE_BOTH
    int64_t col_stride;        // host elements from one column to the next: per_col = packed, more = padded rows (packed on
                               // upload), 0 = one row shared by all columns, uploaded once ahead of the first chunk
    int32_t nslab;             // slabs of ncol columns each ...
    int64_t slab_stride;       // ... this many host elements apart
    bool once;                 // does not scale with the chunk: uploaded whole ahead of the first chunk (the caller's grids)
    bool keep_slot;            // holds its slot even when absent
    // what stage_plan fills in (dev: stage_open)
    size_t offset, slab_bytes; // the slot's first byte in the staging memory; bytes from one staged slab to the next
    void *dev;                 // the slot in device memory; null when absent
};

template <class T> StageArray stage_array(const T *host, int64_t per_col, int dir)
{ return StageArray{host, sizeof(T), per_col, dir, per_col, 1, 0, false, false, 0, 0, nullptr}; }
// an input profile of nz values with the column stride of the C ABI: 0 = one profile for all columns, else >= nz
template <class T> StageArray stage_rows(const T *host, int64_t nz, int64_t col_stride)
{
    StageArray a = stage_array(host, nz, STAGE_UP);
    a.col_stride = col_stride;
    return a;
}
template <class T> StageArray stage_once(const T *host, int64_t count)
{
    StageArray a = stage_array(host, count, STAGE_UP);
    a.once = true;
    return a;
}
inline StageArray stage_slabs(StageArray a, int32_t nslab, int64_t slab_stride) { a.nslab = nslab; a.slab_stride = slab_stride; return a; }
inline StageArray stage_keep(StageArray a) { a.keep_slot = true; return a; }
template <class T> T *staged(const StageArray &a) { return static_cast<T *>(a.dev); }

// the columns per chunk of a host-array entry: the context's setting (kidmp_set_host_chunk), else chosen from ncol
inline int64_t stage_pick_chunk(int64_t host_chunk, int64_t ncol)
{
    if (host_chunk > 0) return host_chunk < ncol ? host_chunk : ncol;
    if (ncol <= 2048) return ncol;                            // one chunk: nothing to overlap with
    int64_t ch = (ncol + 3) / 4;                              // at least four chunks ...
    ch = (ch + 255) / 256 * 256;
    return ch > 8192 ? 8192 : ch;                             // ... of at most 8 192 columns (7.9 MB per profile slice; measured optimum)
}

inline bool stage_has_slot(const StageArray &a) { return a.host || a.keep_slot; }
inline bool stage_before_loop(const StageArray &a) { return a.once || a.col_stride == 0; }
inline size_t stage_slab_bytes(int64_t chunk, int64_t per_col, size_t elem) { return (size_t(chunk) * size_t(per_col) * elem + 255) / 256 * 256; }
inline size_t stage_total(const StageArray *a, int na, int64_t chunk)
{
    size_t total = 0;
    for (int i = 0; i < na; ++i)
        if (stage_has_slot(a[i])) total += size_t(a[i].nslab) * stage_slab_bytes(a[i].once ? 1 : chunk, a[i].per_col, a[i].elem);
    return total;
}

struct StagePlan {
    StageArray *a;
    int na;
    int64_t ncol, chunk;       // chunk >= 1
    size_t total;              // bytes of staging memory
};

// chunk: 1 .. ncol, what the entry would take; cap (0: none): bytes of staging above which the chunk is narrowed to the
// largest one, at least 1, whose slots fit
inline StagePlan stage_plan(StageArray *a, int na, int64_t ncol, int64_t chunk, size_t cap = 0)
{
    if (cap && stage_total(a, na, chunk) > cap) {
        int64_t fits = 1, over = chunk;                       // the total grows with the chunk
        while (over - fits > 1) {
            const int64_t mid = fits + (over - fits) / 2;
            (stage_total(a, na, mid) <= cap ? fits : over) = mid;
        }
        chunk = fits;
    }
    size_t off = 0;
    for (int i = 0; i < na; ++i) {
        a[i].offset = off;
        a[i].slab_bytes = stage_slab_bytes(a[i].once ? 1 : chunk, a[i].per_col, a[i].elem);
        a[i].dev = nullptr;
        if (stage_has_slot(a[i])) off += size_t(a[i].nslab) * a[i].slab_bytes;
    }
    return StagePlan{a, na, ncol, chunk, off};
}
template <size_t N> StagePlan stage_plan(StageArray (&a)[N], int64_t ncol, int64_t chunk, size_t cap = 0)
{ return stage_plan(a, int(N), ncol, chunk, cap); }
// the chunks are [c0, c0 + stage_chunk_cols) for c0 = 0, chunk, 2 chunk, .. below ncol: the last one may be short
inline int64_t stage_chunk_cols(const StagePlan &p, int64_t c0) { return c0 + p.chunk <= p.ncol ? p.chunk : p.ncol - c0; }

// One copy of one slab, in bytes: `rows` rows of row_bytes, host_pitch apart on the host and packed in the slot
struct StageCopy { size_t host_off, stage_off, row_bytes, rows, host_pitch; };
// the columns [c0, c0 + n) of slab `slab` (an array that goes up ahead of the loop has no columns to choose)
inline StageCopy stage_copy(const StageArray &a, int slab, int64_t c0, int64_t n)
{
    const size_t row = size_t(a.per_col) * a.elem, base = size_t(slab) * size_t(a.slab_stride) * a.elem;
    const size_t dst = a.offset + size_t(slab) * a.slab_bytes;
    if (stage_before_loop(a)) return StageCopy{base, dst, row, 1, row};
    if (a.col_stride == a.per_col) return StageCopy{base + size_t(c0) * row, dst, size_t(n) * row, 1, size_t(n) * row};
    const size_t pitch = size_t(a.col_stride) * a.elem;
    return StageCopy{base + size_t(c0) * pitch, dst, row, size_t(n), pitch};
}
}  // namespace kidmp
