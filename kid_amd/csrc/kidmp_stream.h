// kidmp_stream.h -- what the streaming kernels of kidmp_adapter.hip and kidmp_kinematic.hip share: 16-byte vectors of T with
// null arrays as zero operands, and the grid of a grid-stride loop.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kidmp {
namespace streaming {
// 16 bytes of T (V = 2 doubles / 4 floats), or one element (V = 1) where nz or an address does not allow the wide form
template <class T, int V> struct alignas(sizeof(T) * V) Vec { T v[V]; };

// a null array is a literal zero operand: never read, and (0 + x), (x + 0) round as with an array of +0.0
template <class T, int V> __device__ inline Vec<T, V> ld(const T *p, int64_t e)
{
    Vec<T, V> r;
    if (p) r = *reinterpret_cast<const Vec<T, V> *>(p + e);
    else
#pragma unroll
        for (int j = 0; j < V; ++j) r.v[j] = T(0);
    return r;
}
template <class T, int V> __device__ inline void st(T *p, int64_t e, const Vec<T, V> &x) { *reinterpret_cast<Vec<T, V> *>(p + e) = x; }

// a grid sized to the chip (256 CUs, eight blocks of 256 lanes each), walked with a grid-stride loop
inline unsigned grid_for(int64_t nvec)
{
    const int64_t g = (nvec + 255) / 256;
    return unsigned(g < 1 ? 1 : g > 2048 ? 2048 : g);
}
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace streaming
}  // namespace kidmp
