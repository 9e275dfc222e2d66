// kidmp_wave.h -- internal to kidmp_kinematic.hip and kidmp_slab.hip (not installed): a column held by one wavefront, level
// k = 64 j + lane, and the moves between neighbouring levels that both advection kernels are built from.
#pragma once
#include <hip/hip_runtime.h>

namespace kidmp {
namespace wave {
// ---- a shift by one level across the whole wave ----
// One DPP move per half: wave_shr:1 hands lane l the value of lane l - 1, wave_shl:1 that of lane l + 1; the one lane
// without a source (0, or 63) keeps `edge`, which is where the neighbouring level group hands its end over.
constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138;
template <int CTRL>
__device__ inline double wave_shift(double edge, double v)
{
    const long long e = __double_as_longlong(edge), b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(int(e & 0xffffffffll), int(b & 0xffffffffll), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(int(e >> 32), int(b >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}
__device__ inline double readlane(double v, int lane)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(int(b & 0xffffffffll), lane);
    const int hi = __builtin_amdgcn_readlane(int(b >> 32), lane);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}
// out[j] of level k = v of level k - 1; level 0 receives an unspecified finite value (the caller masks it)
template <int NJ>
__device__ inline void level_below(const double (&v)[NJ], double (&out)[NJ])
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) out[j] = wave_shift<DPP_WAVE_SHR1>(j ? readlane(v[j - 1], 63) : 0., v[j]);
}
// out[j] of level k = v of level k + 1; the last lane of the last group receives an unspecified finite value
template <int NJ>
__device__ inline void level_above(const double (&v)[NJ], double (&out)[NJ])
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) out[j] = wave_shift<DPP_WAVE_SHL1>(j + 1 < NJ ? readlane(v[j + 1], 0) : 0., v[j]);
}
__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}
}  // namespace wave
}  // namespace kidmp
