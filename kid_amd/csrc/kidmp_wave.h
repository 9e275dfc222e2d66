// kidmp_wave.h -- internal to kidmp_kinematic.hip, kidmp_slab.hip, kidmp_scan.hip and the wave-per-column diagnostics
// (kidmp_column.h; not installed): a column (or a ray) held by one wavefront, level (gate) k = 64 j + lane, the moves between
// neighbouring levels that both advection kernels are built from, and the sum scan that the path integrals of the column
// diagnostics and of the scan share.
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
// inclusive sum scan over the wave, Kogge-Stone over __shfl_up: lane l receives v[0] + ... + v[l], in an order that l alone
// fixes.  DOWN is its mirror image over __shfl_down: lane l receives v[l] + ... + v[63].  `total` receives the sum of the
// whole wave as the last (DOWN: the first) lane holds it, wave-uniform.  Whole wavefronts only.
template <bool DOWN>
__device__ inline double wave_prefix_sum(double v, int lane, double &total)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = DOWN ? __shfl_down(v, d, 64) : __shfl_up(v, d, 64);
        if (DOWN ? lane + d < 64 : lane >= d) v += o;
    }
    total = readlane(v, DOWN ? 0 : 63);
    return v;
}
__device__ inline double wave_max(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}
}  // namespace wave
}  // namespace kidmp
