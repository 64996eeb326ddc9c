// counter_rng.hpp -- the counter-based generator of conan_slam_amd/synth.py on the device: splitmix64(seed, idx) ->
// 53-bit uniforms -> Box-Muller, in f64 and in synth.py's operation order.  Shared by the batched scan generator
// (cslam_sim_batch.hip) and the particle filter's draws (pf_draw_kernels.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "device_math.hpp" // kPi

namespace cslam
{

// (also on the host: the seed of the particle filter's control stream, pf_control_seed, is derived there once per call)
__host__ __device__ inline unsigned long long splitmix64(unsigned long long seed, unsigned long long idx)
{
    unsigned long long z = seed * 0x9E3779B97F4A7C15ull + idx + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline double uniform01(unsigned long long seed, unsigned long long idx)
{
    return (double)(splitmix64(seed, idx) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ inline double counter_normal(unsigned long long seed, unsigned long long idx)
{
    const double u1 = uniform01(seed, 2ull * idx), u2 = uniform01(seed, 2ull * idx + 1ull);
    return sqrt(-2.0 * log(1.0 - u1)) * cos((2.0 * kPi) * u2);
}

} // namespace cslam
