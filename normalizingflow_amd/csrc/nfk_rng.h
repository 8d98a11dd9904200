// nfk_rng.h -- the counter-based random numbers of the device: Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
// Random123 constants) and the normal draw made from it.  ONE definition, shared
// by the fill kernel and the Langevin kernels of nfk_langevin.hip, so a normal
// inside a trajectory has the bits of the fill kernel's.  Plain C++ and
// __umulhi, accurate logf / sqrtf / sincospif.  Include after
// <hip/hip_runtime.h> and nfk_systems_dev.h (group_sum).
//
// Addressing (never a function of the launch geometry):
//   counter = (step_lo, step_hi, particle, row)    step: absolute 64-bit step index
//   key     = (seed_lo, seed_hi | tag << 31)       seed < 2^63; row = row_base + b as uint32
// tag 0 is thermostat noise, tag 1 initial velocities.  One call gives four
// words, hence four normals: component d of a particle is normal d (dim <= 4).
#ifndef NFK_RNG_H_
#define NFK_RNG_H_

#include <cstdint>

namespace {

struct RngKey {
    uint32_t k0, k1;   // seed_lo, seed_hi | tag << 31
    uint32_t row_base;
    int zero_mean;
};

struct Words4 {
    uint32_t w[4];
};

__device__ __forceinline__ Words4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    Words4 o;
    o.w[0] = c0;
    o.w[1] = c1;
    o.w[2] = c2;
    o.w[3] = c3;
    return o;
}

__device__ __forceinline__ Words4 rng_words(const RngKey& key, uint64_t step, uint32_t particle, uint32_t row) {
    return philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), particle, row, key.k0, key.k1);
}

// u in (0, 1): the word's upper 24 bits, centred in their cell
__device__ __forceinline__ float rng_unit(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-08f; }

// four normals of one call: two Box-Muller pairs, (w0, w1) -> z0, z1 and (w2, w3) -> z2, z3;
// |z| <= sqrt(-2 log(2^-25)) = 5.89
__device__ __forceinline__ void rng_normal4(const RngKey& key, uint64_t step, uint32_t particle, uint32_t row,
                                            float (&z)[4]) {
    const Words4 o = rng_words(key, step, particle, row);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float r = sqrtf(-2.0f * logf(rng_unit(o.w[2 * h])));
        float s, c;
        sincospif(2.0f * rng_unit(o.w[2 * h + 1]), &s, &c);
        z[2 * h] = r * c;
        z[2 * h + 1] = r * s;
    }
}

// The per-dimension mean of a row's normals (the thermostat's `zero yes`) in the
// mapping of the row kernels: lane c0 of an aligned group of G lanes sums its own
// particles c0 + q G < n in ascending order, the butterfly combines the lanes, the
// sum is divided by n.  Every lane of the group gets the mean.  Call with all 64
// lanes of the wave active.
template <int G>
__device__ __forceinline__ void rng_row_mean(const RngKey& key, uint64_t step, uint32_t row, int n, int c0,
                                             float (&mean)[4]) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, z[4];
    for (int p = c0; p < n; p += G) {
        rng_normal4(key, step, (uint32_t)p, row, z);
#pragma unroll
        for (int d = 0; d < 4; ++d) s[d] += z[d];
    }
    const float fn = (float)n;
#pragma unroll
    for (int d = 0; d < 4; ++d) mean[d] = group_sum<G>(s[d]) / fn;
}

// group_sum over aligned groups of g lanes, g a power of two <= 64 known at run time
__device__ __forceinline__ float group_sum_rt(float v, int g) {
    for (int off = g >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// rng_row_mean for a kernel whose groups of W lanes are wider than the g = lanes_for(n)
// lanes of the particle mapping (a lane per coordinate): the first g lanes of the group
// (c0 < g) do rng_row_mean's sums and its butterfly, the group's first lane hands the
// result to the others.  The same operations in the same order: the same bits.
template <int W>
__device__ __forceinline__ void rng_row_mean_in(const RngKey& key, uint64_t step, uint32_t row, int n, int g,
                                                int c0, float (&mean)[4]) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, z[4];
    if (c0 < g)
        for (int p = c0; p < n; p += g) {
            rng_normal4(key, step, (uint32_t)p, row, z);
#pragma unroll
            for (int d = 0; d < 4; ++d) s[d] += z[d];
        }
    const float fn = (float)n;
    const int first = (threadIdx.x & 63) - c0;
#pragma unroll
    for (int d = 0; d < 4; ++d) mean[d] = __shfl(group_sum_rt(s[d], g) / fn, first, 64);
}

// the key of a call: NFK_EINVAL-worthy seeds are refused by the entry points
inline RngKey rng_key(int64_t seed, int tag, int64_t row_base, int zero_mean) {
    RngKey k;
    k.k0 = (uint32_t)((uint64_t)seed & 0xffffffffu);
    k.k1 = (uint32_t)((uint64_t)seed >> 32) | ((uint32_t)tag << 31);
    k.row_base = (uint32_t)row_base;
    k.zero_mean = zero_mean ? 1 : 0;
    return k;
}

}  // namespace

#endif  // NFK_RNG_H_
