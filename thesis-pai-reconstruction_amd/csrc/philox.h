// Counter-based random numbers inside the kernels: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
// as 1, 2, 3", SC 2011; the Random123 constants).  A random value is a pure function of (seed, step, site, element index):
// nothing random is stored, a backward pass regenerates what its forward used, and a run is reproducible from two integers.
//
// Addressing, the same in every kernel (include/pai_hip.h, "Device random numbers"):
//   key     = (seed low 32 bits, seed high 32 bits)
//   counter = (block, sub, stream, step)
//   block   = flat element index / 4 (uniform, normal, integer, raw) or / 8 (keep bits) of the tensor as it lies in memory
//   sub     = 0, except in the sampler: the draw index k (0 is y_T, k the k-th reverse step)
//   stream  = PHILOX_STREAM_T | _U | _Z | _SAMPLER, PHILOX_STREAM_DROPOUT + i for the i-th ResBlock of Palette, or
//             PHILOX_STREAM_DROPOUT2D + j for the Dropout2d behind decoder j of a GAN-family U-Net (there sub = (rank << 16) | k,
//             k the index of the train-mode forward within the step, and the mask is the flat [N][C] tensor)
//   step    = the training step or the index of the sampling call, passed by value -- or, in the _dev forms the planned sampler
//             records, read from a uint32 in device memory (the mirror of DeviceRNG.step)
// Derived values (fixed: the tests are bit-exact against a host restatement):
//   uniform   (w >> 8) 2^-24 in [0, 1), exact; four per block
//   integer   __umulhi(w, T) in [0, T); four per block
//   keep bit  eight per block: lane j = (w[j / 2] >> 16 (j % 2)) & 0xffff, kept iff lane >= thr, thr = round(p 65536)
//   normal    four per block, Box-Muller on (w0, w1) and on (w2, w3): u1 = ((w >> 9) + 1) 2^-23 in (0, 1], v = (w' >> 8) 2^-24,
//             r = sqrtf(-2 logf(u1)), sincospif(2 v): z0 = r cos, z1 = r sin.  No fast intrinsics; the two products are pinned
//             to one rounding each (__fmul_rn), so that no caller's contraction changes the bits.
// Plain C++ with __umulhi: no inline assembly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t PHILOX_STREAM_T = 0;         // t of the training objective
constexpr uint32_t PHILOX_STREAM_U = 1;         // u, the position of gamma between gammas_prev[t] and gammas[t]
constexpr uint32_t PHILOX_STREAM_Z = 2;         // z of the forward noising
constexpr uint32_t PHILOX_STREAM_SAMPLER = 3;   // the sampler's y_T and per-step noise
constexpr uint32_t PHILOX_STREAM_DROPOUT = 16;  // + i: the dropout of the i-th ResBlock
constexpr uint32_t PHILOX_STREAM_DROPOUT2D = 4096;  // + j: nn.Dropout2d behind decoder j (pai_dropout2d_rng), clear of 16 + i

struct PhiloxKey {
    uint32_t k0, k1;                            // seed low, seed high
    uint32_t sub, stream, step;                 // counter words 1 .. 3
};

__host__ __device__ __forceinline__ PhiloxKey philox_key(uint64_t seed, uint32_t sub, uint32_t stream, uint32_t step) {
    return {(uint32_t)seed, (uint32_t)(seed >> 32), sub, stream, step};
}

struct PhiloxBlock {
    uint32_t w[4];
};

__device__ __forceinline__ PhiloxBlock philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
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
    return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ PhiloxBlock philox_block(const PhiloxKey& k, uint32_t block) {
    return philox4x32_10(k.k0, k.k1, block, k.sub, k.stream, k.step);
}

__device__ __forceinline__ float philox_uniform(uint32_t w) {
    return (float)(w >> 8) * 0x1p-24f;
}

__device__ __forceinline__ int philox_int(uint32_t w, uint32_t T) {
    return (int)__umulhi(w, T);
}

// the 16-bit lane of element j (0 .. 7) of a keep block
__device__ __forceinline__ uint32_t philox_lane16(const PhiloxBlock& b, int j) {
    return (b.w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

// the eight keep flags of a block as eight bytes (1 keeps, 0 drops): the 8-byte vector a uint8 mask holds for the same elements
__device__ __forceinline__ uint2 philox_keep8(const PhiloxBlock& b, uint32_t thr) {
    uint2 v = make_uint2(0u, 0u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v.x |= (philox_lane16(b, j) >= thr ? 1u : 0u) << (8 * j);
        v.y |= (philox_lane16(b, 4 + j) >= thr ? 1u : 0u) << (8 * j);
    }
    return v;
}

// Box-Muller on one pair of words
__device__ __forceinline__ void philox_normal2(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const float u1 = (float)((wa >> 9) + 1u) * 0x1p-23f;          // (0, 1], exact
    const float v2 = (float)(wb >> 8) * 0x1p-23f;                 // 2 v, exact
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(v2, &s, &c);
    z0 = __fmul_rn(r, c);
    z1 = __fmul_rn(r, s);
}

__device__ __forceinline__ void philox_normal4(const PhiloxBlock& b, float* z) {
    philox_normal2(b.w[0], b.w[1], z[0], z[1]);
    philox_normal2(b.w[2], b.w[3], z[2], z[3]);
}

// element i of a tensor of normals (the ragged paths): the whole pair is formed, one half is returned
__device__ __forceinline__ float philox_normal_at(const PhiloxKey& k, int64_t i) {
    const PhiloxBlock b = philox_block(k, (uint32_t)(i >> 2));
    const int l = (int)(i & 3);
    float z0, z1;
    philox_normal2((l & 2) ? b.w[2] : b.w[0], (l & 2) ? b.w[3] : b.w[1], z0, z1);
    return (l & 1) ? z1 : z0;
}
