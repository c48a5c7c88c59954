// pai_philox_fill: the generator of philox.h written out as a tensor -- the surface its bits are pinned through, and a utility
// (the sampler's y_T).  A thread owns one block: four elements (raw, uniform, normal, integer) or eight (keep), stored as one
// vector where the whole block lies below n and `out` is aligned for it, element by element otherwise.
#include "common.h"
#include "philox.h"

template <int KIND>
__device__ __forceinline__ void philox_fill_body(void* out, int64_t n, const PhiloxKey& key, uint32_t param, int vec) {
    constexpr int E = KIND == PAI_PHILOX_KEEP ? 8 : 4;
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = b * E;
    if (i0 >= n) return;
    const PhiloxBlock blk = philox_block(key, (uint32_t)b);
    const bool whole = vec && i0 + E <= n;
    if (KIND == PAI_PHILOX_KEEP) {
        const uint2 v = philox_keep8(blk, param);
        unsigned char* o = (unsigned char*)out;
        if (whole) {
            *(uint2*)(o + i0) = v;
        } else {
            for (int e = 0; e < 8 && i0 + e < n; ++e) o[i0 + e] = (unsigned char)(((e < 4 ? v.x : v.y) >> (8 * (e & 3))) & 0xffu);
        }
        return;
    }
    uint32_t w[4];                                 // the four elements as their bit patterns
    if (KIND == PAI_PHILOX_NORMAL) {
        float z[4];
        philox_normal4(blk, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = __float_as_uint(z[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            w[e] = KIND == PAI_PHILOX_UNIFORM ? __float_as_uint(philox_uniform(blk.w[e]))
                   : KIND == PAI_PHILOX_INT   ? (uint32_t)philox_int(blk.w[e], param)
                                              : blk.w[e];
    }
    uint32_t* o = (uint32_t*)out;
    if (whole) {
        *(uint4*)(o + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < n) o[i0 + e] = w[e];
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void philox_fill_k(void* out, int64_t n, PhiloxKey key, uint32_t param, int vec) {
    philox_fill_body<KIND>(out, n, key, param, vec);
}

// the same body with counter word 3 read from device memory: a recorded launch follows a step counter that advances on the device
template <int KIND>
__global__ __launch_bounds__(256) void philox_fill_dev_k(void* out, int64_t n, PhiloxKey key, const uint32_t* step_dev, uint32_t param,
                                                         int vec) {
    key.step = *step_dev;
    philox_fill_body<KIND>(out, n, key, param, vec);
}

// ---- device-held counters: the sampler's step index and the mirror of DeviceRNG.step ---------------------------------------------
// One thread, plain loads and stores; unsigned arithmetic wraps at 2^32 as DeviceRNG.advance does on the host.
__global__ void counter_set_k(uint32_t* c, uint32_t v) { *c = v; }
__global__ void counter_add_k(uint32_t* c, uint32_t d) { *c = *c + d; }

extern "C" int pai_counter_set(uint32_t* c, uint32_t v, void* stream) {
    PAI_CHECK(c, "pai_counter_set: null counter");
    PAI_CHECK((uintptr_t)c % 4 == 0, "pai_counter_set: the counter is not aligned to 4 bytes");
    PAI_LAUNCH(counter_set_k, dim3(1), dim3(1), 0, (hipStream_t)stream, c, v);
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_counter_add(uint32_t* c, uint32_t d, void* stream) {
    PAI_CHECK(c, "pai_counter_add: null counter");
    PAI_CHECK((uintptr_t)c % 4 == 0, "pai_counter_add: the counter is not aligned to 4 bytes");
    PAI_LAUNCH(counter_add_k, dim3(1), dim3(1), 0, (hipStream_t)stream, c, d);
    PAI_LAUNCH_CHECK();
    return 0;
}

// the refusals and the launch geometry shared by pai_philox_fill and pai_philox_fill_dev
static int philox_fill_launch(const char* who, int kind, void* out, int64_t n, uint64_t seed, uint32_t sub, uint32_t stream,
                              uint32_t step, const uint32_t* step_dev, bool dev, uint32_t param, void* stream_handle) {
    PAI_CHECK(kind >= PAI_PHILOX_RAW && kind <= PAI_PHILOX_KEEP, "%s: kind=%d", who, kind);
    PAI_CHECK(out, "%s: null tensor", who);
    PAI_CHECK(!dev || step_dev, "%s: null step counter", who);
    PAI_CHECK(n >= 1, "%s: n=%lld", who, (long long)n);
    PAI_CHECK(kind != PAI_PHILOX_INT || (param >= 1 && param <= 0x7fffffffu), "%s: T=%u (1 .. 2^31 - 1)", who, param);
    PAI_CHECK(kind != PAI_PHILOX_KEEP || param <= 65536u, "%s: thr=%u (round(p 65536), at most 65536)", who, param);
    const int E = kind == PAI_PHILOX_KEEP ? 8 : 4, esz = kind == PAI_PHILOX_KEEP ? 1 : 4;
    PAI_CHECK((uintptr_t)out % esz == 0, "%s: out is not aligned to its element type", who);
    const int64_t blocks = (n - 1) / E + 1;
    PAI_CHECK(blocks <= (1ll << 32), "%s: tensor too large (more than 2^32 blocks of %d)", who, E);
    const int vec = (uintptr_t)out % (E * esz) == 0;
    const dim3 grid((unsigned)((blocks + 255) / 256));
    const PhiloxKey key = philox_key(seed, sub, stream, step);
    hipStream_t s = (hipStream_t)stream_handle;
#define PAI_PHILOX_FILL(K)                                                                              \
    do {                                                                                                \
        if (dev) PAI_LAUNCH(philox_fill_dev_k<K>, grid, dim3(256), 0, s, out, n, key, step_dev, param, vec); \
        else PAI_LAUNCH(philox_fill_k<K>, grid, dim3(256), 0, s, out, n, key, param, vec);              \
    } while (0)
    switch (kind) {
        case PAI_PHILOX_RAW: PAI_PHILOX_FILL(PAI_PHILOX_RAW); break;
        case PAI_PHILOX_UNIFORM: PAI_PHILOX_FILL(PAI_PHILOX_UNIFORM); break;
        case PAI_PHILOX_NORMAL: PAI_PHILOX_FILL(PAI_PHILOX_NORMAL); break;
        case PAI_PHILOX_INT: PAI_PHILOX_FILL(PAI_PHILOX_INT); break;
        default: PAI_PHILOX_FILL(PAI_PHILOX_KEEP); break;
    }
#undef PAI_PHILOX_FILL
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_philox_fill(int kind, void* out, int64_t n, uint64_t seed, uint32_t sub, uint32_t stream, uint32_t step,
                               uint32_t param, void* stream_handle) {
    return philox_fill_launch("pai_philox_fill", kind, out, n, seed, sub, stream, step, nullptr, false, param, stream_handle);
}

extern "C" int pai_philox_fill_dev(int kind, void* out, int64_t n, uint64_t seed, uint32_t sub, uint32_t stream,
                                   const uint32_t* step_dev, uint32_t param, void* stream_handle) {
    return philox_fill_launch("pai_philox_fill_dev", kind, out, n, seed, sub, stream, 0, step_dev, true, param, stream_handle);
}

// ---- nn.Dropout2d with the keep flags of the device generator (GAN families) ----------------------------------------------------
// out[n][p][c] = x[n][p][c] * (keep(n, c) ? keep_scale : 0) on an NHWC tensor.  The mask is the flat [N][C] tensor: the eight
// channels of a vector are one keep block, block index n * C / 8 + c0 / 8 -- a "column", the same for every pixel of the image.
// A thread owns one column: it runs the ten rounds once and then walks its pixels, so a 32-byte vector costs a load, eight
// multiplies and a store.  A workgroup is TC columns x 256 / TC pixels (TC a power of two, chosen on the host so that the lanes
// of a wave read neighbouring vectors); grid.x strides over the columns, grid.y over the pixels.  The body after the flags is
// that of dropout2d_k (csrc/misc.hip): for the same flags the bits of pai_dropout2d given the mask {0, keep_scale}.
template <typename T>
__device__ __forceinline__ void dropout2d_rng_body(const T* x, int64_t ncol, int CV, int64_t HW, const PhiloxKey& key, uint32_t thr,
                                                   float keep_scale, int tc_shift, T* out) {
    const int TC = 1 << tc_shift, TP = 256 >> tc_shift;
    const int ic = threadIdx.x & (TC - 1), ip = threadIdx.x >> tc_shift;
    const int64_t C = (int64_t)CV * 8;
    for (int64_t col = (int64_t)blockIdx.x * TC + ic; col < ncol; col += (int64_t)gridDim.x * TC) {
        const int64_t n = col / CV;
        const int64_t base = n * HW * C + (col - n * CV) * 8;
        const PhiloxBlock blk = philox_block(key, (uint32_t)col);
        float m[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = philox_lane16(blk, k) >= thr ? keep_scale : 0.f;
        for (int64_t p = (int64_t)blockIdx.y * TP + ip; p < HW; p += (int64_t)gridDim.y * TP) {
            float v[8];
            V8<T>::ld(x + base + p * C, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= m[k];
            V8<T>::st(out + base + p * C, v);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dropout2d_rng_k(const T* x, int64_t ncol, int CV, int64_t HW, PhiloxKey key, uint32_t thr,
                                                       float keep_scale, int tc_shift, T* out) {
    dropout2d_rng_body<T>(x, ncol, CV, HW, key, thr, keep_scale, tc_shift, out);
}

// the same body with counter word 3 read from device memory
template <typename T>
__global__ __launch_bounds__(256) void dropout2d_rng_dev_k(const T* x, int64_t ncol, int CV, int64_t HW, PhiloxKey key,
                                                           const uint32_t* step_dev, uint32_t thr, float keep_scale, int tc_shift,
                                                           T* out) {
    key.step = *step_dev;
    dropout2d_rng_body<T>(x, ncol, CV, HW, key, thr, keep_scale, tc_shift, out);
}

constexpr int DROPOUT2D_RNG_GRID_X = 4096;      // columns past 4096 workgroups' worth are further trips of the column loop

// the refusals and the launch geometry shared by pai_dropout2d_rng and pai_dropout2d_rng_dev
static int dropout2d_rng_launch(const char* who, int dtype, const void* x, int N, int64_t HW, int C, uint64_t seed, uint32_t sub,
                                uint32_t stream, uint32_t step, const uint32_t* step_dev, bool dev, uint32_t thr, float keep_scale,
                                void* out, void* stream_handle) {
    PAI_CHECK(x && out, "%s: null pointer", who);
    PAI_CHECK(!dev || step_dev, "%s: null step counter", who);
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "%s: dtype=%d", who, dtype);
    PAI_CHECK(C >= 8 && C % 8 == 0 && N >= 1 && HW >= 1, "%s: bad shape N=%d HW=%lld C=%d", who, N, (long long)HW, C);
    PAI_CHECK(thr <= 65536u, "%s: thr=%u (round(p 65536), at most 65536)", who, thr);
    const int CV = C / 8;
    const int64_t ncol = (int64_t)N * CV;
    PAI_CHECK(ncol <= (1ll << 32), "%s: mask too large (more than 2^32 blocks of 8)", who);
    PAI_CHECK(HW <= INT64_MAX / 8 / ncol, "%s: tensor too large N=%d HW=%lld C=%d", who, N, (long long)HW, C);
    // TC: the columns of one pixel side by side, up to 256; the rest of the workgroup goes over pixels -- unless the image has
    // fewer pixels than that, where the spare lanes take further columns (HW = 1, the token form, is 256 columns a workgroup)
    int tc_shift = 0;
    while ((1 << tc_shift) < CV && tc_shift < 8) ++tc_shift;
    while (tc_shift < 8 && (256 >> tc_shift) / 2 >= HW) ++tc_shift;
    const int TC = 1 << tc_shift, TP = 256 >> tc_shift;
    int64_t gx = (ncol + TC - 1) / TC;
    if (gx > DROPOUT2D_RNG_GRID_X) gx = DROPOUT2D_RNG_GRID_X;
    // pixels per thread: as many as leave about two workgroups for each of the 256 compute units
    int64_t gy = (HW + TP - 1) / TP;
    const int64_t want = (512 + gx - 1) / gx;
    if (gy > want) gy = want;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    const PhiloxKey key = philox_key(seed, sub, stream, step);
    hipStream_t s = (hipStream_t)stream_handle;
    if (dtype == PAI_F32) {
        if (dev) PAI_LAUNCH(dropout2d_rng_dev_k<float>, grid, dim3(256), 0, s, (const float*)x, ncol, CV, HW, key, step_dev, thr,
                            keep_scale, tc_shift, (float*)out);
        else PAI_LAUNCH(dropout2d_rng_k<float>, grid, dim3(256), 0, s, (const float*)x, ncol, CV, HW, key, thr, keep_scale, tc_shift,
                        (float*)out);
    } else {
        if (dev) PAI_LAUNCH(dropout2d_rng_dev_k<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, ncol, CV, HW, key, step_dev, thr,
                            keep_scale, tc_shift, (bf16_t*)out);
        else PAI_LAUNCH(dropout2d_rng_k<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, ncol, CV, HW, key, thr, keep_scale,
                        tc_shift, (bf16_t*)out);
    }
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_dropout2d_rng(int dtype, const void* x, int N, int64_t HW, int C, uint64_t seed, uint32_t sub, uint32_t stream,
                                 uint32_t step, uint32_t thr, float keep_scale, void* out, void* stream_handle) {
    return dropout2d_rng_launch("pai_dropout2d_rng", dtype, x, N, HW, C, seed, sub, stream, step, nullptr, false, thr, keep_scale, out,
                                stream_handle);
}

extern "C" int pai_dropout2d_rng_dev(int dtype, const void* x, int N, int64_t HW, int C, uint64_t seed, uint32_t sub,
                                     uint32_t stream, const uint32_t* step_dev, uint32_t thr, float keep_scale, void* out,
                                     void* stream_handle) {
    return dropout2d_rng_launch("pai_dropout2d_rng_dev", dtype, x, N, HW, C, seed, sub, stream, 0, step_dev, true, thr, keep_scale,
                                out, stream_handle);
}
