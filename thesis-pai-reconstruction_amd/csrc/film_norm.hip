// Train-mode norm sites of the guided-diffusion U-Net (reference models/guided_diffusion/unet.py:141-172,206-210 and
// nn.py:16-23,51-68): BatchNorm with batch statistics, the per-sample FiLM scale / shift, SiLU and element-wise Dropout as
// one differentiable op on [N][rows][C].
//
//   xhat = (x - mean_c) rstd_c,  v = gamma_c xhat + beta_c,  u = v (1 + s_nc) + t_nc,  y = m k act(u)
//
//   pai_film_norm_fwd    one pass.  The statistics come from pai_bn_stats + pai_bn_finalize.
//   pai_film_norm_bwd    three launches, du = g m k act'(u) rebuilt in the first and the third and never stored:
//                          reduce    grid (slabs, N): S0 = sum_p du and S1 = sum_p du xhat of the rows of one (slab, sample)
//                          finalize  the slabs summed in fp64 in a fixed order; demb, dgamma +=, dbeta +=, dbeta / M, dgamma / M
//                          apply     dx = gamma rstd (du (1 + s) - dbeta / M - xhat dgamma / M)
//                        No atomics, no sum across workgroups in arrival order: the same bits on every run.
//   pai_film_norm_fwd_rng, pai_film_norm_bwd_rng    the same kernel bodies with the keep flags m formed from a Philox block per
//                        vector (philox.h) instead of read from a mask: no mask tensor exists, the backward rebuilds the flags.
//
// All three tensor kernels share one geometry: C = 8 G, a thread keeps the channel group tid % G and the row lane tid / G
// of the R = 256 / G rows a workgroup covers at a time (threads past R * G idle), builds its coefficients once and has FV
// 16-byte vectors per tensor in flight (the mask: one 8-byte vector per tensor vector).  Workgroup (slab, n) owns the rows
// [slab * rps, (slab + 1) * rps) of sample n, rps = ceil(rows / slabs); a slab past the last row owns nothing, and in the
// reduce it still writes its (zero) partial sums, so the finalize never reads what no launch wrote.
#include "common.h"
#include "philox.h"

#include <math.h>

constexpr int FV = 4;                  // vectors in flight per thread and tensor
constexpr int FN_SLAB_ROWS = 64;       // rows of a slab until FN_MAX_SLABS is reached
constexpr int FN_MAX_SLABS = 256;

// fn_sig (common.h): sigmoid(u) and 1 - sigmoid(u) from e = exp(-|u|).
template <int ACT, bool EXACT> __device__ __forceinline__ float fn_act(float u) {
    if (ACT != PAI_ACT_SILU) return u;
    float sig, oms;
    fn_sig<EXACT>(u, sig, oms);
    return u * sig;
}
template <int ACT, bool EXACT> __device__ __forceinline__ float fn_dact(float u) {
    if (ACT != PAI_ACT_SILU) return 1.f;
    float sig, oms;
    fn_sig<EXACT>(u, sig, oms);
    return sig * fmaf(u, oms, 1.f);
}

// per-thread coefficients of one (sample, channel group): u = xhat * a + b with a = gamma (1 + s), b = beta (1 + s) + t
template <typename T>
__device__ __forceinline__ void fn_coeffs(const float* gamma, const float* beta, const T* emb, int64_t ld, int n, int C, int c0,
                                          float* a, float* b, float* sc) {
    V8<float>::ld(gamma + c0, a);
    V8<float>::ld(beta + c0, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = 1.f;
        if (emb) {
            const T* row = emb + (int64_t)n * ld + c0 + e;
            sc[e] = 1.0f + Conv<T>::ld(row);
            a[e] *= sc[e];
            b[e] = fmaf(b[e], sc[e], Conv<T>::ld(row + C));
        }
    }
}

// the eight mask bytes of one vector (all kept without dropout), and m k of element e: ks = k, or 1 without dropout
__device__ __forceinline__ uint2 fn_mask_ld(const unsigned char* mask, int64_t off) {
    return mask ? *(const uint2*)(mask + off) : make_uint2(0x01010101u, 0x01010101u);
}
__device__ __forceinline__ float fn_mk(uint2 v, int e, float ks) {
    return (((e < 4 ? v.x : v.y) >> (8 * (e & 3))) & 0xffu) ? ks : 0.f;
}

// Where the eight keep flags of a vector come from: a uint8 mask in memory (pai_film_norm_fwd / _bwd), or one Philox block of
// (seed, stream, step) per vector (the _rng forms; philox.h) -- integer work that has no operand from memory, so it runs while
// the vector loads issued in front of it are in flight.  `off` is the flat element offset of the vector, a multiple of 8.
struct FnMaskSrc {
    const unsigned char* mask;
    bool aligned() const { return ((uintptr_t)mask) % 8 == 0; }
    __device__ __forceinline__ bool on() const { return mask != nullptr; }
    __device__ __forceinline__ uint2 operator()(int64_t off) const { return fn_mask_ld(mask, off); }
};
struct FnRngSrc {
    PhiloxKey key;
    uint32_t thr;
    bool aligned() const { return true; }
    __device__ __forceinline__ bool on() const { return true; }
    __device__ __forceinline__ uint2 operator()(int64_t off) const {
        return philox_keep8(philox_block(key, (uint32_t)(off >> 3)), thr);
    }
};

struct FnRows {
    int64_t r0, r1;                    // rows of this workgroup
};
__device__ __forceinline__ FnRows fn_rows(int64_t rows) {
    const int64_t rps = (rows + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = min(rows, (int64_t)blockIdx.x * rps);
    return {r0, min(rows, r0 + rps)};
}

template <typename T, int ACT, typename KS>
__global__ __launch_bounds__(256) void film_norm_fwd_k(const T* x, int64_t rows, int G, int R, const float* mean, const float* rstd,
                                                       const float* gamma, const float* beta, const T* emb, int64_t ld,
                                                       KS keep, float keep_scale, T* out) {
    const int cg = threadIdx.x % G, rr = threadIdx.x / G;
    if (rr >= R) return;
    const int C = G * 8, n = blockIdx.y;
    const float ks = keep.on() ? keep_scale : 1.f;
    float mu[8], rs[8], a[8], b[8], sc[8];
    V8<float>::ld(mean + cg * 8, mu);
    V8<float>::ld(rstd + cg * 8, rs);
    fn_coeffs<T>(gamma, beta, emb, ld, n, C, cg * 8, a, b, sc);
    const int64_t base = (int64_t)n * rows * C + cg * 8;
    const FnRows w = fn_rows(rows);
    for (int64_t rb = w.r0 + rr; rb < w.r1; rb += (int64_t)R * FV) {
        float v[FV][8];
        uint2 mv[FV];
#pragma unroll
        for (int k = 0; k < FV; ++k) {
            const int64_t r = rb + (int64_t)k * R;
            if (r < w.r1) {
                V8<T>::ld(x + base + r * C, v[k]);
                mv[k] = keep(base + r * C);
            }
        }
#pragma unroll
        for (int k = 0; k < FV; ++k) {
            const int64_t r = rb + (int64_t)k * R;
            if (r < w.r1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xh = (v[k][e] - mu[e]) * rs[e];
                    v[k][e] = fn_mk(mv[k], e, ks) * fn_act<ACT, sizeof(T) == 4>(fmaf(xh, a[e], b[e]));
                }
                V8<T>::st(out + base + r * C, v[k]);
            }
        }
    }
}

// ws: [N][slabs][2][C] partial (S0, S1), then [2][C] = (dbeta / M, dgamma / M)
template <typename T, int ACT, typename KS>
__global__ __launch_bounds__(256) void film_norm_bwd_reduce_k(const T* g, const T* x, int64_t rows, int G, int R, const float* mean,
                                                              const float* rstd, const float* gamma, const float* beta,
                                                              const T* emb, int64_t ld, KS keep, float keep_scale,
                                                              float* ws) {
    __shared__ __attribute__((aligned(16))) float red[2][256 * 8];
    const int cg = threadIdx.x % G, rr = threadIdx.x / G;
    const int C = G * 8, n = blockIdx.y;
    const float ks = keep.on() ? keep_scale : 1.f;
    float s0[8], s1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
    if (rr < R) {
        float mu[8], rs[8], a[8], b[8], sc[8];
        V8<float>::ld(mean + cg * 8, mu);
        V8<float>::ld(rstd + cg * 8, rs);
        fn_coeffs<T>(gamma, beta, emb, ld, n, C, cg * 8, a, b, sc);
        const int64_t base = (int64_t)n * rows * C + cg * 8;
        const FnRows w = fn_rows(rows);
        for (int64_t rb = w.r0 + rr; rb < w.r1; rb += (int64_t)R * FV) {
            float v[FV][8], gv[FV][8];
            uint2 mv[FV];
#pragma unroll
            for (int k = 0; k < FV; ++k) {
                const int64_t r = rb + (int64_t)k * R;
                if (r < w.r1) {
                    V8<T>::ld(x + base + r * C, v[k]);
                    V8<T>::ld(g + base + r * C, gv[k]);
                    mv[k] = keep(base + r * C);
                }
            }
#pragma unroll
            for (int k = 0; k < FV; ++k) {
                const int64_t r = rb + (int64_t)k * R;
                if (r < w.r1) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float xh = (v[k][e] - mu[e]) * rs[e];
                        const float du = gv[k][e] * fn_mk(mv[k], e, ks) * fn_dact<ACT, sizeof(T) == 4>(fmaf(xh, a[e], b[e]));
                        s0[e] += du;
                        s1[e] = fmaf(du, xh, s1[e]);
                    }
                }
            }
        }
        V8<float>::st(&red[0][threadIdx.x * 8], s0);
        V8<float>::st(&red[1][threadIdx.x * 8], s1);
    }
    __syncthreads();
    if (rr == 0) {                     // the R row lanes of a channel group in the order of the lanes
#pragma unroll
        for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
        for (int l = 0; l < R; ++l) {
            float p0[8], p1[8];
            V8<float>::ld(&red[0][(l * G + cg) * 8], p0);
            V8<float>::ld(&red[1][(l * G + cg) * 8], p1);
#pragma unroll
            for (int e = 0; e < 8; ++e) { s0[e] += p0[e]; s1[e] += p1[e]; }
        }
        float* dst = ws + ((int64_t)n * gridDim.x + blockIdx.x) * 2 * C + cg * 8;
        V8<float>::st(dst, s0);
        V8<float>::st(dst + C, s1);
    }
}

// One workgroup of 16 waves per 8 channels; wave w takes the samples w, w + 16, ...  The 8 row lanes of a wave split the slabs
// of a sample and meet by shuffles, the 16 waves meet through LDS in the order of the waves: fp64 throughout.
template <typename T>
__global__ __launch_bounds__(1024) void film_norm_bwd_finalize_k(float* ws, int N, int slabs, int C, double inv_m, const float* gamma,
                                                                 const float* beta, const T* emb, int64_t ld, T* demb,
                                                                 float* dgamma, float* dbeta) {
    __shared__ double red[2][16][8];
    const int cl = threadIdx.x & 7, rl = (threadIdx.x >> 3) & 7, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * 8 + cl;            // C is a multiple of 8: always a channel
    const double gm = gamma[c], bt = beta[c];
    double ab = 0.0, ag = 0.0;                    // this wave's part of dbeta, dgamma
    for (int n = wv; n < N; n += 16) {
        const float* p = ws + (int64_t)n * slabs * 2 * C + c;
        double t0 = 0.0, t1 = 0.0;
        for (int sl = rl; sl < slabs; sl += 8) {
            t0 += (double)p[(int64_t)sl * 2 * C];
            t1 += (double)p[(int64_t)sl * 2 * C + C];
        }
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) {
            t0 += __shfl_xor(t0, o, 64);
            t1 += __shfl_xor(t1, o, 64);
        }
        double sc = 1.0;
        if (emb) {
            sc = 1.0 + (double)Conv<T>::ld(emb + (int64_t)n * ld + c);
            if (rl == 0) {
                Conv<T>::st(demb + (int64_t)n * ld + c, (float)(gm * t1 + bt * t0));     // ds
                Conv<T>::st(demb + (int64_t)n * ld + C + c, (float)t0);                  // dt
            }
        }
        ab += sc * t0;
        ag += sc * t1;
    }
    if (rl == 0) {
        red[0][wv][cl] = ab;
        red[1][wv][cl] = ag;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        ab = ag = 0.0;
#pragma unroll
        for (int l = 0; l < 16; ++l) { ab += red[0][l][cl]; ag += red[1][l][cl]; }
        if (dbeta) dbeta[c] += (float)ab;
        if (dgamma) dgamma[c] += (float)ag;
        float* tail = ws + (int64_t)N * slabs * 2 * C;
        tail[c] = (float)(ab * inv_m);
        tail[C + c] = (float)(ag * inv_m);
    }
}

// dx = du p - q - xhat w with p = gamma (1 + s) rstd, q = gamma rstd dbeta / M, w = gamma rstd dgamma / M
template <typename T, int ACT, typename KS>
__global__ __launch_bounds__(256) void film_norm_bwd_apply_k(const T* g, const T* x, int64_t rows, int G, int R, const float* mean,
                                                             const float* rstd, const float* gamma, const float* beta,
                                                             const T* emb, int64_t ld, KS keep, float keep_scale,
                                                             const float* tail, T* dx) {
    const int cg = threadIdx.x % G, rr = threadIdx.x / G;
    if (rr >= R) return;
    const int C = G * 8, n = blockIdx.y;
    const float ks = keep.on() ? keep_scale : 1.f;
    float mu[8], rs[8], a[8], b[8], p[8], qv[8], wv[8];
    V8<float>::ld(mean + cg * 8, mu);
    V8<float>::ld(rstd + cg * 8, rs);
    V8<float>::ld(gamma + cg * 8, p);             // gamma, for q and w, before fn_coeffs folds 1 + s into a
    V8<float>::ld(tail + cg * 8, qv);
    V8<float>::ld(tail + C + cg * 8, wv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float gr = p[e] * rs[e];
        qv[e] *= gr;
        wv[e] *= gr;
    }
    fn_coeffs<T>(gamma, beta, emb, ld, n, C, cg * 8, a, b, p);
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = a[e] * rs[e];
    const int64_t base = (int64_t)n * rows * C + cg * 8;
    const FnRows w = fn_rows(rows);
    for (int64_t rb = w.r0 + rr; rb < w.r1; rb += (int64_t)R * FV) {
        float v[FV][8], gv[FV][8];
        uint2 mv[FV];
#pragma unroll
        for (int k = 0; k < FV; ++k) {
            const int64_t r = rb + (int64_t)k * R;
            if (r < w.r1) {
                V8<T>::ld(x + base + r * C, v[k]);
                V8<T>::ld(g + base + r * C, gv[k]);
                mv[k] = keep(base + r * C);
            }
        }
#pragma unroll
        for (int k = 0; k < FV; ++k) {
            const int64_t r = rb + (int64_t)k * R;
            if (r < w.r1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xh = (v[k][e] - mu[e]) * rs[e];
                    const float du = gv[k][e] * fn_mk(mv[k], e, ks) * fn_dact<ACT, sizeof(T) == 4>(fmaf(xh, a[e], b[e]));
                    v[k][e] = fmaf(du, p[e], -fmaf(xh, wv[e], qv[e]));
                }
                V8<T>::st(dx + base + r * C, v[k]);
            }
        }
    }
}

extern "C" int pai_film_norm_slabs(int64_t rows) {
    if (rows < 1) return 0;
    return (int)min((int64_t)FN_MAX_SLABS, (rows + FN_SLAB_ROWS - 1) / FN_SLAB_ROWS);
}

extern "C" int64_t pai_film_norm_ws_floats(int N, int64_t rows, int C) {
    if (N < 1 || rows < 1 || C < 1) return 0;
    return (int64_t)N * pai_film_norm_slabs(rows) * 2 * C + 2 * (int64_t)C;
}

static int film_norm_check(const char* who, int dtype, int64_t rows, int N, int C, const void* emb, int64_t ld, int act) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "%s: dtype=%d", who, dtype);
    PAI_CHECK(act == PAI_ACT_NONE || act == PAI_ACT_SILU, "%s: act=%d (none or SiLU)", who, act);
    PAI_CHECK(N >= 1 && N <= 65535 && rows >= 1, "%s: N=%d rows=%lld (N at most 65535)", who, N, (long long)rows);
    PAI_CHECK(C >= 8 && C % 8 == 0 && C <= 2048, "%s: C=%d (a multiple of 8, at most 2048)", who, C);
    PAI_CHECK(!emb || ld >= 2 * (int64_t)C, "%s: ld=%lld is less than 2 C = %d", who, (long long)ld, 2 * C);
    return 0;
}

// The launches of both forms: `keep` is the mask pointer or the Philox tuple; the caller has checked what is its own.
template <typename KS>
static int film_norm_fwd_launch(const char* who, int dtype, const void* x, int64_t rows, int N, int C, const float* mean,
                                const float* rstd, const float* gamma, const float* beta, const void* emb, int64_t ld, KS keep,
                                float keep_scale, int act, void* out, void* stream) {
    if (film_norm_check(who, dtype, rows, N, C, emb, ld, act)) return 1;
    PAI_CHECK(x && mean && rstd && gamma && beta && out, "%s: null tensor", who);
    PAI_CHECK((((uintptr_t)x) | ((uintptr_t)out) | ((uintptr_t)mean) | ((uintptr_t)rstd) | ((uintptr_t)gamma) | ((uintptr_t)beta)) % 16 == 0 &&
                  keep.aligned(),
              "%s: tensors must be 16-byte aligned (the mask 8-byte)", who);
    const int G = C / 8, R = 256 / G;
    const dim3 grid(pai_film_norm_slabs(rows), N);
    hipStream_t s = (hipStream_t)stream;
#define PAI_FN_FWD(TT, ACT)                                                                                                        \
    PAI_LAUNCH((film_norm_fwd_k<TT, ACT, KS>), grid, dim3(256), 0, s, (const TT*)x, rows, G, R, mean, rstd, gamma, beta, \
                       (const TT*)emb, ld, keep, keep_scale, (TT*)out)
    if (dtype == PAI_F32) {
        if (act == PAI_ACT_SILU) PAI_FN_FWD(float, PAI_ACT_SILU); else PAI_FN_FWD(float, PAI_ACT_NONE);
    } else {
        if (act == PAI_ACT_SILU) PAI_FN_FWD(bf16_t, PAI_ACT_SILU); else PAI_FN_FWD(bf16_t, PAI_ACT_NONE);
    }
#undef PAI_FN_FWD
    PAI_LAUNCH_CHECK();
    return 0;
}

template <typename KS>
static int film_norm_bwd_launch(const char* who, int dtype, const void* g, const void* x, int64_t rows, int N, int C,
                                const float* mean, const float* rstd, const float* gamma, const float* beta, const void* emb,
                                int64_t ld, KS keep, float keep_scale, int act, void* dx, void* demb, float* dgamma, float* dbeta,
                                float* ws, void* stream) {
    if (film_norm_check(who, dtype, rows, N, C, emb, ld, act)) return 1;
    PAI_CHECK(g && x && mean && rstd && gamma && beta && dx && ws, "%s: null tensor", who);
    PAI_CHECK(!emb || demb, "%s: emb without demb", who);
    PAI_CHECK((((uintptr_t)g) | ((uintptr_t)x) | ((uintptr_t)dx) | ((uintptr_t)ws) | ((uintptr_t)mean) | ((uintptr_t)rstd) |
               ((uintptr_t)gamma) | ((uintptr_t)beta)) % 16 == 0 && keep.aligned(),
              "%s: tensors must be 16-byte aligned (the mask 8-byte)", who);
    const int G = C / 8, R = 256 / G, slabs = pai_film_norm_slabs(rows);
    const dim3 grid(slabs, N);
    float* tail = ws + (int64_t)N * slabs * 2 * C;
    const double inv_m = 1.0 / ((double)N * (double)rows);
    hipStream_t s = (hipStream_t)stream;
#define PAI_FN_BWD(TT, ACT)                                                                                                        \
    PAI_LAUNCH((film_norm_bwd_reduce_k<TT, ACT, KS>), grid, dim3(256), 0, s, (const TT*)g, (const TT*)x, rows, G, R, mean, \
                       rstd, gamma, beta, (const TT*)emb, ld, keep, keep_scale, ws);                                               \
    PAI_LAUNCH((film_norm_bwd_finalize_k<TT>), dim3(C / 8), dim3(1024), 0, s, ws, N, slabs, C, inv_m, gamma, beta,        \
                       (const TT*)emb, ld, (TT*)demb, dgamma, dbeta);                                                              \
    PAI_LAUNCH((film_norm_bwd_apply_k<TT, ACT, KS>), grid, dim3(256), 0, s, (const TT*)g, (const TT*)x, rows, G, R, mean,  \
                       rstd, gamma, beta, (const TT*)emb, ld, keep, keep_scale, (const float*)tail, (TT*)dx)
    if (dtype == PAI_F32) {
        if (act == PAI_ACT_SILU) { PAI_FN_BWD(float, PAI_ACT_SILU); } else { PAI_FN_BWD(float, PAI_ACT_NONE); }
    } else {
        if (act == PAI_ACT_SILU) { PAI_FN_BWD(bf16_t, PAI_ACT_SILU); } else { PAI_FN_BWD(bf16_t, PAI_ACT_NONE); }
    }
#undef PAI_FN_BWD
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_film_norm_fwd(int dtype, const void* x, int64_t rows, int N, int C, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, const void* emb, int64_t ld, const unsigned char* mask,
                                 float keep_scale, int act, void* out, void* stream) {
    return film_norm_fwd_launch("pai_film_norm_fwd", dtype, x, rows, N, C, mean, rstd, gamma, beta, emb, ld, FnMaskSrc{mask},
                                keep_scale, act, out, stream);
}

extern "C" int pai_film_norm_bwd(int dtype, const void* g, const void* x, int64_t rows, int N, int C, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, const void* emb, int64_t ld,
                                 const unsigned char* mask, float keep_scale, int act, void* dx, void* demb, float* dgamma,
                                 float* dbeta, float* ws, void* stream) {
    return film_norm_bwd_launch("pai_film_norm_bwd", dtype, g, x, rows, N, C, mean, rstd, gamma, beta, emb, ld, FnMaskSrc{mask},
                                keep_scale, act, dx, demb, dgamma, dbeta, ws, stream);
}

// The Philox forms: one block per vector of eight elements, block = flat offset / 8 (philox.h).
static int film_norm_rng_check(const char* who, int64_t rows, int N, int C, uint32_t thr) {
    PAI_CHECK(thr <= 65536u, "%s: thr=%u (round(p 65536), at most 65536)", who, thr);
    PAI_CHECK(N < 1 || rows < 1 || C < 8 || rows <= ((1ll << 35) / C) / N, "%s: tensor too large (more than 2^32 blocks of 8)", who);
    return 0;
}

extern "C" int pai_film_norm_fwd_rng(int dtype, const void* x, int64_t rows, int N, int C, const float* mean, const float* rstd,
                                     const float* gamma, const float* beta, const void* emb, int64_t ld, uint64_t seed,
                                     uint32_t stream, uint32_t step, uint32_t thr, float keep_scale, int act, void* out,
                                     void* stream_handle) {
    if (film_norm_rng_check("pai_film_norm_fwd_rng", rows, N, C, thr)) return 1;
    return film_norm_fwd_launch("pai_film_norm_fwd_rng", dtype, x, rows, N, C, mean, rstd, gamma, beta, emb, ld,
                                FnRngSrc{philox_key(seed, 0, stream, step), thr}, keep_scale, act, out, stream_handle);
}

extern "C" int pai_film_norm_bwd_rng(int dtype, const void* g, const void* x, int64_t rows, int N, int C, const float* mean,
                                     const float* rstd, const float* gamma, const float* beta, const void* emb, int64_t ld,
                                     uint64_t seed, uint32_t stream, uint32_t step, uint32_t thr, float keep_scale, int act,
                                     void* dx, void* demb, float* dgamma, float* dbeta, float* ws, void* stream_handle) {
    if (film_norm_rng_check("pai_film_norm_bwd_rng", rows, N, C, thr)) return 1;
    return film_norm_bwd_launch("pai_film_norm_bwd_rng", dtype, g, x, rows, N, C, mean, rstd, gamma, beta, emb, ld,
                                FnRngSrc{philox_key(seed, 0, stream, step), thr}, keep_scale, act, dx, demb, dgamma, dbeta, ws,
                                stream_handle);
}
