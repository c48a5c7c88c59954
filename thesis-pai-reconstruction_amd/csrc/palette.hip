// Palette sampling (reference models/palette.py:79-100,233-306 and models/guided_diffusion/unet.py, nn.py): the kernels the
// eval-mode guided-diffusion U-Net and the reverse step need beside the convolution family, the attention's backward, and the
// training objective.
//
//   pai_sattn_fwd        QKVAttentionLegacy (unet.py:265-297) over the T = H * W tokens of a level, flash style: the T x T
//                        scores are never stored.  bf16: one workgroup of four waves per 128 queries of one (image, head),
//                        each wave 32 queries, the K / V tiles shared through LDS.  Both products run on
//                        v_mfma_f32_32x32x16_bf16 in the orientation that keeps every per-query quantity on the query's own
//                        lane: S^T = K Q^T has the query on the lane and the keys in the 16 registers, and O^T = V^T P^T
//                        takes that accumulator, rounded to bf16, directly as its B operand and again has the query on
//                        the lane -- running max, running sum and the rescale factor never cross lanes except for the one
//                        exchange between the two lane halves that split a query's keys.  V^T fragments come from a
//                        row-major LDS image through ds_read_b64_tr_b16 in the k order the accumulator imposes.  The
//                        rescale happens at every tile (no deferred maximum).  fp32 (parity mode): a vector-ALU kernel with
//                        the same online softmax, sequential FMA chains.
//   pai_sattn_fwd_lse    the same kernels with the lse output (natural-log sum-exp of every query's scaled scores).
//   pai_sattn_bwd        its backward from qkv, out, lse and dout in three launches (delta; dK / dV, key on the lane; dQ, query
//                        on the lane), no sum across workgroups: in front of the kernels below.
//   pai_affine_act       out = act(x * A + B), A / B per channel or per (sample, channel): every BatchNorm (eval) + SiLU
//                        site of the network, FiLM included.
//   pai_film_coeffs      A = a (1 + scale), B = b (1 + scale) + shift from the BatchNorm eval coefficients and emb_out.
//   pai_avgpool2         2 x 2 mean (Downsample(use_conv=False)).
//   pai_avgpool2_bwd     its backward: dout / 4 to the four positions (training).
//   pai_silu_bwd         du = g SiLU'(u): the two SiLUs of the embedding path (training).
//   pai_gamma_embedding  [cos(g f_i) | sin(g f_i)] (nn.py:140-157).
//   pai_palette_step     one reverse diffusion step, elementwise (palette.py:233-306).
//   pai_palette_noise    the forward noising q(y_t | y_0) with t, gammas and gammas_prev on the device (palette.py:214-231; training).
//   pai_palette_step_rng, pai_palette_noise_rng  the same two kernels with their random numbers drawn inside (philox.h).
//   pai_palette_objective  the MSE + variational-bound loss and its gradient into the U-Net output (palette.py:122-140, 254-333,
//                        368-427; training): a pass over (slab, sample) workgroups with fp64 partial sums, then one workgroup
//                        that adds them in a fixed order.
#include "common.h"
#include "philox.h"

#include <math.h>

typedef __attribute__((ext_vector_type(8))) __bf16 pbf8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 pbf4_t;
typedef __attribute__((ext_vector_type(16))) float pf16_t;

// ---- spatial self-attention, bf16 -------------------------------------------------------------------------------------------
// LDS images of a K / V tile: rows of CH bf16, the 16-byte chunks of a row permuted by an XOR that depends on the row.
//   K is read row-wise (ds_read_b128: lane = key row, one chunk per k-step): the XOR spreads the 16 rows of a lane group
//   over the 16 chunk slots of a 256-byte bank line.
//   V is read through the transposed 4-row x 16-column blocks: the XOR moves the four rows of a block to different 64-byte
//   quarters of the bank line.
template <int CH> __device__ __forceinline__ int sattn_kswz(int row) {
    constexpr int CPR = CH / 8;
    if (CPR >= 16) return row & 15;
    constexpr int SH = CPR == 8 ? 1 : 2;          // rows per 256 bytes: 2 (CH 64), 4 (CH 32)
    return (row >> SH) & (CPR - 1);
}
template <int CH> __device__ __forceinline__ int sattn_vswz(int row) {
    constexpr int CPR = CH / 8;
    if (CPR >= 16) return (row & 3) << 2;
    if (CPR == 8) return ((row >> 1) & 1) << 2;
    return 0;
}

// A-operand fragment of O^T = V^T P^T for the 16 keys R0 .. R0 + 15 of the tile and the 32 channels d0 .. d0 + 31: element j
// of lane (r = lane & 31, hh = lane >> 5) is V[R0 + 8 (j >> 2) + 4 hh + (j & 3)][d0 + r] -- the key order of registers
// 8s .. 8s + 7 of the S^T accumulator.  Two transposed reads of 4 rows x 16 columns per 16-lane group.
template <int CH>
__device__ __forceinline__ pbf8_t sattn_vt_frag(const bf16_t* Vs, int R0, int d0, int lane) {
    const int q = (lane & 15) >> 2, p = lane & 3, hh = lane >> 5;
    const int col = d0 + 16 * ((lane >> 4) & 1) + 4 * p;
    const int rlo = R0 + 4 * hh + q, rhi = rlo + 8;
    const bf16_t* alo = Vs + rlo * CH + 8 * ((col >> 3) ^ sattn_vswz<CH>(rlo)) + (col & 7);
    const bf16_t* ahi = Vs + rhi * CH + 8 * ((col >> 3) ^ sattn_vswz<CH>(rhi)) + (col & 7);
    typedef pbf4_t __attribute__((address_space(3))) * lds4_t;
    const pbf4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4_t)(const void*)alo);
    const pbf4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4_t)(const void*)ahi);
    return (pbf8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int CH>
__global__ __launch_bounds__(256) void sattn_bf16_k(const bf16_t* qkv, int T, int heads, float scale2, bf16_t* out,
                                                    float* lse) {
    constexpr int KVB = CH > 128 ? 32 : 64;       // keys per tile
    constexpr int NS = KVB / 32;                  // 32-key sub-tiles
    constexpr int CPR = CH / 8;                   // 16-byte chunks per row
    constexpr int KS = CH / 16;                   // k-steps of S^T
    constexpr int DB = CH / 32;                   // 32-channel blocks of O^T
    constexpr bool QREG = CH <= 128;              // Q fragments stay in registers (CH 256: read again per tile, L1 hits)
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KVB * CH];
    __shared__ __attribute__((aligned(16))) bf16_t Vs[KVB * CH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int n = blockIdx.y / heads, h = blockIdx.y - n * heads;
    const int64_t RS = (int64_t)heads * 3 * CH;
    const bf16_t* base = qkv + (int64_t)n * T * RS + (int64_t)h * 3 * CH;
    const int q0 = blockIdx.x * 128 + w * 32;
    const bool active = q0 < T;                   // wave-uniform
    const int qi = q0 + r;
    const bf16_t* qrow = base + (int64_t)min(qi, T - 1) * RS;
    pbf8_t qf[QREG ? KS : 1];
    if (QREG) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const pbf8_t*)(qrow + 16 * ks + 8 * hh);
    }
    pf16_t o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int t = 0; t < 16; ++t) o[d][t] = 0.f;
    float m = -INFINITY, l = 0.f;                 // running maximum (shared by the two lane halves) and this lane's part of the sum

    for (int k0 = 0; k0 < T; k0 += KVB) {
        __syncthreads();                          // the previous tile has been read
        for (int c = tid; c < KVB * CPR; c += 256) {
            const int row = c / CPR, ch = c - row * CPR;
            uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
            if (k0 + row < T) {                   // the key tail is zero-filled, never read
                const bf16_t* src = base + (int64_t)(k0 + row) * RS + CH + 8 * ch;
                kv = *(const uint4*)src;
                vv = *(const uint4*)(src + CH);
            }
            *(uint4*)(Ks + row * CH + 8 * (ch ^ sattn_kswz<CH>(row))) = kv;
            *(uint4*)(Vs + row * CH + 8 * (ch ^ sattn_vswz<CH>(row))) = vv;
        }
        __syncthreads();
        if (!active) continue;
        // S^T = K Q^T: D[row key][col query]; register t of lane (r, hh) is key 8 (t >> 2) + 4 hh + (t & 3) of the sub-tile
        pf16_t s[NS];
        float mx = -INFINITY;
#pragma unroll
        for (int sb = 0; sb < NS; ++sb) {
#pragma unroll
            for (int t = 0; t < 16; ++t) s[sb][t] = 0.f;
            const int krow = 32 * sb + r;
            const bf16_t* kr = Ks + krow * CH;
            const int kx = sattn_kswz<CH>(krow);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const pbf8_t kf = *(const pbf8_t*)(kr + 8 * ((2 * ks + hh) ^ kx));
                const pbf8_t qv = QREG ? qf[QREG ? ks : 0] : *(const pbf8_t*)(qrow + 16 * ks + 8 * hh);
                s[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qv, s[sb], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int key = k0 + 32 * sb + 8 * (t >> 2) + 4 * hh + (t & 3);
                const float v = key < T ? s[sb][t] * scale2 : -INFINITY;     // s * s on the fp32 score
                s[sb][t] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // the other half of this query's keys
        const float mn = fmaxf(m, mx);            // finite: key k0 of every tile exists
        const float alpha = __expf(m - mn);       // 0 at the first tile (m = -inf)
        m = mn;
        float ls = 0.f;
        pbf8_t pf[NS][2];
#pragma unroll
        for (int sb = 0; sb < NS; ++sb)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float p = __expf(s[sb][t] - mn);
                ls += p;
                pf[sb][t >> 3][t & 7] = (__bf16)p;
            }
        l = fmaf(l, alpha, ls);
        // O^T = O^T alpha + V^T P^T: D[row channel][col query]
#pragma unroll
        for (int d = 0; d < DB; ++d) {
#pragma unroll
            for (int t = 0; t < 16; ++t) o[d][t] *= alpha;
#pragma unroll
            for (int sb = 0; sb < NS; ++sb)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
                    o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sattn_vt_frag<CH>(Vs, 32 * sb + 16 * s2, 32 * d, lane),
                                                                   pf[sb][s2], o[d], 0, 0, 0);
        }
    }
    if (!active) return;
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if (qi < T) {
        if (lse && hh == 0) lse[(int64_t)blockIdx.y * T + qi] = m + logf(l);      // [n][h][t], natural log
        bf16_t* orow = out + ((int64_t)n * T + qi) * heads * CH + (int64_t)h * CH;
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {         // registers 4g .. 4g + 3: channels 32 d + 8 g + 4 hh + (0 .. 3)
                uint2 pk;
                pk.x = pk2bf(o[d][4 * g] * inv, o[d][4 * g + 1] * inv);
                pk.y = pk2bf(o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv);
                *(uint2*)(orow + 32 * d + 8 * g + 4 * hh) = pk;
            }
    }
}

// ---- spatial self-attention, fp32 (parity mode) -------------------------------------------------------------------------
// 32 queries per workgroup, eight threads per query: each takes every eighth key of the tile for the scores and a slice of
// the channels for the output.  Sequential FMA chains over the channels (scores) and over the keys (output).
template <int CH, int KVB>
__global__ __launch_bounds__(256) void sattn_f32_k(const float* qkv, int T, int heads, float scale2, float* out, float* lse) {
    constexpr int NE = KVB / 8, ND = CH / 32;
    __shared__ __attribute__((aligned(16))) float Ks[KVB * CH];
    __shared__ __attribute__((aligned(16))) float Vs[KVB * CH];
    __shared__ float Ps[32][KVB + 1];
    const int tid = threadIdx.x, ql = tid >> 3, g = tid & 7;
    const int n = blockIdx.y / heads, h = blockIdx.y - n * heads;
    const int64_t RS = (int64_t)heads * 3 * CH;
    const float* base = qkv + (int64_t)n * T * RS + (int64_t)h * 3 * CH;
    const int qi = blockIdx.x * 32 + ql;
    const float* qrow = base + (int64_t)min(qi, T - 1) * RS;
    float4 o[ND];
#pragma unroll
    for (int e = 0; e < ND; ++e) o[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < T; k0 += KVB) {
        __syncthreads();
        for (int c = tid; c < KVB * (CH / 4); c += 256) {
            const int row = c / (CH / 4), c4 = c - row * (CH / 4);
            float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
            if (k0 + row < T) {
                const float* src = base + (int64_t)(k0 + row) * RS + CH + 4 * c4;
                kv = *(const float4*)src;
                vv = *(const float4*)(src + CH);
            }
            *(float4*)(Ks + row * CH + 4 * c4) = kv;
            *(float4*)(Vs + row * CH + 4 * c4) = vv;
        }
        __syncthreads();
        float s[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) s[e] = 0.f;
        for (int c = 0; c < CH; c += 4) {
            const float4 qv = *(const float4*)(qrow + c);
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const float4 kv = *(const float4*)(Ks + (g + 8 * e) * CH + c);
                s[e] = fmaf(qv.x, kv.x, s[e]);
                s[e] = fmaf(qv.y, kv.y, s[e]);
                s[e] = fmaf(qv.z, kv.z, s[e]);
                s[e] = fmaf(qv.w, kv.w, s[e]);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            s[e] = (k0 + g + 8 * e) < T ? s[e] * scale2 : -INFINITY;
            mx = fmaxf(mx, s[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = expf(m - mn);
        m = mn;
        float ls = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const float p = expf(s[e] - mn);
            Ps[ql][g + 8 * e] = p;
            ls += p;
        }
        ls += __shfl_xor(ls, 1, 64);
        ls += __shfl_xor(ls, 2, 64);
        ls += __shfl_xor(ls, 4, 64);
        l = fmaf(l, alpha, ls);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < ND; ++e) { o[e].x *= alpha; o[e].y *= alpha; o[e].z *= alpha; o[e].w *= alpha; }
        for (int k = 0; k < KVB; ++k) {
            const float p = Ps[ql][k];
#pragma unroll
            for (int e = 0; e < ND; ++e) {
                const float4 v = *(const float4*)(Vs + k * CH + 4 * g + 32 * e);
                o[e].x = fmaf(p, v.x, o[e].x);
                o[e].y = fmaf(p, v.y, o[e].y);
                o[e].z = fmaf(p, v.z, o[e].z);
                o[e].w = fmaf(p, v.w, o[e].w);
            }
        }
    }
    if (qi < T) {
        float* orow = out + ((int64_t)n * T + qi) * heads * CH + (int64_t)h * CH;
        const float inv = 1.0f / l;
        if (lse && g == 0) lse[(int64_t)blockIdx.y * T + qi] = m + logf(l);
#pragma unroll
        for (int e = 0; e < ND; ++e)
            *(float4*)(orow + 4 * g + 32 * e) = make_float4(o[e].x * inv, o[e].y * inv, o[e].z * inv, o[e].w * inv);
    }
}

// ---- spatial self-attention, backward ------------------------------------------------------------------------------------
// Three launches, none of which adds across workgroups: no atomics, no hand-off.  P is recomputed from q, k and the forward's
// lse (P_ij = exp(scale2 s_ij - lse_i), the exponent one difference), so S is computed twice -- once per kernel below.
//   delta     ws[n][h][i] = sum_c dO_ic O_ic, a streaming row dot.
//   kv        one workgroup per 128 keys of one (image, head), a wave per 32 keys: key on the lane.  K and V fragments stay in
//             registers as B operands; S = Q K^T and dP = dO V^T take the Q / dO rows of a query tile from LDS (K swizzle) and
//             have the key on the lane and the queries in the 16 registers, so P and dS, rounded once to bf16, are the B
//             operands of dV^T += dO^T P and dK^T += Q^T dS; dO^T / Q^T come through ds_read_b64_tr_b16 from a second LDS image
//             (V swizzle) in the k order the accumulator imposes (sattn_vt_frag).  dK^T / dV^T stay in accumulators for the
//             whole sweep over the queries.
//   q         the forward's structure, query on the lane: S^T = K Q^T and dP^T = V dO^T with K / V rows from LDS and the
//             Q / dO fragments in registers, dS^T rounded once to bf16 as the B operand of dQ^T += K^T dS^T, K^T through
//             ds_read_b64_tr_b16 from a second image of K.
// Queries (kv) and keys (q) past T are zero-filled in LDS and get P = 0 explicitly.
template <typename T, int CH>
__global__ __launch_bounds__(256) void sattn_bwd_delta_k(const T* dout, const T* out, int64_t rows, int Tn, int heads, float* ws) {
    constexpr int L = CH / 8;                     // lanes per row
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gi / L;                   // (n * Tn + t) * heads + h
    const int sub = (int)(gi - row * L);
    float acc = 0.f;
    if (row < rows) {                             // the tail lanes add 0 and still take part in the shuffles below
        float a[8], b[8];
        V8<T>::ld(dout + row * CH + 8 * sub, a);
        V8<T>::ld(out + row * CH + 8 * sub, b);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = fmaf(a[i], b[i], acc);
    }
#pragma unroll
    for (int o = 1; o < L; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (row < rows && sub == 0) {
        const int64_t nt = row / heads;
        const int h = (int)(row - nt * heads);
        const int64_t n = nt / Tn;
        ws[(n * heads + h) * Tn + (nt - n * Tn)] = acc;
    }
}

template <int CH>
__global__ __launch_bounds__(256) void sattn_bwd_kv_bf16_k(const bf16_t* qkv, const bf16_t* dout, const float* lse,
                                                           const float* delta, int T, int heads, float scale2, bf16_t* dqkv) {
    constexpr int QB = CH > 64 ? 32 : 64;         // queries per tile
    constexpr int NS = QB / 32;
    constexpr int CPR = CH / 8;
    constexpr int KS = CH / 16;
    constexpr int DB = CH / 32;
    __shared__ __attribute__((aligned(16))) bf16_t Qr[QB * CH];      // K swizzle: row reads
    __shared__ __attribute__((aligned(16))) bf16_t Qt[QB * CH];      // V swizzle: transposed reads
    __shared__ __attribute__((aligned(16))) bf16_t Dr[QB * CH];
    __shared__ __attribute__((aligned(16))) bf16_t Dt[QB * CH];
    __shared__ __attribute__((aligned(16))) float Ls[QB];
    __shared__ __attribute__((aligned(16))) float Es[QB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int n = blockIdx.y / heads, h = blockIdx.y - n * heads;
    const int64_t RS = (int64_t)heads * 3 * CH, OS = (int64_t)heads * CH;
    const bf16_t* base = qkv + (int64_t)n * T * RS + (int64_t)h * 3 * CH;
    const bf16_t* dob = dout + (int64_t)n * T * OS + (int64_t)h * CH;
    const float* lrow = lse + (int64_t)blockIdx.y * T;
    const float* erow = delta + (int64_t)blockIdx.y * T;
    const int kw0 = blockIdx.x * 128 + w * 32;
    const bool active = kw0 < T;                  // wave-uniform
    const int kj = kw0 + r;
    const bool kvalid = kj < T;
    const bf16_t* krow = base + (int64_t)min(kj, T - 1) * RS + CH;
    pbf8_t kf[KS], vf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        kf[ks] = *(const pbf8_t*)(krow + 16 * ks + 8 * hh);
        vf[ks] = *(const pbf8_t*)(krow + CH + 16 * ks + 8 * hh);
    }
    pf16_t dk[DB], dv[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int t = 0; t < 16; ++t) dk[d][t] = dv[d][t] = 0.f;

    for (int q0 = 0; q0 < T; q0 += QB) {
        __syncthreads();                          // the previous tile has been read
        for (int c = tid; c < QB * CPR; c += 256) {
            const int row = c / CPR, ch = c - row * CPR;
            uint4 qv = make_uint4(0, 0, 0, 0), dv4 = make_uint4(0, 0, 0, 0);
            if (q0 + row < T) {                   // the query tail is zero-filled, never read
                qv = *(const uint4*)(base + (int64_t)(q0 + row) * RS + 8 * ch);
                dv4 = *(const uint4*)(dob + (int64_t)(q0 + row) * OS + 8 * ch);
            }
            const int ok = row * CH + 8 * (ch ^ sattn_kswz<CH>(row)), ov = row * CH + 8 * (ch ^ sattn_vswz<CH>(row));
            *(uint4*)(Qr + ok) = qv;
            *(uint4*)(Qt + ov) = qv;
            *(uint4*)(Dr + ok) = dv4;
            *(uint4*)(Dt + ov) = dv4;
        }
        if (tid < QB) {
            const bool in = q0 + tid < T;
            Ls[tid] = in ? lrow[q0 + tid] : 0.f;
            Es[tid] = in ? erow[q0 + tid] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
#pragma unroll
        for (int sb = 0; sb < NS; ++sb) {
            // S = Q K^T and dP = dO V^T: D[row query][col key]; register t of lane (r, hh) is query 8 (t >> 2) + 4 hh + (t & 3)
            pf16_t s, dp;
#pragma unroll
            for (int t = 0; t < 16; ++t) s[t] = dp[t] = 0.f;
            const int qrow = 32 * sb + r;
            const int qx = sattn_kswz<CH>(qrow);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int off = qrow * CH + 8 * ((2 * ks + hh) ^ qx);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const pbf8_t*)(Qr + off), kf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const pbf8_t*)(Dr + off), vf[ks], dp, 0, 0, 0);
            }
            pbf8_t pf[2], df[2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i0 = 32 * sb + 8 * g + 4 * hh;
                const float4 l4 = *(const float4*)(Ls + i0), e4 = *(const float4*)(Es + i0);
                const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = 4 * g + u;
                    // padded queries and padded keys contribute exactly zero
                    const float p = (kvalid && q0 + i0 + u < T) ? __expf(fmaf(s[t], scale2, -lv[u])) : 0.f;
                    const float ds = p * (dp[t] - ev[u]);
                    pf[t >> 3][t & 7] = (__bf16)p;
                    df[t >> 3][t & 7] = (__bf16)ds;
                }
            }
            // dV^T += dO^T P, dK^T += Q^T dS: D[row channel][col key]
#pragma unroll
            for (int d = 0; d < DB; ++d)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    dv[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sattn_vt_frag<CH>(Dt, 32 * sb + 16 * s2, 32 * d, lane), pf[s2],
                                                                    dv[d], 0, 0, 0);
                    dk[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sattn_vt_frag<CH>(Qt, 32 * sb + 16 * s2, 32 * d, lane), df[s2],
                                                                    dk[d], 0, 0, 0);
                }
        }
    }
    if (!kvalid) return;
    bf16_t* grow = dqkv + ((int64_t)n * T + kj) * RS + (int64_t)h * 3 * CH + CH;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {             // registers 4g .. 4g + 3: channels 32 d + 8 g + 4 hh + (0 .. 3)
            uint2 pk;
            pk.x = pk2bf(dk[d][4 * g] * scale2, dk[d][4 * g + 1] * scale2);
            pk.y = pk2bf(dk[d][4 * g + 2] * scale2, dk[d][4 * g + 3] * scale2);
            *(uint2*)(grow + 32 * d + 8 * g + 4 * hh) = pk;
            pk.x = pk2bf(dv[d][4 * g], dv[d][4 * g + 1]);
            pk.y = pk2bf(dv[d][4 * g + 2], dv[d][4 * g + 3]);
            *(uint2*)(grow + CH + 32 * d + 8 * g + 4 * hh) = pk;
        }
}

template <int CH>
__global__ __launch_bounds__(256) void sattn_bwd_q_bf16_k(const bf16_t* qkv, const bf16_t* dout, const float* lse,
                                                          const float* delta, int T, int heads, float scale2, bf16_t* dqkv) {
    constexpr int KVB = 64;                       // keys per tile
    constexpr int NS = KVB / 32;
    constexpr int CPR = CH / 8;
    constexpr int KS = CH / 16;
    constexpr int DB = CH / 32;
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KVB * CH];     // K swizzle: row reads
    __shared__ __attribute__((aligned(16))) bf16_t Vs[KVB * CH];     // K swizzle: row reads
    __shared__ __attribute__((aligned(16))) bf16_t Kt[KVB * CH];     // V swizzle: transposed reads
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int n = blockIdx.y / heads, h = blockIdx.y - n * heads;
    const int64_t RS = (int64_t)heads * 3 * CH, OS = (int64_t)heads * CH;
    const bf16_t* base = qkv + (int64_t)n * T * RS + (int64_t)h * 3 * CH;
    const int q0 = blockIdx.x * 128 + w * 32;
    const bool active = q0 < T;                   // wave-uniform
    const int qi = q0 + r;
    const int qc = min(qi, T - 1);
    const bf16_t* qrow = base + (int64_t)qc * RS;
    const bf16_t* drow = dout + ((int64_t)n * T + qc) * OS + (int64_t)h * CH;
    pbf8_t qf[KS], dof[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = *(const pbf8_t*)(qrow + 16 * ks + 8 * hh);
        dof[ks] = *(const pbf8_t*)(drow + 16 * ks + 8 * hh);
    }
    const float lq = lse[(int64_t)blockIdx.y * T + qc], eq = delta[(int64_t)blockIdx.y * T + qc];
    pf16_t dq[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int t = 0; t < 16; ++t) dq[d][t] = 0.f;

    for (int k0 = 0; k0 < T; k0 += KVB) {
        __syncthreads();                          // the previous tile has been read
        for (int c = tid; c < KVB * CPR; c += 256) {
            const int row = c / CPR, ch = c - row * CPR;
            uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
            if (k0 + row < T) {                   // the key tail is zero-filled, never read
                const bf16_t* src = base + (int64_t)(k0 + row) * RS + CH + 8 * ch;
                kv = *(const uint4*)src;
                vv = *(const uint4*)(src + CH);
            }
            const int ok = row * CH + 8 * (ch ^ sattn_kswz<CH>(row));
            *(uint4*)(Ks + ok) = kv;
            *(uint4*)(Vs + ok) = vv;
            *(uint4*)(Kt + row * CH + 8 * (ch ^ sattn_vswz<CH>(row))) = kv;
        }
        __syncthreads();
        if (!active) continue;
#pragma unroll
        for (int sb = 0; sb < NS; ++sb) {
            // S^T = K Q^T and dP^T = V dO^T: D[row key][col query]; register t of lane (r, hh) is key 8 (t >> 2) + 4 hh + (t & 3)
            pf16_t s, dp;
#pragma unroll
            for (int t = 0; t < 16; ++t) s[t] = dp[t] = 0.f;
            const int krow = 32 * sb + r;
            const int kx = sattn_kswz<CH>(krow);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int off = krow * CH + 8 * ((2 * ks + hh) ^ kx);
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const pbf8_t*)(Ks + off), qf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const pbf8_t*)(Vs + off), dof[ks], dp, 0, 0, 0);
            }
            pbf8_t df[2];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int key = k0 + 32 * sb + 8 * (t >> 2) + 4 * hh + (t & 3);
                const float p = key < T ? __expf(fmaf(s[t], scale2, -lq)) : 0.f;       // keys past T: P = 0
                df[t >> 3][t & 7] = (__bf16)(p * (dp[t] - eq));
            }
            // dQ^T += K^T dS^T: D[row channel][col query]
#pragma unroll
            for (int d = 0; d < DB; ++d)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
                    dq[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sattn_vt_frag<CH>(Kt, 32 * sb + 16 * s2, 32 * d, lane), df[s2],
                                                                    dq[d], 0, 0, 0);
        }
    }
    if (!active || qi >= T) return;
    bf16_t* grow = dqkv + ((int64_t)n * T + qi) * RS + (int64_t)h * 3 * CH;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {             // registers 4g .. 4g + 3: channels 32 d + 8 g + 4 hh + (0 .. 3)
            uint2 pk;
            pk.x = pk2bf(dq[d][4 * g] * scale2, dq[d][4 * g + 1] * scale2);
            pk.y = pk2bf(dq[d][4 * g + 2] * scale2, dq[d][4 * g + 3] * scale2);
            *(uint2*)(grow + 32 * d + 8 * g + 4 * hh) = pk;
        }
}

// fp32 (parity mode): vector-ALU kernels, sequential FMA chains.  One kernel serves both sweeps: 32 "own" rows per workgroup
// (queries for dQ, keys for dK / dV), eight threads per own row; each takes every eighth row of the "other" tile for the
// scores and a slice of the channels for the gradients.
//   KV = false: own = query i, other = key j:   dQ_i = scale2 sum_j dS_ij K_j
//   KV = true:  own = key j, other = query i:   dK_j = scale2 sum_i dS_ij Q_i, dV_j = sum_i P_ij dO_i
template <int CH, int OB, bool KV>
__global__ __launch_bounds__(256) void sattn_bwd_f32_k(const float* qkv, const float* dout, const float* lse, const float* delta,
                                                       int T, int heads, float scale2, float* dqkv) {
    constexpr int NE = OB / 8, ND = CH / 32;
    __shared__ __attribute__((aligned(16))) float As[OB * CH];       // other rows of S: K (dQ) or Q (dK / dV)
    __shared__ __attribute__((aligned(16))) float Bs[OB * CH];       // other rows of dP: V (dQ) or dO (dK / dV)
    __shared__ float Ps[32][OB + 1];
    __shared__ float Ds[32][OB + 1];
    const int tid = threadIdx.x, ol = tid >> 3, g = tid & 7;
    const int n = blockIdx.y / heads, h = blockIdx.y - n * heads;
    const int64_t RS = (int64_t)heads * 3 * CH, OS = (int64_t)heads * CH;
    const float* base = qkv + (int64_t)n * T * RS + (int64_t)h * 3 * CH;
    const float* dob = dout + (int64_t)n * T * OS + (int64_t)h * CH;
    const float* lrow = lse + (int64_t)blockIdx.y * T;
    const float* erow = delta + (int64_t)blockIdx.y * T;
    const int oi = blockIdx.x * 32 + ol;
    const int oc = min(oi, T - 1);
    // the own row of S and of dP
    const float* arow = base + (int64_t)oc * RS + (KV ? CH : 0);
    const float* brow = KV ? base + (int64_t)oc * RS + 2 * CH : dob + (int64_t)oc * OS;
    const float lo = KV ? 0.f : lrow[oc], eo = KV ? 0.f : erow[oc];
    float4 ga[ND], gb[ND];                        // dQ or dK; dV
#pragma unroll
    for (int e = 0; e < ND; ++e) ga[e] = gb[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < T; t0 += OB) {
        __syncthreads();
        for (int c = tid; c < OB * (CH / 4); c += 256) {
            const int row = c / (CH / 4), c4 = c - row * (CH / 4);
            float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
            if (t0 + row < T) {
                const float* src = base + (int64_t)(t0 + row) * RS + 4 * c4;
                av = *(const float4*)(src + (KV ? 0 : CH));
                bv = KV ? *(const float4*)(dob + (int64_t)(t0 + row) * OS + 4 * c4) : *(const float4*)(src + 2 * CH);
            }
            *(float4*)(As + row * CH + 4 * c4) = av;
            *(float4*)(Bs + row * CH + 4 * c4) = bv;
        }
        __syncthreads();
        float s[NE], dp[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) s[e] = dp[e] = 0.f;
#pragma unroll 2                                  // a full unroll hoists the own rows out of the tile loop and spills
        for (int c = 0; c < CH; c += 4) {
            const float4 a = *(const float4*)(arow + c), b = *(const float4*)(brow + c);
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const float4 x = *(const float4*)(As + (g + 8 * e) * CH + c), y = *(const float4*)(Bs + (g + 8 * e) * CH + c);
                s[e] = fmaf(a.x, x.x, s[e]);
                s[e] = fmaf(a.y, x.y, s[e]);
                s[e] = fmaf(a.z, x.z, s[e]);
                s[e] = fmaf(a.w, x.w, s[e]);
                dp[e] = fmaf(b.x, y.x, dp[e]);
                dp[e] = fmaf(b.y, y.y, dp[e]);
                dp[e] = fmaf(b.z, y.z, dp[e]);
                dp[e] = fmaf(b.w, y.w, dp[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int ti = t0 + g + 8 * e;
            const bool in = ti < T;               // padded rows of the other side: P = 0
            const float li = KV ? (in ? lrow[ti] : 0.f) : lo, ei = KV ? (in ? erow[ti] : 0.f) : eo;
            const float p = in ? expf(fmaf(s[e], scale2, -li)) : 0.f;
            Ps[ol][g + 8 * e] = p;
            Ds[ol][g + 8 * e] = p * (dp[e] - ei);
        }
        __syncthreads();
        for (int k = 0; k < OB; ++k) {
            const float ds = Ds[ol][k];
#pragma unroll
            for (int e = 0; e < ND; ++e) {
                const float4 x = *(const float4*)(As + k * CH + 4 * g + 32 * e);
                ga[e].x = fmaf(ds, x.x, ga[e].x);
                ga[e].y = fmaf(ds, x.y, ga[e].y);
                ga[e].z = fmaf(ds, x.z, ga[e].z);
                ga[e].w = fmaf(ds, x.w, ga[e].w);
            }
            if (KV) {
                const float p = Ps[ol][k];
#pragma unroll
                for (int e = 0; e < ND; ++e) {
                    const float4 y = *(const float4*)(Bs + k * CH + 4 * g + 32 * e);
                    gb[e].x = fmaf(p, y.x, gb[e].x);
                    gb[e].y = fmaf(p, y.y, gb[e].y);
                    gb[e].z = fmaf(p, y.z, gb[e].z);
                    gb[e].w = fmaf(p, y.w, gb[e].w);
                }
            }
        }
    }
    if (oi < T) {
        float* grow = dqkv + ((int64_t)n * T + oi) * RS + (int64_t)h * 3 * CH + (KV ? CH : 0);
#pragma unroll
        for (int e = 0; e < ND; ++e) {
            *(float4*)(grow + 4 * g + 32 * e) = make_float4(ga[e].x * scale2, ga[e].y * scale2, ga[e].z * scale2, ga[e].w * scale2);
            if (KV) *(float4*)(grow + CH + 4 * g + 32 * e) = gb[e];
        }
    }
}

// ONE selection per call: the launchers branch on .idx / .bwd_ok and pai_sattn_kernel_name prints .fwd / .bwd of the same struct.
struct SattnSel {
    int idx;                                      // 0 .. 3: ch 32, 64, 128, 256; -1: no kernel
    bool bwd_ok;
    const char* fwd;
    const char* bwd;
};

static SattnSel sattn_select(int dtype, int ch) {
    static const char* const fwd_bf[4] = {"sattn_bf16_k<32>", "sattn_bf16_k<64>", "sattn_bf16_k<128>", "sattn_bf16_k<256>"};
    static const char* const fwd_f[4] = {"sattn_f32_k<32, 32>", "sattn_f32_k<64, 32>", "sattn_f32_k<128, 32>", "sattn_f32_k<256, 16>"};
    static const char* const bwd_bf[3] = {
        "sattn_bwd_delta_k<unsigned short, 32>+sattn_bwd_kv_bf16_k<32>+sattn_bwd_q_bf16_k<32>",
        "sattn_bwd_delta_k<unsigned short, 64>+sattn_bwd_kv_bf16_k<64>+sattn_bwd_q_bf16_k<64>",
        "sattn_bwd_delta_k<unsigned short, 128>+sattn_bwd_kv_bf16_k<128>+sattn_bwd_q_bf16_k<128>"};
    static const char* const bwd_f[4] = {
        "sattn_bwd_delta_k<float, 32>+sattn_bwd_f32_k<32, 32, true>+sattn_bwd_f32_k<32, 32, false>",
        "sattn_bwd_delta_k<float, 64>+sattn_bwd_f32_k<64, 32, true>+sattn_bwd_f32_k<64, 32, false>",
        "sattn_bwd_delta_k<float, 128>+sattn_bwd_f32_k<128, 32, true>+sattn_bwd_f32_k<128, 32, false>",
        "sattn_bwd_delta_k<float, 256>+sattn_bwd_f32_k<256, 16, true>+sattn_bwd_f32_k<256, 16, false>"};
    const int idx = ch == 32 ? 0 : ch == 64 ? 1 : ch == 128 ? 2 : ch == 256 ? 3 : -1;
    if (idx < 0) return {-1, false, "", ""};
    if (dtype == PAI_BF16) return {idx, idx < 3, fwd_bf[idx], idx < 3 ? bwd_bf[idx] : ""};
    return {idx, true, fwd_f[idx], bwd_f[idx]};
}

static int sattn_check(const char* who, int dtype, int N, int T, int heads, int ch) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "%s: dtype=%d", who, dtype);
    PAI_CHECK(N >= 1 && T >= 1 && heads >= 1, "%s: N=%d T=%d heads=%d", who, N, T, heads);
    PAI_CHECK(sattn_select(dtype, ch).idx >= 0, "%s: ch=%d (32, 64, 128 or 256 channels per head)", who, ch);
    PAI_CHECK((int64_t)N * heads <= 65535, "%s: N * heads = %lld (at most 65535)", who, (long long)N * heads);
    return 0;
}

static int sattn_forward(const char* who, int dtype, const void* qkv, int N, int T, int heads, int ch, void* out, float* lse,
                         void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "%s: dtype=%d", who, dtype);
    PAI_CHECK(qkv && out, "%s: null tensor", who);
    if (sattn_check(who, dtype, N, T, heads, ch)) return 1;
    PAI_CHECK((((uintptr_t)qkv) | ((uintptr_t)out)) % 16 == 0, "%s: tensors must be 16-byte aligned", who);
    const SattnSel sel = sattn_select(dtype, ch);
    hipStream_t s = (hipStream_t)stream;
    const float scale2 = 1.0f / sqrtf((float)ch);           // (ch ** -0.25) ** 2
    if (dtype == PAI_BF16) {
        const dim3 grid(cdiv(T, 128), N * heads);
#define PAI_SATTN_BF16(CH) \
    PAI_LAUNCH((sattn_bf16_k<CH>), grid, dim3(256), 0, s, (const bf16_t*)qkv, T, heads, scale2, (bf16_t*)out, lse)
        switch (sel.idx) {
            case 0: PAI_SATTN_BF16(32); break;
            case 1: PAI_SATTN_BF16(64); break;
            case 2: PAI_SATTN_BF16(128); break;
            default: PAI_SATTN_BF16(256); break;
        }
#undef PAI_SATTN_BF16
    } else {
        const dim3 grid(cdiv(T, 32), N * heads);
#define PAI_SATTN_F32(CH, KVB) \
    PAI_LAUNCH((sattn_f32_k<CH, KVB>), grid, dim3(256), 0, s, (const float*)qkv, T, heads, scale2, (float*)out, lse)
        switch (sel.idx) {
            case 0: PAI_SATTN_F32(32, 32); break;
            case 1: PAI_SATTN_F32(64, 32); break;
            case 2: PAI_SATTN_F32(128, 32); break;
            default: PAI_SATTN_F32(256, 16); break;
        }
#undef PAI_SATTN_F32
    }
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_sattn_fwd(int dtype, const void* qkv, int N, int T, int heads, int ch, void* out, void* stream) {
    return sattn_forward("pai_sattn_fwd", dtype, qkv, N, T, heads, ch, out, nullptr, stream);
}

extern "C" int pai_sattn_fwd_lse(int dtype, const void* qkv, int N, int T, int heads, int ch, void* out, float* lse,
                                 void* stream) {
    PAI_CHECK(lse, "pai_sattn_fwd_lse: null tensor");
    return sattn_forward("pai_sattn_fwd_lse", dtype, qkv, N, T, heads, ch, out, lse, stream);
}

extern "C" int pai_sattn_bwd(int dtype, const void* dout, const void* qkv, const void* out, const float* lse, int N, int T,
                             int heads, int ch, void* dqkv, float* ws, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "pai_sattn_bwd: dtype=%d", dtype);
    PAI_CHECK(dout && qkv && out && lse && dqkv && ws, "pai_sattn_bwd: null tensor");
    if (sattn_check("pai_sattn_bwd", dtype, N, T, heads, ch)) return 1;
    const SattnSel sel = sattn_select(dtype, ch);
    PAI_CHECK(sel.bwd_ok, "pai_sattn_bwd: ch=256 has no bf16 backward (bf16: 32, 64 or 128 channels per head; fp32 also 256)");
    PAI_CHECK((((uintptr_t)dout) | ((uintptr_t)qkv) | ((uintptr_t)out) | ((uintptr_t)lse) | ((uintptr_t)dqkv) | ((uintptr_t)ws)) % 16 == 0,
              "pai_sattn_bwd: tensors must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const float scale2 = 1.0f / sqrtf((float)ch);
    const int64_t rows = (int64_t)N * T * heads;
    PAI_CHECK(rows * (ch / 8) < ((int64_t)1 << 31) * 256, "pai_sattn_bwd: too many rows");
    const dim3 dgrid(cdiv(rows * (ch / 8), 256));
    if (dtype == PAI_BF16) {
        const dim3 grid(cdiv(T, 128), N * heads);
#define PAI_SATTN_BWD_BF16(CH)                                                                                                 \
    PAI_LAUNCH((sattn_bwd_delta_k<bf16_t, CH>), dgrid, dim3(256), 0, s, (const bf16_t*)dout, (const bf16_t*)out, rows, \
                       T, heads, ws);                                                                                          \
    PAI_LAUNCH((sattn_bwd_kv_bf16_k<CH>), grid, dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dout, lse,         \
                       (const float*)ws, T, heads, scale2, (bf16_t*)dqkv);                                                     \
    PAI_LAUNCH((sattn_bwd_q_bf16_k<CH>), grid, dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)dout, lse,          \
                       (const float*)ws, T, heads, scale2, (bf16_t*)dqkv)
        switch (sel.idx) {
            case 0: PAI_SATTN_BWD_BF16(32); break;
            case 1: PAI_SATTN_BWD_BF16(64); break;
            default: PAI_SATTN_BWD_BF16(128); break;
        }
#undef PAI_SATTN_BWD_BF16
    } else {
        const dim3 grid(cdiv(T, 32), N * heads);
#define PAI_SATTN_BWD_F32(CH, OB)                                                                                           \
    PAI_LAUNCH((sattn_bwd_delta_k<float, CH>), dgrid, dim3(256), 0, s, (const float*)dout, (const float*)out, rows, \
                       T, heads, ws);                                                                                       \
    PAI_LAUNCH((sattn_bwd_f32_k<CH, OB, true>), grid, dim3(256), 0, s, (const float*)qkv, (const float*)dout, lse,  \
                       (const float*)ws, T, heads, scale2, (float*)dqkv);                                                   \
    PAI_LAUNCH((sattn_bwd_f32_k<CH, OB, false>), grid, dim3(256), 0, s, (const float*)qkv, (const float*)dout, lse, \
                       (const float*)ws, T, heads, scale2, (float*)dqkv)
        switch (sel.idx) {
            case 0: PAI_SATTN_BWD_F32(32, 32); break;
            case 1: PAI_SATTN_BWD_F32(64, 32); break;
            case 2: PAI_SATTN_BWD_F32(128, 32); break;
            default: PAI_SATTN_BWD_F32(256, 16); break;
        }
#undef PAI_SATTN_BWD_F32
    }
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_sattn_kernel_name(int dtype, int ch, int op, char* name, int name_len) {
    PAI_CHECK(name && name_len > 0, "pai_sattn_kernel_name: bad arguments");
    PAI_CHECK(op == 0 || op == 1, "pai_sattn_kernel_name: op %d (0 forward, 1 backward)", op);
    if (sattn_check("pai_sattn_kernel_name", dtype, 1, 1, 1, ch)) return 1;
    const SattnSel sel = sattn_select(dtype, ch);
    PAI_CHECK(op == 0 || sel.bwd_ok,
              "pai_sattn_kernel_name: ch=256 has no bf16 backward (bf16: 32, 64 or 128 channels per head; fp32 also 256)");
    snprintf(name, (size_t)name_len, "%s", op == 0 ? sel.fwd : sel.bwd);
    return 0;
}

// ---- out = act(x * A + B) -----------------------------------------------------------------------------------------------------
// [N][rows][C], C = 8 G.  A workgroup covers 256 / G rows at a time; a thread keeps its channel group, so the coefficients
// (per channel or per sample and channel) are loaded once, and has SV vectors in flight.
constexpr int AV = 4;

template <bool EXACT> __device__ __forceinline__ float silu_f(float v) {
    return EXACT ? v / (1.0f + expf(-v)) : v / (1.0f + __expf(-v));
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void affine_act_k(const T* x, int64_t rows, int G, int R, const float* A, const float* B,
                                                    int per_sample, T* out) {
    const int cg = threadIdx.x % G, rr = threadIdx.x / G;
    if (rr >= R) return;
    const int C = G * 8, n = blockIdx.y;
    const float* ap = A + (per_sample ? (int64_t)n * C : 0) + cg * 8;
    const float* bp = B + (per_sample ? (int64_t)n * C : 0) + cg * 8;
    float a[8], b[8];
    V8<float>::ld(ap, a);
    V8<float>::ld(bp, b);
    const T* xs = x + (int64_t)n * rows * C + cg * 8;
    T* os = out + (int64_t)n * rows * C + cg * 8;
    const int64_t step = (int64_t)gridDim.x * R * AV;
    for (int64_t r0 = (int64_t)blockIdx.x * R * AV + rr; r0 < rows; r0 += step) {
        float v[AV][8];
#pragma unroll
        for (int k = 0; k < AV; ++k)
            if (r0 + (int64_t)k * R < rows) V8<T>::ld(xs + (r0 + (int64_t)k * R) * C, v[k]);
#pragma unroll
        for (int k = 0; k < AV; ++k)
            if (r0 + (int64_t)k * R < rows) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float t = fmaf(v[k][e], a[e], b[e]);
                    v[k][e] = ACT == PAI_ACT_SILU ? silu_f<sizeof(T) == 4>(t) : t;
                }
                V8<T>::st(os + (r0 + (int64_t)k * R) * C, v[k]);
            }
    }
}

extern "C" int pai_affine_act(int dtype, const void* x, int64_t rows_per_sample, int N, int C, const float* A, const float* B,
                              int per_sample, int act, void* out, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "pai_affine_act: dtype=%d", dtype);
    PAI_CHECK(x && out && A && B, "pai_affine_act: null tensor");
    PAI_CHECK(act == PAI_ACT_NONE || act == PAI_ACT_SILU, "pai_affine_act: act=%d (none or SiLU)", act);
    PAI_CHECK(N >= 1 && N <= 65535 && rows_per_sample >= 1, "pai_affine_act: N=%d rows=%lld", N, (long long)rows_per_sample);
    PAI_CHECK(C >= 8 && C % 8 == 0 && C <= 2048, "pai_affine_act: C=%d (a multiple of 8, at most 2048)", C);
    const int G = C / 8, R = 256 / G;
    const dim3 grid((unsigned)min((int64_t)4096, (rows_per_sample + (int64_t)R * AV - 1) / ((int64_t)R * AV)), N);
    hipStream_t s = (hipStream_t)stream;
#define PAI_AFF(TT, ACT) \
    PAI_LAUNCH((affine_act_k<TT, ACT>), grid, dim3(256), 0, s, (const TT*)x, rows_per_sample, G, R, A, B, per_sample, (TT*)out)
    if (dtype == PAI_F32) {
        if (act == PAI_ACT_SILU) PAI_AFF(float, PAI_ACT_SILU); else PAI_AFF(float, PAI_ACT_NONE);
    } else {
        if (act == PAI_ACT_SILU) PAI_AFF(bf16_t, PAI_ACT_SILU); else PAI_AFF(bf16_t, PAI_ACT_NONE);
    }
#undef PAI_AFF
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- FiLM coefficients ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void film_coeffs_k(int C, int N, const float* a, const float* b, const T* emb, int64_t ld,
                                                     float* A, float* B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * C) return;
    const int n = i / C, c = i - n * C;
    const float sc = 1.0f + Conv<T>::ld(emb + n * ld + c), sh = Conv<T>::ld(emb + n * ld + C + c);
    A[i] = a[c] * sc;
    B[i] = fmaf(b[c], sc, sh);
}

extern "C" int pai_film_coeffs(int dtype, int C, int N, const float* a, const float* b, const void* emb_out, int64_t ld,
                               float* A, float* B, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "pai_film_coeffs: dtype=%d", dtype);
    PAI_CHECK(a && b && emb_out && A && B, "pai_film_coeffs: null tensor");
    PAI_CHECK(C >= 1 && N >= 1 && ld >= 2 * (int64_t)C && (int64_t)N * C < (1ll << 31), "pai_film_coeffs: C=%d N=%d ld=%lld", C, N,
              (long long)ld);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAI_F32)
        PAI_LAUNCH(film_coeffs_k<float>, dim3(cdiv((int64_t)N * C, 256)), dim3(256), 0, s, C, N, a, b, (const float*)emb_out, ld, A, B);
    else
        PAI_LAUNCH(film_coeffs_k<bf16_t>, dim3(cdiv((int64_t)N * C, 256)), dim3(256), 0, s, C, N, a, b, (const bf16_t*)emb_out, ld, A, B);
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- 2 x 2 mean ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_k(const T* x, int64_t nvec, int OH, int OW, int G, T* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const int cg = (int)(i % G);
    int64_t p = i / G;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const int64_t n = p / OH;
    const int C = G * 8, W = 2 * OW;
    const T* s = x + (((n * 2 * OH + 2 * oy) * W + 2 * ox) * (int64_t)C) + cg * 8;
    float a[8], b[8], c[8], d[8];
    V8<T>::ld(s, a);
    V8<T>::ld(s + C, b);
    V8<T>::ld(s + (int64_t)W * C, c);
    V8<T>::ld(s + (int64_t)W * C + C, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = ((a[e] + b[e]) + (c[e] + d[e])) * 0.25f;
    V8<T>::st(out + i * 8, a);
}

extern "C" int pai_avgpool2(int dtype, const void* x, int N, int H, int W, int C, void* out, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "pai_avgpool2: dtype=%d", dtype);
    PAI_CHECK(x && out, "pai_avgpool2: null tensor");
    PAI_CHECK(N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "pai_avgpool2: N=%d H=%d W=%d (even sizes)", N, H, W);
    PAI_CHECK(C >= 8 && C % 8 == 0, "pai_avgpool2: C=%d (a multiple of 8)", C);
    const int64_t nvec = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
    PAI_CHECK((nvec + 255) / 256 < (1ll << 31), "pai_avgpool2: tensor too large");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((nvec + 255) / 256));
    if (dtype == PAI_F32)
        PAI_LAUNCH(avgpool2_k<float>, grid, dim3(256), 0, s, (const float*)x, nvec, H / 2, W / 2, C / 8, (float*)out);
    else
        PAI_LAUNCH(avgpool2_k<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, nvec, H / 2, W / 2, C / 8, (bf16_t*)out);
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- backward of the 2 x 2 mean --------------------------------------------------------------------------------------------------------
// The geometry of avgpool2_k: a thread owns one 16-byte channel vector of dout and stores it, times 0.25, to the four
// positions of dx it was averaged from.  Every element of dx is written exactly once.
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_bwd_k(const T* dout, int64_t nvec, int OH, int OW, int G, T* dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const int cg = (int)(i % G);
    int64_t p = i / G;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const int64_t n = p / OH;
    const int C = G * 8, W = 2 * OW;
    float v[8];
    V8<T>::ld(dout + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= 0.25f;
    T* d = dx + (((n * 2 * OH + 2 * oy) * W + 2 * ox) * (int64_t)C) + cg * 8;
    V8<T>::st(d, v);
    V8<T>::st(d + C, v);
    V8<T>::st(d + (int64_t)W * C, v);
    V8<T>::st(d + (int64_t)W * C + C, v);
}

extern "C" int pai_avgpool2_bwd(int dtype, const void* dout, int N, int H, int W, int C, void* dx, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "pai_avgpool2_bwd: dtype=%d", dtype);
    PAI_CHECK(dout && dx, "pai_avgpool2_bwd: null tensor");
    PAI_CHECK(((uintptr_t)dout & 15) == 0 && ((uintptr_t)dx & 15) == 0, "pai_avgpool2_bwd: tensors must be 16-byte aligned");
    PAI_CHECK(N >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "pai_avgpool2_bwd: N=%d H=%d W=%d (even sizes)", N, H, W);
    PAI_CHECK(C >= 8 && C % 8 == 0, "pai_avgpool2_bwd: C=%d (a multiple of 8)", C);
    const int64_t nvec = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
    PAI_CHECK((nvec + 255) / 256 < (1ll << 31), "pai_avgpool2_bwd: tensor too large");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((nvec + 255) / 256));
    if (dtype == PAI_F32)
        PAI_LAUNCH(avgpool2_bwd_k<float>, grid, dim3(256), 0, s, (const float*)dout, nvec, H / 2, W / 2, C / 8, (float*)dx);
    else
        PAI_LAUNCH(avgpool2_bwd_k<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)dout, nvec, H / 2, W / 2, C / 8, (bf16_t*)dx);
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- du = g SiLU'(u) -------------------------------------------------------------------------------------------------------------------
// SiLU'(u) = sig (1 + u (1 - sig)) with sig and 1 - sig from fn_sig, as film_norm.hip forms it.  A thread owns eight
// consecutive elements: one 16-byte vector per tensor where all eight exist, element by element in the ragged tail.  It
// reads its elements of g before it writes them to du, so du may alias g.
template <typename T>
__global__ __launch_bounds__(256) void silu_bwd_k(const T* g, const T* u, int64_t numel, T* du) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= numel) return;
    constexpr bool EXACT = sizeof(T) == 4;
    if (i0 + 8 <= numel) {
        float gv[8], uv[8];
        V8<T>::ld(g + i0, gv);
        V8<T>::ld(u + i0, uv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float sig, oms;
            fn_sig<EXACT>(uv[e], sig, oms);
            gv[e] *= sig * fmaf(uv[e], oms, 1.f);
        }
        V8<T>::st(du + i0, gv);
    } else {
        for (int64_t i = i0; i < numel; ++i) {
            const float uu = Conv<T>::ld(u + i);
            float sig, oms;
            fn_sig<EXACT>(uu, sig, oms);
            Conv<T>::st(du + i, Conv<T>::ld(g + i) * (sig * fmaf(uu, oms, 1.f)));
        }
    }
}

extern "C" int pai_silu_bwd(int dtype, const void* g, const void* u, int64_t numel, void* du, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "pai_silu_bwd: dtype=%d", dtype);
    PAI_CHECK(g && u && du, "pai_silu_bwd: null tensor");
    PAI_CHECK(((uintptr_t)g & 15) == 0 && ((uintptr_t)u & 15) == 0 && ((uintptr_t)du & 15) == 0,
              "pai_silu_bwd: tensors must be 16-byte aligned");
    PAI_CHECK(numel >= 1, "pai_silu_bwd: numel=%lld", (long long)numel);
    const int64_t nthr = (numel + 7) / 8;
    PAI_CHECK((nthr + 255) / 256 < (1ll << 31), "pai_silu_bwd: tensor too large");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((nthr + 255) / 256));
    if (dtype == PAI_F32)
        PAI_LAUNCH(silu_bwd_k<float>, grid, dim3(256), 0, s, (const float*)g, (const float*)u, numel, (float*)du);
    else
        PAI_LAUNCH(silu_bwd_k<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)g, (const bf16_t*)u, numel, (bf16_t*)du);
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- sinusoidal embedding of the noise level ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gamma_embedding_k(const float* gammas, int N, int dim, T* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * dim) return;
    const int n = i / dim, j = i - n * dim, half = dim / 2;
    float v = 0.f;                                // the last column of an odd dim
    if (j < 2 * half) {
        const int k = j < half ? j : j - half;
        const double arg = (double)gammas[n] * exp(-9.210340371976184 /* ln 10000 */ * (double)k / (double)half);
        v = (float)(j < half ? cos(arg) : sin(arg));
    }
    Conv<T>::st(out + i, v);
}

extern "C" int pai_gamma_embedding(int dtype, const float* gammas, int N, int dim, void* out, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "pai_gamma_embedding: dtype=%d", dtype);
    PAI_CHECK(gammas && out, "pai_gamma_embedding: null tensor");
    PAI_CHECK(N >= 1 && dim >= 2 && (int64_t)N * dim < (1ll << 31), "pai_gamma_embedding: N=%d dim=%d", N, dim);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PAI_F32)
        PAI_LAUNCH(gamma_embedding_k<float>, dim3(cdiv((int64_t)N * dim, 256)), dim3(256), 0, s, gammas, N, dim, (float*)out);
    else
        PAI_LAUNCH(gamma_embedding_k<bf16_t>, dim3(cdiv((int64_t)N * dim, 256)), dim3(256), 0, s, gammas, N, dim, (bf16_t*)out);
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- one reverse step ------------------------------------------------------------------------------------------------------------------
// y0 = clamp((y_t - s1 eps) rs, -1, 1); mean = c0 y0 + c1 y_t; log variance = v log_hi + (1 - v) log_lo with v = (var + 1) / 2
// (learn_var) or log_lo; y_{t-1} = mean + exp(0.5 log variance) noise (add_noise) -- the expression order of
// palette.py:233-306.  Pixels are [pixel][channel]; the model output has C (or, learn_var, 2 C: eps | var) columns.
// RNG: the noise of element i is normal i of the Philox tuple `key` (stream 3, sub = the draw index), not noise[i].
// One body for the four kernels below: the by-value forms and the device-state forms differ only in where (i, the six scalars,
// the noise) come from, so for equal values they give equal bits.
template <typename T, bool RNG>
__device__ __forceinline__ void palette_step_body(const T* mo, const float* y_t, const float* noise, const PhiloxKey& key,
                                                  int64_t numel, int C, int learn_var, int add_noise, float s1, float rs, float c0,
                                                  float c1, float log_lo, float log_hi, float* y_next, T* xy_next) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= numel) return;
    const int64_t px = i / C;
    const int c = (int)(i - px * C);
    const int Cm = learn_var ? 2 * C : C;
    const float eps = Conv<T>::ld(mo + px * Cm + c), y = y_t[i];
    // one rounding for y_t - s1 eps: rs reaches 800 at the first step, and a rounded product would cost 1e-4 of y0 there
    float y0 = rs * fmaf(-s1, eps, y);
    y0 = fminf(fmaxf(y0, -1.f), 1.f);
    const float mean = c0 * y0 + c1 * y;
    float lv = log_lo;
    if (learn_var) {
        const float vi = (Conv<T>::ld(mo + px * Cm + C + c) + 1.f) * 0.5f;
        lv = vi * log_hi + (1.f - vi) * log_lo;
    }
    float z = 0.f;
    if (add_noise) z = RNG ? philox_normal_at(key, i) : noise[i];
    const float out = add_noise ? mean + expf(0.5f * lv) * z : mean;
    y_next[i] = out;
    if (xy_next) Conv<T>::st(xy_next + px * 2 * C + C + c, out);
}

template <typename T, bool RNG>
__global__ __launch_bounds__(256) void palette_step_k(const T* mo, const float* y_t, const float* noise, PhiloxKey key, int64_t numel,
                                                      int C, int learn_var, int add_noise, float s1, float rs, float c0, float c1,
                                                      float log_lo, float log_hi, float* y_next, T* xy_next) {
    palette_step_body<T, RNG>(mo, y_t, noise, key, numel, C, learn_var, add_noise, s1, rs, c0, c1, log_lo, log_hi, y_next, xy_next);
}

// The step whose index lives on the device (a recorded launch stands for every step of the chain): k = *pos clamped into [1, T]
// is the 1-based index of the reverse step, i = T - k its row of `table` (fp32 [T][6], the scalars of palette_step_k in its
// argument order), add_noise = i > 1, the noise row k of noise_stack [T + 1][numel] or (RNG) Philox at sub = k, step = *rng_step.
// The first workgroup also writes gamma_next[0 .. N) = gammas[max(i - 1, 0)], the noise level the NEXT U-Net pass embeds.
// pos and rng_step are only read: every workgroup reads them, and the launch that advances pos comes behind this one.
template <typename T, bool RNG>
__global__ __launch_bounds__(256) void palette_step_dev_k(const T* mo, const float* y_t, const float* noise_stack, PhiloxKey key,
                                                          const uint32_t* rng_step, int64_t numel, int C, int learn_var,
                                                          const float* table, int Tn, const uint32_t* pos, const float* gammas,
                                                          int N, float* gamma_next, float* y_next, T* xy_next) {
    uint32_t k = *pos;
    k = k < 1u ? 1u : (k > (uint32_t)Tn ? (uint32_t)Tn : k);
    const int i = Tn - (int)k;
    if (blockIdx.x == 0) {
        const float g = gammas[i > 0 ? i - 1 : 0];
        for (int n = threadIdx.x; n < N; n += 256) gamma_next[n] = g;
    }
    const float* row = table + 6 * i;
    const float* noise = nullptr;
    if (RNG) {
        key.sub = k;
        key.step = *rng_step;
    } else {
        noise = noise_stack + (int64_t)k * numel;
    }
    palette_step_body<T, RNG>(mo, y_t, noise, key, numel, C, learn_var, i > 1 ? 1 : 0, row[0], row[1], row[2], row[3], row[4], row[5],
                              y_next, xy_next);
}

template <bool RNG>
static int palette_step_launch(const char* who, int dtype, const void* model_out, const float* y_t, const float* noise, PhiloxKey key,
                               int64_t pixels, int C, int learn_var, int add_noise, float s1, float rs, float c0, float c1,
                               float log_lo, float log_hi, float* y_next, void* xy_next, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "%s: dtype=%d", who, dtype);
    PAI_CHECK(model_out && y_t && y_next && (RNG || noise || !add_noise), "%s: null tensor", who);
    PAI_CHECK(pixels >= 1 && C >= 1, "%s: pixels=%lld C=%d", who, (long long)pixels, C);
    PAI_CHECK(!RNG || pixels <= (1ll << 34) / C, "%s: tensor too large (more than 2^32 blocks of 4)", who);
    const int64_t numel = pixels * C;
    PAI_CHECK((numel + 255) / 256 < (1ll << 31), "%s: tensor too large", who);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((numel + 255) / 256));
    if (dtype == PAI_F32)
        PAI_LAUNCH((palette_step_k<float, RNG>), grid, dim3(256), 0, s, (const float*)model_out, y_t, noise, key, numel, C,
                           learn_var, add_noise, s1, rs, c0, c1, log_lo, log_hi, y_next, (float*)xy_next);
    else
        PAI_LAUNCH((palette_step_k<bf16_t, RNG>), grid, dim3(256), 0, s, (const bf16_t*)model_out, y_t, noise, key, numel, C,
                           learn_var, add_noise, s1, rs, c0, c1, log_lo, log_hi, y_next, (bf16_t*)xy_next);
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_palette_step(int dtype, const void* model_out, const float* y_t, const float* noise, int64_t pixels, int C,
                                int learn_var, int add_noise, float s1, float rs, float c0, float c1, float log_lo, float log_hi,
                                float* y_next, void* xy_next, void* stream) {
    return palette_step_launch<false>("pai_palette_step", dtype, model_out, y_t, noise, PhiloxKey{}, pixels, C, learn_var, add_noise,
                                      s1, rs, c0, c1, log_lo, log_hi, y_next, xy_next, stream);
}

extern "C" int pai_palette_step_rng(int dtype, const void* model_out, const float* y_t, int64_t pixels, int C, int learn_var,
                                    int add_noise, float s1, float rs, float c0, float c1, float log_lo, float log_hi,
                                    uint64_t seed, uint32_t sub, uint32_t step, float* y_next, void* xy_next, void* stream_handle) {
    return palette_step_launch<true>("pai_palette_step_rng", dtype, model_out, y_t, nullptr,
                                     philox_key(seed, sub, PHILOX_STREAM_SAMPLER, step), pixels, C, learn_var, add_noise, s1, rs, c0,
                                     c1, log_lo, log_hi, y_next, xy_next, stream_handle);
}

template <bool RNG>
static int palette_step_dev_launch(const char* who, int dtype, const void* model_out, const float* y_t, const float* noise_stack,
                                   PhiloxKey key, const uint32_t* rng_step, int64_t pixels, int C, int learn_var, const float* table,
                                   int T, const uint32_t* pos, const float* gammas, int N, float* gamma_next, float* y_next,
                                   void* xy_next, void* stream) {
    PAI_CHECK(dtype == PAI_F32 || dtype == PAI_BF16, "%s: dtype=%d", who, dtype);
    PAI_CHECK(model_out && y_t && y_next && table && pos && gammas && gamma_next && (RNG ? rng_step != nullptr : noise_stack != nullptr),
              "%s: null tensor", who);
    PAI_CHECK(pixels >= 1 && C >= 1, "%s: pixels=%lld C=%d", who, (long long)pixels, C);
    PAI_CHECK(T >= 1 && N >= 1, "%s: T=%d N=%d", who, T, N);
    PAI_CHECK(!RNG || pixels <= (1ll << 34) / C, "%s: tensor too large (more than 2^32 blocks of 4)", who);
    PAI_CHECK(pixels <= (1ll << 62) / C / ((int64_t)T + 1), "%s: tensor too large", who);
    const int64_t numel = pixels * C;
    PAI_CHECK((numel + 255) / 256 < (1ll << 31), "%s: tensor too large", who);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((numel + 255) / 256));
    if (dtype == PAI_F32)
        PAI_LAUNCH((palette_step_dev_k<float, RNG>), grid, dim3(256), 0, s, (const float*)model_out, y_t, noise_stack, key, rng_step,
                   numel, C, learn_var, table, T, pos, gammas, N, gamma_next, y_next, (float*)xy_next);
    else
        PAI_LAUNCH((palette_step_dev_k<bf16_t, RNG>), grid, dim3(256), 0, s, (const bf16_t*)model_out, y_t, noise_stack, key, rng_step,
                   numel, C, learn_var, table, T, pos, gammas, N, gamma_next, y_next, (bf16_t*)xy_next);
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_palette_step_dev(int dtype, const void* model_out, const float* y_t, const float* noise_stack, int64_t pixels,
                                    int C, int learn_var, const float* table, int T, const uint32_t* pos, const float* gammas, int N,
                                    float* gamma_next, float* y_next, void* xy_next, void* stream) {
    return palette_step_dev_launch<false>("pai_palette_step_dev", dtype, model_out, y_t, noise_stack, PhiloxKey{}, nullptr, pixels, C,
                                          learn_var, table, T, pos, gammas, N, gamma_next, y_next, xy_next, stream);
}

extern "C" int pai_palette_step_rng_dev(int dtype, const void* model_out, const float* y_t, int64_t pixels, int C, int learn_var,
                                        const float* table, int T, const uint32_t* pos, const float* gammas, int N,
                                        float* gamma_next, uint64_t seed, const uint32_t* rng_step, float* y_next, void* xy_next,
                                        void* stream_handle) {
    return palette_step_dev_launch<true>("pai_palette_step_rng_dev", dtype, model_out, y_t, nullptr,
                                         philox_key(seed, 0, PHILOX_STREAM_SAMPLER, 0), rng_step, pixels, C, learn_var, table, T, pos,
                                         gammas, N, gamma_next, y_next, xy_next, stream_handle);
}

// ---- forward noising q(y_t | y_0) ----------------------------------------------------------------------------------------------------
// gamma = (gammas[t] - gammas_prev[t]) u + gammas_prev[t], noise = z (t > 0), y_t = sqrt(gamma) y0 + sqrt(1 - gamma) noise
// (palette.py:214-231).  Grid (chunks, N): sample n reads its t, clamped into the table, once.  VEC: 4 | P C, a thread owns one
// 16-byte vector of each tensor; otherwise one element.  The thread (0, 0) of a sample writes gamma[n].
// RNG: t[n], u[n] and z are drawn here (philox.h: integer n of stream 0, uniform n of stream 1, the normals of stream 2 over the
// flat [N][P][C] tensor); every workgroup of sample n recomputes t and u, the thread (0, 0) of the sample writes t[n].
template <bool VEC, bool RNG>
__global__ __launch_bounds__(256) void palette_noise_k(const float* y0, const float* z, const float* u, const int* t, PhiloxKey key,
                                                       int* t_out, const float* gammas, const float* gammas_prev, int T, int64_t PC,
                                                       float* y_t, float* noise, float* gamma) {
    const int n = blockIdx.y;
    int tn;
    float un;
    if (RNG) {
        PhiloxKey kt = key, ku = key;
        kt.stream = PHILOX_STREAM_T;
        ku.stream = PHILOX_STREAM_U;
        const PhiloxBlock bt = philox_block(kt, (uint32_t)n >> 2), bu = philox_block(ku, (uint32_t)n >> 2);
        const int l = n & 3;
        tn = philox_int(l == 0 ? bt.w[0] : l == 1 ? bt.w[1] : l == 2 ? bt.w[2] : bt.w[3], (uint32_t)T);
        un = philox_uniform(l == 0 ? bu.w[0] : l == 1 ? bu.w[1] : l == 2 ? bu.w[2] : bu.w[3]);
    } else {
        tn = t[n];
        un = u[n];
    }
    const int tc = min(max(tn, 0), T - 1);
    const float gp = gammas_prev[tc];
    const float g = fmaf(gammas[tc] - gp, un, gp);
    const float keep = tc > 0 ? 1.f : 0.f;             // the product z * 0 keeps the sign of z, as torch's z * (t > 0)
    const float sg = sqrtf(g), s1 = sqrtf(1.f - g);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        gamma[n] = g;
        if (RNG) t_out[n] = tn;
    }
    const int64_t base = (int64_t)n * PC;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= PC) return;
    if (VEC) {
        const float4 a = *(const float4*)(y0 + base + i);
        float4 b;
        if (RNG) {
            float zz[4];
            philox_normal4(philox_block(key, (uint32_t)((base + i) >> 2)), zz);       // 4 | P C: base + i is a multiple of 4
            b = make_float4(zz[0], zz[1], zz[2], zz[3]);
        } else {
            b = *(const float4*)(z + base + i);
        }
        float4 e, y;
        e.x = b.x * keep, e.y = b.y * keep, e.z = b.z * keep, e.w = b.w * keep;
        y.x = fmaf(sg, a.x, s1 * e.x), y.y = fmaf(sg, a.y, s1 * e.y), y.z = fmaf(sg, a.z, s1 * e.z), y.w = fmaf(sg, a.w, s1 * e.w);
        *(float4*)(noise + base + i) = e;
        *(float4*)(y_t + base + i) = y;
    } else {
        const float e = (RNG ? philox_normal_at(key, base + i) : z[base + i]) * keep;
        noise[base + i] = e;
        y_t[base + i] = fmaf(sg, y0[base + i], s1 * e);
    }
}

#define PAI_ALIGNED16(p) (((uintptr_t)(p) & 15) == 0)

template <bool RNG>
static int palette_noise_launch(const char* who, const float* y0, const float* z, const float* u, const int32_t* t, PhiloxKey key,
                                int32_t* t_out, const float* gammas, const float* gammas_prev, int T, int N, int64_t P, int C,
                                float* y_t, float* noise, float* gamma, void* stream) {
    PAI_CHECK(y0 && (RNG ? t_out != nullptr : (z && u && t)) && gammas && gammas_prev && y_t && noise && gamma, "%s: null tensor", who);
    PAI_CHECK(N >= 1 && P >= 1, "%s: N=%d P=%lld", who, N, (long long)P);
    PAI_CHECK(C >= 1 && C <= 4, "%s: C=%d (1..4)", who, C);
    PAI_CHECK(T >= 1, "%s: T=%d", who, T);
    PAI_CHECK(PAI_ALIGNED16(y0) && PAI_ALIGNED16(z) && PAI_ALIGNED16(u) && PAI_ALIGNED16(t) && PAI_ALIGNED16(t_out) &&
                  PAI_ALIGNED16(gammas) && PAI_ALIGNED16(gammas_prev) && PAI_ALIGNED16(y_t) && PAI_ALIGNED16(noise) &&
                  PAI_ALIGNED16(gamma),
              "%s: tensors must be 16-byte aligned", who);
    PAI_CHECK(N <= 65535 && P <= (1ll << 40), "%s: tensor too large (N=%d P=%lld)", who, N, (long long)P);
    const int64_t PC = P * C;
    const bool vec = PC % 4 == 0;
    const int64_t chunks = ((vec ? PC / 4 : PC) + 255) / 256;
    PAI_CHECK(chunks < (1ll << 31) && PC <= (1ll << 62) / N, "%s: tensor too large", who);
    PAI_CHECK(!RNG || (PC * N + 3) / 4 <= (1ll << 32), "%s: tensor too large (more than 2^32 blocks of 4)", who);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks, (unsigned)N);
    if (vec)
        PAI_LAUNCH((palette_noise_k<true, RNG>), grid, dim3(256), 0, s, y0, z, u, t, key, t_out, gammas, gammas_prev, T, PC,
                           y_t, noise, gamma);
    else
        PAI_LAUNCH((palette_noise_k<false, RNG>), grid, dim3(256), 0, s, y0, z, u, t, key, t_out, gammas, gammas_prev, T, PC,
                           y_t, noise, gamma);
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_palette_noise(const float* y0, const float* z, const float* u, const int32_t* t, const float* gammas,
                                 const float* gammas_prev, int T, int N, int64_t P, int C, float* y_t, float* noise, float* gamma,
                                 void* stream) {
    return palette_noise_launch<false>("pai_palette_noise", y0, z, u, t, PhiloxKey{}, nullptr, gammas, gammas_prev, T, N, P, C, y_t,
                                       noise, gamma, stream);
}

extern "C" int pai_palette_noise_rng(const float* y0, const float* gammas, const float* gammas_prev, int T, int N, int64_t P, int C,
                                     uint64_t seed, uint32_t step, int32_t* t, float* y_t, float* noise, float* gamma,
                                     void* stream_handle) {
    return palette_noise_launch<true>("pai_palette_noise_rng", y0, nullptr, nullptr, nullptr, philox_key(seed, 0, PHILOX_STREAM_Z, step),
                                      t, gammas, gammas_prev, T, N, P, C, y_t, noise, gamma, stream_handle);
}

// ---- MSE + variational bound and the gradient into the U-Net output -----------------------------------------------------------
// The formulas of pai_hip.h (palette.py:254-333, 368-427).  Everything per element is fp32 with expf / logf / tanhf (the KL term
// cancels to 1e-18 at large t and exp(-plv) reaches 1e10 at t = 0: no fast intrinsics); the sums leave the thread as fp64.
struct PaletteRow {
    float s1, rs, c0, c1, log_lo, log_hi;
};

// Phi(a), the tanh approximation of the normal CDF, and phi = dPhi / da
__device__ __forceinline__ void palette_cdf(float a, float& cdf, float& pdf) {
    const float k = 0.7978845608028654f;              // sqrt(2 / pi)
    const float th = tanhf(k * (a + 0.044715f * (a * a * a)));
    const float s = 1.f - th * th;
    cdf = 0.5f * (1.f + th);
    pdf = s == 0.f ? 0.f : 0.5f * s * (k * (1.f + 3.f * 0.044715f * (a * a)));      // a saturated tanh: 0, not 0 * inf
}

// One element: returns term, and dterm / dplv in `dplv` (LV only).  nll is uniform over the workgroup.
template <bool LV>
__device__ __forceinline__ float palette_term(const PaletteRow& r, bool nll, float eps, float var, float y0, float yt, float& dplv) {
    float y0hat = r.rs * fmaf(-r.s1, eps, yt);
    y0hat = fminf(fmaxf(y0hat, -1.f), 1.f);
    const float pm = r.c0 * y0hat + r.c1 * yt;
    float plv = r.log_lo, x = 0.f;                     // x = plv - tlv = v (log_hi - log_lo), formed without the two large logs
    if (LV) {
        const float v = (var + 1.f) * 0.5f;
        plv = v * r.log_hi + (1.f - v) * r.log_lo;
        x = v * (r.log_hi - r.log_lo);
    }
    if (!nll) {
        // -1 + x + exp(-x) as x + expm1(-x): at large t x is 1e-3 and the sum of the three would keep only the rounding of 1
        const float tm = r.c0 * y0 + r.c1 * yt;
        const float d = tm - pm, em = expm1f(-x), e2 = d == 0.f ? 0.f : (d * d) * expf(-plv);
        dplv = 0.5f * (-em - e2);
        return 0.5f * ((x + em) + e2);
    }
    // 1 / stddev, kept finite: a variance output far outside [-1, 1] takes exp past the fp32 range, and inf * 0 would be a NaN
    // where exact arithmetic has a saturated CDF
    const float inv = fminf(expf(-0.5f * plv), 3e37f), cx = y0 - pm;
    const float ap = inv * (cx + 1.f / 255.f), am = inv * (cx - 1.f / 255.f);
    float cp, pp, cm, pmn;
    palette_cdf(ap, cp, pp);
    palette_cdf(am, cm, pmn);
    float q, num;                                      // L = log(max(q, 1e-12)), dL/dls = num / q where q >= 1e-12
    if (y0 < -0.999f) {
        q = cp, num = -ap * pp;
    } else if (y0 > 0.999f) {
        q = 1.f - cm, num = am * pmn;
    } else {
        q = cp - cm, num = am * pmn - ap * pp;
    }
    const bool pass = q >= 1e-12f;
    dplv = pass ? -0.5f * (num / q) : 0.f;
    return -logf(pass ? q : 1e-12f);
}

__device__ __forceinline__ PaletteRow palette_row(const float* table, const int* t, int n, int T, bool& nll) {
    const int tc = min(max(t[n], 0), T - 1);
    const float* row = table + (int64_t)tc * 6;
    nll = tc == 0;
    return PaletteRow{row[0], row[1], row[2], row[3], row[4], row[5]};
}

// The two sums of a workgroup, in a fixed order: lanes by xor shuffles, the four waves by thread 0.
__device__ __forceinline__ void palette_block_sums(float se, float tm, double* dst) {
    __shared__ double red[2][4];
    double a = (double)se, b = (double)tm;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = a, red[1][threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        dst[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        dst[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// 4 | P: a thread owns four consecutive pixels, C 16-byte vectors of each pixel tensor and Co of model_out / dout.
template <int C, bool LV>
__global__ __launch_bounds__(256) void palette_objective_vec_k(const float* mo, const float* noise, const float* y0, const float* y_t,
                                                               const int* t, const float* table, int T, int64_t P, int64_t pps,
                                                               float ge_scale, float gv_scale, float* dout, double* ws) {
    constexpr int Co = LV ? 2 * C : C;
    const int n = blockIdx.y;
    bool nll;
    const PaletteRow r = palette_row(table, t, n, T, nll);
    const float gv = gv_scale * (r.log_hi - r.log_lo);
    const int64_t p0 = (int64_t)blockIdx.x * pps, p1 = min(P, p0 + pps);
    float se = 0.f, tm = 0.f;
    for (int64_t p = p0 + threadIdx.x * 4; p < p1; p += 1024) {
        const int64_t px = (int64_t)n * P + p;
        alignas(16) float m[4 * Co], e[4 * C], a[4 * C], y[4 * C];
#pragma unroll
        for (int v = 0; v < Co; ++v) *(float4*)(m + 4 * v) = *(const float4*)(mo + px * Co + 4 * v);
#pragma unroll
        for (int v = 0; v < C; ++v) {
            *(float4*)(e + 4 * v) = *(const float4*)(noise + px * C + 4 * v);
            *(float4*)(a + 4 * v) = *(const float4*)(y0 + px * C + 4 * v);
            *(float4*)(y + 4 * v) = *(const float4*)(y_t + px * C + 4 * v);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float eps = m[k * Co + c], d = eps - e[k * C + c];
                float dplv = 0.f;
                tm += palette_term<LV>(r, nll, eps, LV ? m[k * Co + C + c] : 0.f, a[k * C + c], y[k * C + c], dplv);
                se += d * d;
                m[k * Co + c] = ge_scale * d;
                if (LV) m[k * Co + C + c] = gv * dplv;
            }
        }
#pragma unroll
        for (int v = 0; v < Co; ++v) *(float4*)(dout + px * Co + 4 * v) = *(const float4*)(m + 4 * v);
    }
    palette_block_sums(se, tm, ws + 2 * ((int64_t)n * gridDim.x + blockIdx.x));
}

// any P: a thread owns one pixel at a time
template <bool LV>
__global__ __launch_bounds__(256) void palette_objective_px_k(const float* mo, const float* noise, const float* y0, const float* y_t,
                                                              const int* t, const float* table, int T, int64_t P, int64_t pps, int C,
                                                              float ge_scale, float gv_scale, float* dout, double* ws) {
    const int Co = LV ? 2 * C : C;
    const int n = blockIdx.y;
    bool nll;
    const PaletteRow r = palette_row(table, t, n, T, nll);
    const float gv = gv_scale * (r.log_hi - r.log_lo);
    const int64_t p0 = (int64_t)blockIdx.x * pps, p1 = min(P, p0 + pps);
    float se = 0.f, tm = 0.f;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const int64_t px = (int64_t)n * P + p;
        for (int c = 0; c < C; ++c) {
            const float eps = mo[px * Co + c], d = eps - noise[px * C + c];
            float dplv = 0.f;
            tm += palette_term<LV>(r, nll, eps, LV ? mo[px * Co + C + c] : 0.f, y0[px * C + c], y_t[px * C + c], dplv);
            se += d * d;
            dout[px * Co + c] = ge_scale * d;
            if (LV) dout[px * Co + C + c] = gv * dplv;
        }
    }
    palette_block_sums(se, tm, ws + 2 * ((int64_t)n * gridDim.x + blockIdx.x));
}

// One workgroup: sample n = thread, thread + 256, ... adds its slabs in order; the samples of a thread in order; then a tree over
// the 256 threads in LDS.  out[0] = mse, out[1] = mean vlb_n, out[2] = the loss, out[3 + n] = vlb_n.
__global__ __launch_bounds__(256) void palette_objective_fin_k(const double* ws, int N, int slabs, double inv_npc, double inv_pc_ln2,
                                                               float vlb_weight, float* out) {
    __shared__ double red[2][256];
    double se = 0.0, vl = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) {
        double a = 0.0, b = 0.0;
        for (int s = 0; s < slabs; ++s) {
            a += ws[2 * ((int64_t)n * slabs + s)];
            b += ws[2 * ((int64_t)n * slabs + s) + 1];
        }
        const double v = b * inv_pc_ln2;
        out[3 + n] = (float)v;
        se += a;
        vl += v;
    }
    red[0][threadIdx.x] = se, red[1][threadIdx.x] = vl;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mse = red[0][0] * inv_npc, vlb = red[1][0] / (double)N;
        out[0] = (float)mse;
        out[1] = (float)vlb;
        out[2] = vlb_weight == 0.f ? (float)mse : (float)(mse + (double)vlb_weight * vlb);
    }
}

extern "C" int pai_palette_objective_slabs(int64_t P) {
    if (P < 1 || P > (1ll << 40)) return 0;
    const int64_t s = (P + 1023) / 1024;
    return (int)(s < 256 ? s : 256);
}

static int64_t palette_objective_pps(int64_t P) {
    const int64_t slabs = pai_palette_objective_slabs(P);
    return ((P + slabs - 1) / slabs + 1023) / 1024 * 1024;
}

extern "C" int64_t pai_palette_objective_ws_floats(int N, int64_t P) {
    const int slabs = pai_palette_objective_slabs(P);
    if (N < 1 || N > 65535 || slabs == 0) return 0;
    return 4 * (int64_t)N * slabs;                     // two fp64 partial sums per (sample, slab)
}

extern "C" int pai_palette_objective(const float* model_out, const float* noise, const float* y0, const float* y_t, const int32_t* t,
                                     const float* table, int T, int N, int64_t P, int C, int learn_var, float vlb_weight, float* out,
                                     float* dout, float* ws, void* stream) {
    PAI_CHECK(model_out && noise && y0 && y_t && t && table && out && dout && ws, "pai_palette_objective: null tensor");
    PAI_CHECK(N >= 1 && P >= 1, "pai_palette_objective: N=%d P=%lld", N, (long long)P);
    PAI_CHECK(C >= 1 && C <= 4, "pai_palette_objective: C=%d (1..4)", C);
    PAI_CHECK(T >= 1, "pai_palette_objective: T=%d", T);
    PAI_CHECK(PAI_ALIGNED16(model_out) && PAI_ALIGNED16(noise) && PAI_ALIGNED16(y0) && PAI_ALIGNED16(y_t) && PAI_ALIGNED16(t) &&
                  PAI_ALIGNED16(table) && PAI_ALIGNED16(out) && PAI_ALIGNED16(dout) && PAI_ALIGNED16(ws),
              "pai_palette_objective: tensors must be 16-byte aligned");
    PAI_CHECK(N <= 65535 && P <= (1ll << 40), "pai_palette_objective: tensor too large (N=%d P=%lld)", N, (long long)P);
    const int slabs = pai_palette_objective_slabs(P);
    const int64_t pps = palette_objective_pps(P);
    const double npc = (double)N * (double)P * (double)C;
    const float ge = (float)(2.0 / npc), gvs = (float)((double)vlb_weight * 0.5 / (npc * 0.6931471805599453));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)slabs, (unsigned)N);
    double* w = (double*)ws;
#define PAI_POBJ_VEC(CC)                                                                                                          \
    case CC:                                                                                                                      \
        if (learn_var)                                                                                                            \
            PAI_LAUNCH((palette_objective_vec_k<CC, true>), grid, dim3(256), 0, s, model_out, noise, y0, y_t, t, table, T, P, \
                               pps, ge, gvs, dout, w);                                                                            \
        else                                                                                                                      \
            PAI_LAUNCH((palette_objective_vec_k<CC, false>), grid, dim3(256), 0, s, model_out, noise, y0, y_t, t, table, T, P, \
                               pps, ge, gvs, dout, w);                                                                            \
        break;
    if (P % 4 == 0) {
        switch (C) {
            PAI_POBJ_VEC(1)
            PAI_POBJ_VEC(2)
            PAI_POBJ_VEC(3)
            PAI_POBJ_VEC(4)
        }
    } else if (learn_var) {
        PAI_LAUNCH(palette_objective_px_k<true>, grid, dim3(256), 0, s, model_out, noise, y0, y_t, t, table, T, P, pps, C, ge,
                           gvs, dout, w);
    } else {
        PAI_LAUNCH(palette_objective_px_k<false>, grid, dim3(256), 0, s, model_out, noise, y0, y_t, t, table, T, P, pps, C, ge,
                           gvs, dout, w);
    }
#undef PAI_POBJ_VEC
    PAI_LAUNCH_CHECK();
    PAI_LAUNCH(palette_objective_fin_k, dim3(1), dim3(256), 0, s, (const double*)w, N, slabs, 1.0 / npc,
                       1.0 / ((double)P * (double)C * 0.6931471805599453), vlb_weight, out);
    PAI_LAUNCH_CHECK();
    return 0;
}
