// SSIM (Gaussian 11x11, sigma 1.5) + squared-error sums in one pass over the image pair, and the
// gradient of the SSIM / PSNR losses.  Replaces torchmetrics.functional
// structural_similarity_index_measure / peak_signal_noise_ratio / mean_squared_error as called
// from models/utils.py:38-47 (data_range = 1.0) and report.py:78-96,207-212, including the
// denormalisation of models/utils.py:11 in front of them.
//
// The window is applied separably (11 + 11 taps instead of 121) from an LDS tile with a 5-px halo;
// reflect padding supplies the halo at image borders exactly like torchmetrics does, the per-image
// value is the mean over the map cropped by 5 px.
#include <math.h>

#include "common.h"

constexpr int KS = 11, PADW = 5;
constexpr int TS = 32;            // output tile
constexpr int TI = TS + 2 * PADW; // 42 input rows/cols
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

struct Gauss { float g[KS]; };

static Gauss make_gauss() {
    Gauss k;
    float sum = 0.f;
    for (int i = 0; i < KS; ++i) {
        float d = (float)(i - PADW);
        float v = d / 1.5f;
        k.g[i] = expf(-(v * v) / 2.f);
        sum += k.g[i];
    }
    for (int i = 0; i < KS; ++i) k.g[i] /= sum;
    return k;
}

__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

// clamp(u, 0, 1) as torch.clamp: a NaN stays a NaN (fmaxf(NaN, 0) = 0 would launder a diverged prediction into a black
// pixel and the metrics into finite numbers -- the ReLU epilogues of the convolutions had the same fault, common.h act_fwd)
__device__ __forceinline__ float denorm_val(float v, int denorm) {
    if (!denorm) return v;
    const float u = v * 0.5f + 0.5f;
    return u != u ? u : fminf(fmaxf(u, 0.f), 1.f);
}

// DET (deterministic mode): the two terms are rounded so that every fp64 addition into the accumulators is exact and the sums
// do not depend on the arrival order (as head_loss_k, head.hip).  a -- a workgroup's share of a plane's crop-mean SSIM, |a| <=
// 1 -- to a multiple of 2^-36 below 2^8: exact while the sum of the |terms| stays below 2^17 (at most one per plane: 131072
// planes).  b -- a sum of squared errors, >= 0 -- to a multiple of 2^-28 below 2^16: exact while the total stays below 2^25.
template <bool DET>
__device__ __forceinline__ void block_add2(double a, double b, double* da, double* db, double* dc) {
    __shared__ double ws[2][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { ws[0][wid] = a; ws[1][wid] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3];
        double sb = ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3];
        if (DET && fabs(sa) < 256.0) sa = rint(sa * 0x1p36) * 0x1p-36;
        if (DET && fabs(sb) < 65536.0) sb = rint(sb * 0x1p28) * 0x1p-28;
        if (da) atomicAdd(da, sa);
        if (dc) atomicAdd(dc, sa);
        if (db) atomicAdd(db, sb);
    }
}

// ---- the stages of one 32 x 32 output tile, shared by ssim_k and eval_planes_k (one source: the per-pixel S of the two
// kernels is the same bits) -----------------------------------------------------------------------------------------------
typedef float TileIn[TI][TI + 1];
typedef float TileH[5][TI][TS];

// stage 1: the 42 x 42 input window of both images (reflect padded, optionally denormalised) into LDS
__device__ __forceinline__ void ssim_tile_fill(const float* p, const float* t, int H, int W, int y0, int x0, int denorm,
                                               TileIn& P, TileIn& T) {
    const int tid = threadIdx.x;
    // all 2 x 7 loads of a thread are issued before the first one is consumed: written as "load, store to LDS,
    // next" the loop was seven dependent HBM round trips per tile
    constexpr int NL = (TI * TI + 255) / 256;
    float pv[NL], tv[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int idx = tid + 256 * i;
        const int r = idx / TI, c = idx - r * TI;
        const int gy = reflect_idx(y0 - PADW + (idx < TI * TI ? r : 0), H), gx = reflect_idx(x0 - PADW + c, W);
        pv[i] = p[(size_t)gy * W + gx];
        tv[i] = t[(size_t)gy * W + gx];
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int idx = tid + 256 * i;
        const int r = idx / TI, c = idx - r * TI;
        if (idx < TI * TI) {
            P[r][c] = denorm_val(pv[i], denorm);
            T[r][c] = denorm_val(tv[i], denorm);
        }
    }
}

// stage 2: horizontal pass, four neighbouring outputs per thread from one 14-value window: a third of the LDS reads and
// of the products a*a, b*b, a*b of the one-output-per-thread form (the kernel is instruction-bound, not HBM-bound)
__device__ __forceinline__ void ssim_tile_hpass(const TileIn& P, const TileIn& T, TileH& Hb, const Gauss& gk) {
    const int tid = threadIdx.x;
    for (int idx = tid; idx < TI * (TS / 4); idx += 256) {
        const int r = idx / (TS / 4), c = (idx - r * (TS / 4)) * 4;
        float wa[KS + 3], wb[KS + 3];
#pragma unroll
        for (int k = 0; k < KS + 3; ++k) { wa[k] = P[r][c + k]; wb[k] = T[r][c + k]; }
        float sp[4] = {0.f, 0.f, 0.f, 0.f}, st[4] = {0.f, 0.f, 0.f, 0.f}, spp[4] = {0.f, 0.f, 0.f, 0.f},
              stt[4] = {0.f, 0.f, 0.f, 0.f}, spt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS + 3; ++k) {
            const float a = wa[k], b = wb[k], aa = a * a, bb = b * b, ab = a * b;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (k - o >= 0 && k - o < KS) {          // same tap order per output as the scalar form: bit-identical sums
                    const float g = gk.g[k - o];
                    sp[o] = fmaf(g, a, sp[o]);
                    st[o] = fmaf(g, b, st[o]);
                    spp[o] = fmaf(g, aa, spp[o]);
                    stt[o] = fmaf(g, bb, stt[o]);
                    spt[o] = fmaf(g, ab, spt[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            Hb[0][r][c + o] = sp[o]; Hb[1][r][c + o] = st[o]; Hb[2][r][c + o] = spp[o]; Hb[3][r][c + o] = stt[o];
            Hb[4][r][c + o] = spt[o];
        }
    }
}

// stage 3: vertical pass: a thread owns column ox and the four rows 4 (tid >> 5) .. +3, one 14-row window per map
__device__ __forceinline__ void ssim_tile_vpass(const TileH& Hb, const Gauss& gk, float (&vm)[5][4]) {
    const int tid = threadIdx.x;
    const int oyb = (tid >> 5) * 4, ox = tid & 31;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        float w[KS + 3];
#pragma unroll
        for (int k = 0; k < KS + 3; ++k) w[k] = Hb[m][oyb + k][ox];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float acc_ = 0.f;
#pragma unroll
            for (int k = 0; k < KS; ++k) acc_ = fmaf(gk.g[k], w[o + k], acc_);
            vm[m][o] = acc_;
        }
    }
}

// stage 4: the SSIM value of output row j of the thread and the factors the gradient needs
struct SsimPix { float mp, mt, A1, A2, B1, B2, S; };
__device__ __forceinline__ SsimPix ssim_pix(const float (&vm)[5][4], int j) {
    SsimPix q;
    q.mp = vm[0][j]; q.mt = vm[1][j];
    const float mp = q.mp, mt = q.mt, epp = vm[2][j], ett = vm[3][j], ept = vm[4][j];
    const float spp = epp - mp * mp, stt = ett - mt * mt, spt = ept - mp * mt;
    q.A1 = 2.f * mp * mt + SSIM_C1; q.A2 = 2.f * spt + SSIM_C2;
    q.B1 = mp * mp + mt * mt + SSIM_C1; q.B2 = spp + stt + SSIM_C2;
    q.S = (q.A1 * q.A2) / (q.B1 * q.B2);
    return q;
}

// MODE 0: forward metrics.  MODE 1: write the three gradient maps (backward pass 1).  MODE 2: MODE 0 with the workgroups'
// terms rounded for exact addition (deterministic mode, block_add2).
template <int MODE>
__global__ __launch_bounds__(256) void ssim_k(const float* pred, const float* target, int H, int W, int denorm,
                                              Gauss gk, double inv_crop, double* out2, double* per_image,
                                              float* full_map, float* dmaps, int NC, float wscale, int xtiles) {
    __shared__ TileIn P, T;
    __shared__ TileH Hb;
    const int tid = threadIdx.x;
    const int nc = blockIdx.z;
    const int y0 = blockIdx.y * TS;
    const float* p = pred + (size_t)nc * H * W;
    const float* t = target + (size_t)nc * H * W;
    // One workgroup walks `xtiles` 32-pixel tiles of its tile row (MODE 0: the whole row, so that the three fp64
    // atomics per workgroup -- all workgroups add to the same two or three words -- happen 512 instead of 4096
    // times per 64-image batch: same-address atomics serialise at the memory side and were most of the 154 us)
    double acc = 0.0, sse = 0.0;
    for (int xt = blockIdx.x * xtiles; xt < (blockIdx.x + 1) * xtiles && xt * TS < W; ++xt) {
    const int x0 = xt * TS;
    if (xt != blockIdx.x * xtiles) __syncthreads();      // the previous tile's readers are done with P, T, Hb
    ssim_tile_fill(p, t, H, W, y0, x0, denorm, P, T);
    __syncthreads();
    ssim_tile_hpass(P, T, Hb, gk);
    __syncthreads();
    float vm[5][4];
    ssim_tile_vpass(Hb, gk, vm);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = (tid >> 5) * 4 + j, ox = tid & 31;
        const int y = y0 + oy, x = x0 + ox;
        if (y >= H || x >= W) continue;
        const SsimPix q = ssim_pix(vm, j);
        const float mp = q.mp, mt = q.mt, A1 = q.A1, A2 = q.A2, B1 = q.B1, B2 = q.B2, S = q.S;
        const bool in_crop = y >= PADW && y < H - PADW && x >= PADW && x < W - PADW;
        if (MODE != 1) {
            if (full_map) full_map[((size_t)nc * H + y) * W + x] = S;
            if (in_crop) acc += (double)S;
            const float d = P[oy + PADW][ox + PADW] - T[oy + PADW][ox + PADW];
            sse += (double)d * d;
        } else {
            // d(mean SSIM)/d{mu_p, E[pp], E[pt]} at this window, weighted by the crop mean
            float dmu = 0.f, dpp = 0.f, dpt = 0.f;
            if (in_crop) {
                const float inv = 1.f / (B1 * B2);
                dmu = (2.f * mt * (A2 - A1)) * inv - S * (2.f * mp / B1 - 2.f * mp / B2);
                dpp = -S / B2;
                dpt = 2.f * A1 * inv;
                dmu *= wscale; dpp *= wscale; dpt *= wscale;
            }
            const size_t plane = (size_t)H * W, o = ((size_t)nc * H + y) * W + x;
            dmaps[o] = dmu;
            dmaps[(size_t)NC * plane + o] = dpp;
            dmaps[2 * (size_t)NC * plane + o] = dpt;
        }
    }
    }   // x tiles
    if (MODE != 1)
        block_add2<MODE == 2>(acc * inv_crop, sse, out2, out2 ? out2 + 1 : nullptr, per_image ? per_image + nc : nullptr);
}

extern "C" int pai_ssim_sse(const float* pred, const float* target, int NC, int H, int W, int denorm,
                            double* out2, double* per_image, float* full_map, void* stream) {
    PAI_CHECK(pred && target && (out2 || per_image || full_map), "pai_ssim_sse: null pointer");
    PAI_CHECK(H > 2 * PADW && W > 2 * PADW, "pai_ssim_sse: image %dx%d smaller than the 11x11 window", H, W);
    static const Gauss gk = make_gauss();
    const double inv_crop = 1.0 / ((double)(H - 2 * PADW) * (double)(W - 2 * PADW));
    // whole tile rows per workgroup once there are enough of them to fill the chip
    const int xt_all = cdiv(W, TS);
    int xtiles = pai_tunable("ssim_rowtiles", 8);
    if (xtiles < 1 || (int64_t)cdiv(H, TS) * NC < 512) xtiles = 1;
    if (xtiles > xt_all) xtiles = xt_all;
    dim3 grid(cdiv(xt_all, xtiles), cdiv(H, TS), NC);
    if (pai_deterministic()) {
        PAI_LAUNCH(ssim_k<2>, grid, dim3(256), 0, (hipStream_t)stream, pred, target, H, W, denorm, gk,
                           inv_crop, out2, per_image, full_map, (float*)nullptr, NC, 0.f, xtiles);
    } else {
        if (out2 || per_image) pai_note_order_dependent();
        PAI_LAUNCH(ssim_k<0>, grid, dim3(256), 0, (hipStream_t)stream, pred, target, H, W, denorm, gk,
                           inv_crop, out2, per_image, full_map, (float*)nullptr, NC, 0.f, xtiles);
    }
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- report evaluation (pai_eval_planes, entry point in eval.hip) --------------------------------------------------------
// ssim_k<0>'s pass with per-plane sums and 8-bit outputs: the SSIM map as to_int(clamp(S, 0, 1)) and the prediction through
// a 256-entry RGB table.  The bytes of a tile are staged in LDS and leave as 32-bit words.
typedef unsigned char TileU8[TS][TS];

// One staged 32 x 32 byte tile -> rows y0.., columns x0.. of a [H][W] byte plane.  `aligned` (plane base and W multiples of
// 4): every word of the tile lies fully inside or fully outside the plane, one plain store per thread.  Otherwise a row
// starts at any byte: up to 9 words per tile row, whole ones stored, the partial ones at both ends merged with a 32-bit
// atomic and / or pair (the other bytes of such a word belong to the neighbouring tile, row or plane, maybe of another
// workgroup; the last word of the buffer may reach into its padding).
__device__ __forceinline__ void store_tile_u8(const TileU8& st, unsigned char* plane, int H, int W, int y0, int x0, bool aligned) {
    const int tid = threadIdx.x;
    if (aligned) {
        const int r = tid >> 3, c = (tid & 7) * 4;
        if (y0 + r < H && x0 + c < W)
            *(unsigned*)(plane + (size_t)(y0 + r) * W + x0 + c) = *(const unsigned*)&st[r][c];
        return;
    }
    const int cols = min(TS, W - x0);
    for (int i = tid; i < TS * 9; i += 256) {
        const int r = i / 9, k = i - r * 9;
        if (y0 + r >= H) continue;
        const uintptr_t s = (uintptr_t)(plane + (size_t)(y0 + r) * W + x0), e = s + cols;
        const uintptr_t w0 = ((s >> 2) + k) << 2;                // this word covers bytes [w0, w0 + 4)
        const uintptr_t lo = max(w0, s), hi = min(w0 + 4, e);
        if (lo >= hi) continue;
        unsigned v = 0, mask = 0;
        for (uintptr_t b = lo; b < hi; ++b) {
            v |= (unsigned)st[r][b - s] << (8 * (b - w0));
            mask |= 0xffu << (8 * (b - w0));
        }
        unsigned* dst = (unsigned*)w0;
        if (mask == 0xffffffffu) {
            *dst = v;
        } else {
            atomicAnd(dst, ~mask);
            atomicOr(dst, v);
        }
    }
}

template <bool DET>
__device__ __forceinline__ void eval_planes_body(const float* pred, const float* target, int H, int W, int denorm,
                                                 const Gauss& gk, double inv_crop, double* ssim_plane, double* sse_plane,
                                                 unsigned char* map_u8, const unsigned char* lut_rgb,
                                                 unsigned char* hot_u8, int xtiles, int aligned) {
    __shared__ TileIn P, T;
    __shared__ TileH Hb;
    __shared__ __align__(16) TileU8 st[4];                 // SSIM map, R, G, B
    __shared__ unsigned lut[256];            // R | G << 8 | B << 16
    const int tid = threadIdx.x;
    const int nc = blockIdx.z;
    const int y0 = blockIdx.y * TS;
    const float* p = pred + (size_t)nc * H * W;
    const float* t = target + (size_t)nc * H * W;
    const size_t plane = (size_t)H * W;
    if (hot_u8) lut[tid] = lut_rgb[3 * tid] | (unsigned)lut_rgb[3 * tid + 1] << 8 | (unsigned)lut_rgb[3 * tid + 2] << 16;
    double acc = 0.0, sse = 0.0;
    for (int xt = blockIdx.x * xtiles; xt < (blockIdx.x + 1) * xtiles && xt * TS < W; ++xt) {
        const int x0 = xt * TS;
        if (xt != blockIdx.x * xtiles) __syncthreads();      // the previous tile's readers are done with P, T, Hb, st
        ssim_tile_fill(p, t, H, W, y0, x0, denorm, P, T);
        __syncthreads();
        ssim_tile_hpass(P, T, Hb, gk);
        __syncthreads();
        float vm[5][4];
        ssim_tile_vpass(Hb, gk, vm);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oy = (tid >> 5) * 4 + j, ox = tid & 31;
            const int y = y0 + oy, x = x0 + ox;
            if (y >= H || x >= W) continue;
            const float S = ssim_pix(vm, j).S;
            if (y >= PADW && y < H - PADW && x >= PADW && x < W - PADW) acc += (double)S;
            const float pv = P[oy + PADW][ox + PADW];
            const float d = pv - T[oy + PADW][ox + PADW];
            sse += (double)d * d;
            if (map_u8) st[0][oy][ox] = (unsigned char)__fmul_rn(fminf(fmaxf(S, 0.f), 1.f), 255.999f);
            if (hot_u8) {
                // matplotlib's Colormap.__call__ on floats: int(x * N) clipped to the table, NaN -> the "bad" colour (black)
                const unsigned c = pv != pv ? 0u : lut[min(max((int)(pv * 256.f), 0), 255)];
                st[1][oy][ox] = (unsigned char)c;
                st[2][oy][ox] = (unsigned char)(c >> 8);
                st[3][oy][ox] = (unsigned char)(c >> 16);
            }
        }
        if (map_u8 || hot_u8) {
            __syncthreads();
            if (map_u8) store_tile_u8(st[0], map_u8 + (size_t)nc * plane, H, W, y0, x0, aligned);
            if (hot_u8) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    store_tile_u8(st[1 + ch], hot_u8 + ((size_t)nc * 3 + ch) * plane, H, W, y0, x0, aligned);
            }
        }
    }
    // one addition per workgroup and sum, to the words of its own plane
    block_add2<DET>(acc * inv_crop, sse, ssim_plane ? ssim_plane + nc : nullptr, sse_plane ? sse_plane + nc : nullptr, nullptr);
}
__global__ __launch_bounds__(256) void eval_planes_k(const float* pred, const float* target, int H, int W, int denorm,
                                                     Gauss gk, double inv_crop, double* ssim_plane, double* sse_plane,
                                                     unsigned char* map_u8, const unsigned char* lut_rgb,
                                                     unsigned char* hot_u8, int xtiles, int aligned) {
    eval_planes_body<false>(pred, target, H, W, denorm, gk, inv_crop, ssim_plane, sse_plane, map_u8, lut_rgb, hot_u8, xtiles, aligned);
}
// deterministic mode: the workgroups of a plane add rounded terms (block_add2)
__global__ __launch_bounds__(256) void eval_planes_det_k(const float* pred, const float* target, int H, int W, int denorm,
                                                         Gauss gk, double inv_crop, double* ssim_plane, double* sse_plane,
                                                         unsigned char* map_u8, const unsigned char* lut_rgb,
                                                         unsigned char* hot_u8, int xtiles, int aligned) {
    eval_planes_body<true>(pred, target, H, W, denorm, gk, inv_crop, ssim_plane, sse_plane, map_u8, lut_rgb, hot_u8, xtiles, aligned);
}

const char* eval_planes_kernel_name() { return pai_deterministic() ? "eval_planes_det_k" : "eval_planes_k"; }

int launch_eval_planes(const float* pred, const float* target, int NC, int H, int W, int denorm, double* ssim_plane,
                       double* sse_plane, unsigned char* map_u8, const unsigned char* lut_rgb, unsigned char* hot_u8,
                       hipStream_t stream) {
    static const Gauss gk = make_gauss();
    const double inv_crop = 1.0 / ((double)(H - 2 * PADW) * (double)(W - 2 * PADW));
    // whole tile rows per workgroup, as ssim_k<0> (very wide images: eight tiles each)
    const int xt_all = cdiv(W, TS);
    const int xtiles = xt_all < 8 ? xt_all : 8;
    const int aligned = W % 4 == 0 && (((uintptr_t)map_u8 | (uintptr_t)hot_u8) & 3) == 0;
    dim3 grid(cdiv(xt_all, xtiles), cdiv(H, TS), NC);
    const bool several = grid.x * grid.y > 1 && (ssim_plane || sse_plane);      // workgroups per plane word
    if (pai_deterministic())
        PAI_LAUNCH(eval_planes_det_k, grid, dim3(256), 0, stream, pred, target, H, W, denorm, gk, inv_crop, ssim_plane, sse_plane,
                   map_u8, lut_rgb, hot_u8, xtiles, aligned);
    else {
        if (several) pai_note_order_dependent();
        PAI_LAUNCH(eval_planes_k, grid, dim3(256), 0, stream, pred, target, H, W, denorm, gk, inv_crop, ssim_plane, sse_plane,
                   map_u8, lut_rgb, hot_u8, xtiles, aligned);
    }
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t pai_ssim_bwd_workspace_floats(int NC, int H, int W) { return (int64_t)3 * NC * H * W; }

// backward pass 2: grad_i = dp/dpred * [ -(G*Dmu)_i - 2 p_i (G*Dpp)_i - t_i (G*Dpt)_i  (SSIM part)
//                                         + w_psnr * (20/ln10) (p_i - t_i) / SSE ]      (PSNR part)
// G* = zero-padded separable Gaussian correlation (the maps vanish outside the crop).
__global__ __launch_bounds__(256) void ssim_bwd2_k(const float* pred, const float* target, int H, int W,
                                                   int denorm, Gauss gk, const float* dmaps, int NC,
                                                   float w_psnr, const double* sse, float* grad) {
    __shared__ float D[3][TI][TI + 1];
    __shared__ float Hb[3][TI][TS];
    const int tid = threadIdx.x, nc = blockIdx.z;
    const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
    const size_t plane = (size_t)H * W;
    for (int idx = tid; idx < TI * TI; idx += 256) {
        const int r = idx / TI, c = idx - r * TI;
        const int gy = y0 - PADW + r, gx = x0 - PADW + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const size_t o = ((size_t)nc * H + (in ? gy : 0)) * W + (in ? gx : 0);
#pragma unroll
        for (int q = 0; q < 3; ++q) D[q][r][c] = in ? dmaps[q * (size_t)NC * plane + o] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < TI * TS; idx += 256) {
        const int r = idx / TS, c = idx - r * TS;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const float g = gk.g[k];
            s0 = fmaf(g, D[0][r][c + k], s0);
            s1 = fmaf(g, D[1][r][c + k], s1);
            s2 = fmaf(g, D[2][r][c + k], s2);
        }
        Hb[0][r][c] = s0; Hb[1][r][c] = s1; Hb[2][r][c] = s2;
    }
    __syncthreads();
    const float psnr_k = w_psnr != 0.f ? (float)(w_psnr * (20.0 / log(10.0)) / *sse) : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = (tid >> 5) + 8 * j, ox = tid & 31;
        const int y = y0 + oy, x = x0 + ox;
        if (y >= H || x >= W) continue;
        float f0 = 0.f, f1 = 0.f, f2 = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const float g = gk.g[k];
            f0 = fmaf(g, Hb[0][oy + k][ox], f0);
            f1 = fmaf(g, Hb[1][oy + k][ox], f1);
            f2 = fmaf(g, Hb[2][oy + k][ox], f2);
        }
        const size_t o = ((size_t)nc * H + y) * W + x;
        const float raw = pred[o];
        const float pv = denorm_val(raw, denorm), tv = denorm_val(target[o], denorm);
        float dd = 1.f;
        if (denorm) {
            const float u = raw * 0.5f + 0.5f;
            dd = (u > 0.f && u < 1.f) ? 0.5f : 0.f;   // clamp passes gradient strictly inside (torch.clamp)
            if (u == 0.f || u == 1.f) dd = 0.5f;      // torch: gradient 1 at the boundary values
        }
        const float gs = -(f0 + 2.f * pv * f1 + tv * f2);
        grad[o] = dd * (gs + psnr_k * (pv - tv));
    }
}

extern "C" int pai_ssim_psnr_bwd(const float* pred, const float* target, int NC, int H, int W, int denorm,
                                 float w_ssim, float w_psnr, const double* sse, float* grad,
                                 float* workspace, void* stream) {
    PAI_CHECK(pred && target && grad && workspace, "pai_ssim_psnr_bwd: null pointer");
    PAI_CHECK(w_psnr == 0.f || sse, "pai_ssim_psnr_bwd: PSNR term needs sse");
    PAI_CHECK(H > 2 * PADW && W > 2 * PADW, "pai_ssim_psnr_bwd: image too small");
    static const Gauss gk = make_gauss();
    const double crop = (double)(H - 2 * PADW) * (double)(W - 2 * PADW);
    // loss = -(w_ssim * mean over NC planes of the crop mean + w_psnr * PSNR)
    const float wscale = (float)((double)w_ssim / (crop * (double)NC));
    dim3 grid(cdiv(W, TS), cdiv(H, TS), NC);
    hipStream_t s = (hipStream_t)stream;
    PAI_LAUNCH(ssim_k<1>, grid, dim3(256), 0, s, pred, target, H, W, denorm, gk, 0.0,
                       (double*)nullptr, (double*)nullptr, (float*)nullptr, workspace, NC, wscale, 1);
    PAI_LAUNCH_CHECK();
    PAI_LAUNCH(ssim_bwd2_k, grid, dim3(256), 0, s, pred, target, H, W, denorm, gk, workspace, NC,
                       w_psnr, sse, grad);
    PAI_LAUNCH_CHECK();
    return 0;
}
