// Device-resident data set: the reference's image resize on the GPU (run once per file, at setup) and the per-step
// assembly of a batch from the cached images (reference dataset.py:51-59,129-132: read_image(GRAY) -> Resize((256, 256),
// antialias=True) on uint8 -> float32 / 255 -> (x - 0.5) / 0.5; dataset.py:77-107: the DataLoader that stacks a batch).
//
//   resize_aa_u8_k   uint8 [n, H, W] -> uint8 [n, S, S]: cast to fp32, aten's antialiased bilinear filter (separable, W pass
//                    first, fp32 intermediate, not rounded), round half to even, cast to uint8.  Byte-identical to the host
//                    operator: the fp32 weight tables come from the host (dataset.aa_tables), and every output value is
//                    t = src[0] * w[0], then t = fma(src[j], w[j], t) in ascending j -- the sums aten's vectorised CPU
//                    kernel forms.  Written with __fmul_rn / fmaf so that no contraction setting decides the rounding.
//   batch_gather_k   out[b] = value(cache[idx[b]]) for both tensors of a pair: uint8 bytes through a 256-entry fp32 table
//                    (byte / 255, optionally * 2 - 1, built on the host with the expression of dataset.load_gray_256), or
//                    fp32 images copied as they are.
#include "common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- antialiased bilinear resize ----------------------------------------------------------------------------------------
// One workgroup owns `TR` output rows of one image.  It fills the horizontally resized source rows those output rows read
// ([ylo, yhi) of the source, S fp32 values each) into LDS, then runs the vertical pass from LDS.
// Tables per axis: bounds[o] = (first source index, number of taps), weights[o][K] (zero padded).  A NULL table means the
// axis keeps its size and the pass is skipped (aten skips it too; the tables of equal sizes are the identity anyway).
__global__ __launch_bounds__(256) void resize_aa_u8_k(const unsigned char* __restrict__ src, int H, int W, int S, int TR,
                                                      const int2* __restrict__ wb, const float* __restrict__ ww, int KW,
                                                      const int2* __restrict__ hb, const float* __restrict__ hw, int KH,
                                                      int lds_rows, unsigned char* __restrict__ dst) {
    extern __shared__ float rows[];          // [lds_rows][S]
    const int y0 = blockIdx.x * TR, y1 = min(S, y0 + TR);
    const unsigned char* img = src + (size_t)blockIdx.y * H * W;
    unsigned char* out = dst + (size_t)blockIdx.y * S * S;
    int ylo = y0, yhi = y1;
    if (hb) {
        ylo = max(hb[y0].x, 0);
        const int2 last = hb[y1 - 1];
        yhi = last.x + last.y;
    }
    // the host sized the LDS for the widest tile of this table: a table that disagrees must not write outside it
    yhi = min(min(yhi, H), ylo + lds_rows);
    const int nrow = yhi - ylo;
    if (nrow <= 0) return;                   // (uniform over the workgroup)
    for (int i = threadIdx.x; i < nrow * S; i += 256) {
        const int r = i / S, x = i - r * S;
        const unsigned char* p = img + (size_t)(ylo + r) * W;
        float t;
        if (wb) {
            const int2 b = wb[x];
            const int x0 = min(max(b.x, 0), W - 1), nt = min(min(b.y, KW), W - x0);
            const float* w = ww + (size_t)x * KW;
            t = __fmul_rn((float)p[x0], w[0]);
            for (int j = 1; j < nt; ++j) t = fmaf((float)p[x0 + j], w[j], t);
        } else {
            t = (float)p[x];
        }
        rows[i] = t;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (y1 - y0) * S; i += 256) {
        const int ry = i / S, x = i - ry * S, y = y0 + ry;
        float t;
        if (hb) {
            const int2 b = hb[y];
            const int r0 = min(max(b.x - ylo, 0), nrow - 1), nt = min(min(b.y, KH), nrow - r0);
            const float* w = hw + (size_t)y * KH;
            t = __fmul_rn(rows[r0 * S + x], w[0]);
            for (int j = 1; j < nt; ++j) t = fmaf(rows[(r0 + j) * S + x], w[j], t);
        } else {
            t = rows[ry * S + x];
        }
        out[(size_t)y * S + x] = (unsigned char)(int)rintf(t);      // v_rndne_f32: half to even, as Tensor.round()
    }
}

// LDS of one CDNA4 compute unit a single workgroup may take (160 KB); up to 64 KB needs no attribute
static const int64_t LDS_PLAIN = 64 * 1024, LDS_MAX = 160 * 1024;

// source rows the vertical pass of output rows [y0, y0 + tr) reads, from the HOST copy of the bounds
static int tile_rows(const int* hb_host, int S, int tr) {
    int need = 0;
    for (int y0 = 0; y0 < S; y0 += tr) {
        const int y1 = (y0 + tr < S ? y0 + tr : S) - 1;
        const int n = hb_host[2 * y1] + hb_host[2 * y1 + 1] - hb_host[2 * y0];
        if (n > need) need = n;
    }
    return need;
}

extern "C" int pai_resize_aa_u8(const void* src, int n, int H, int W, int S, const int* wbounds, const float* wweights,
                                int KW, const int* hbounds, const float* hweights, int KH, const int* hbounds_host,
                                void* dst, void* stream) {
    PAI_CHECK(src && dst && n >= 0 && H > 0 && W > 0 && S > 0, "pai_resize_aa_u8: bad arguments");
    PAI_CHECK((wbounds != nullptr) == (wweights != nullptr) && (hbounds != nullptr) == (hweights != nullptr),
              "pai_resize_aa_u8: bounds and weights of an axis come together");
    PAI_CHECK(wbounds ? (KW >= 1 && W != S) : W == S, "pai_resize_aa_u8: W = %d -> %d needs a width table, equal sizes take none", W, S);
    PAI_CHECK(hbounds ? (KH >= 1 && H != S && hbounds_host) : H == S,
              "pai_resize_aa_u8: H = %d -> %d needs a height table (device and host copy), equal sizes take none", H, S);
    PAI_CHECK((int64_t)n <= 65535, "pai_resize_aa_u8: at most 65535 images per call (got %d)", n);
    if (n == 0) return 0;
    int tr = 8, need = 0;
    for (;; tr >>= 1) {
        need = hbounds ? tile_rows(hbounds_host, S, tr) : tr;
        PAI_CHECK(need >= 1 && need <= H, "pai_resize_aa_u8: the height table reads %d rows of a %d-row image", need, H);
        if ((int64_t)need * S * 4 <= LDS_PLAIN || tr == 1) break;
    }
    const int64_t lds = (int64_t)need * S * 4;
    PAI_CHECK(lds <= LDS_MAX, "pai_resize_aa_u8: %d x %d -> %d: one output row reads %d source rows (%lld bytes of LDS, limit %lld)",
              H, W, S, need, (long long)lds, (long long)LDS_MAX);
    if (lds > LDS_PLAIN) {
        hipError_t e = hipFuncSetAttribute((const void*)resize_aa_u8_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
        PAI_CHECK(e == hipSuccess, "pai_resize_aa_u8: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    PAI_LAUNCH(resize_aa_u8_k, dim3(cdiv(S, tr), n), dim3(256), lds, (hipStream_t)stream, (const unsigned char*)src, H, W, S, tr,
               (const int2*)wbounds, wweights, KW, (const int2*)hbounds, hweights, KH, need, (unsigned char*)dst);
    PAI_LAUNCH_CHECK();
    return 0;
}

// ---- batch assembly -----------------------------------------------------------------------------------------------------
// grid = (blocks per image, images of the batch, 2 tensors of a pair).  The image a workgroup copies is fixed, so the source
// and destination bases are loop invariant; GV 16-byte loads are in flight per thread before the first store.
constexpr int GV = 4;

template <typename T> struct Gather;
template <> struct Gather<unsigned char> {      // 16 pixels per 16-byte load, four 16-byte stores
    static constexpr int PIX = 16;
    static __device__ __forceinline__ void put(u32x4 v, const float* lut, float* o) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f32x4 f;
            f[0] = lut[v[k] & 255u];
            f[1] = lut[(v[k] >> 8) & 255u];
            f[2] = lut[(v[k] >> 16) & 255u];
            f[3] = lut[v[k] >> 24];
            *(f32x4*)(o + 4 * k) = f;
        }
    }
};
template <> struct Gather<float> {              // 4 pixels per 16-byte load, one store
    static constexpr int PIX = 4;
    static __device__ __forceinline__ void put(u32x4 v, const float*, float* o) { *(u32x4*)o = v; }
};

template <typename T>
__global__ __launch_bounds__(256) void batch_gather_k(const T* __restrict__ ca, const T* __restrict__ cb, int64_t M,
                                                      const int64_t* __restrict__ idx, int64_t per_image,
                                                      const float* __restrict__ table, float* __restrict__ oa,
                                                      float* __restrict__ ob) {
    __shared__ float lut[256];
    if (sizeof(T) == 1) {
        lut[threadIdx.x] = table[threadIdx.x];
        __syncthreads();
    }
    const int64_t im = idx[blockIdx.y];
    if (im < 0 || im >= M) return;              // an index outside the cache reads nothing (the host checks them as well)
    const T* s = (blockIdx.z ? cb : ca) + im * per_image;
    float* d = (blockIdx.z ? ob : oa) + (int64_t)blockIdx.y * per_image;
    constexpr int PIX = Gather<T>::PIX;
    const int nvec = (int)(per_image / PIX);
    const int step = gridDim.x * 256 * GV;
    for (int i = blockIdx.x * 256 * GV + threadIdx.x; i < nvec; i += step) {
        u32x4 v[GV];
#pragma unroll
        for (int k = 0; k < GV; ++k)
            if (i + k * 256 < nvec) v[k] = *(const u32x4*)(s + (size_t)(i + k * 256) * PIX);
#pragma unroll
        for (int k = 0; k < GV; ++k)
            if (i + k * 256 < nvec) Gather<T>::put(v[k], lut, d + (size_t)(i + k * 256) * PIX);
    }
}

extern "C" int pai_batch_gather(int src_dtype, const void* cache_a, const void* cache_b, int64_t M, int64_t per_image,
                                const int64_t* indices, int count, const float* table, float* out_a, float* out_b,
                                void* stream) {
    PAI_CHECK(src_dtype == PAI_U8 || src_dtype == PAI_F32, "pai_batch_gather: source dtype %d (PAI_U8 or PAI_F32 expected)", src_dtype);
    PAI_CHECK(cache_a && cache_b && indices && out_a && out_b && M > 0 && count >= 0, "pai_batch_gather: bad arguments");
    PAI_CHECK(src_dtype != PAI_U8 || table, "pai_batch_gather: a uint8 cache needs the 256-entry value table");
    const int pix = src_dtype == PAI_U8 ? 16 : 4;
    PAI_CHECK(per_image > 0 && per_image % pix == 0 && per_image / pix <= INT32_MAX / 2,
              "pai_batch_gather: %lld elements per image (a multiple of %d expected)", (long long)per_image, pix);
    PAI_CHECK(((((uintptr_t)cache_a) | ((uintptr_t)cache_b) | ((uintptr_t)out_a) | ((uintptr_t)out_b)) & 15) == 0,
              "pai_batch_gather: 16-byte aligned buffers expected");
    PAI_CHECK(count <= 65535, "pai_batch_gather: at most 65535 images per batch (got %d)", count);
    if (count == 0) return 0;
    const dim3 grid(cdiv(per_image / pix, 256 * GV), count, 2);
    if (src_dtype == PAI_U8)
        PAI_LAUNCH(batch_gather_k<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)cache_a,
                   (const unsigned char*)cache_b, M, indices, per_image, table, out_a, out_b);
    else
        PAI_LAUNCH(batch_gather_k<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)cache_a, (const float*)cache_b,
                   M, indices, per_image, table, out_a, out_b);
    PAI_LAUNCH_CHECK();
    return 0;
}

extern "C" int pai_data_kernel_name(int op, int src_dtype, char* name, int name_len) {
    PAI_CHECK(name && name_len > 0, "pai_data_kernel_name: bad arguments");
    const char* s = op == 0 ? "resize_aa_u8_k"
                            : (op == 1 ? (src_dtype == PAI_U8 ? "batch_gather_k<unsigned char>" : "batch_gather_k<float>") : nullptr);
    PAI_CHECK(s, "pai_data_kernel_name: op %d (0 resize, 1 batch gather)", op);
    snprintf(name, (size_t)name_len, "%s", s);
    return 0;
}
