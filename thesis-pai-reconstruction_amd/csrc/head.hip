// The PatchGAN head (Conv2d(Cin, 1, k4, s1, p1, bias=False), reference models/wrapper.py:233) with everything that hangs on
// its logits in ONE launch: logits, BCE-with-logits against a per-image constant target (the fp64 loss sum and the logit
// gradient), and the head's input gradient with the LeakyReLU derivative of the block in front of it.  As separate
// launches (thin_dgrad_gemm_k + thin_col2im_k, loss_k x 2, cast_k, head_dgrad_k) these ran alone on the main queue, each a
// 5-20 us launch around 28,800 logits and one 33.5 MB tensor (batch 128).  Every value is computed by the expressions of
// the launches it replaces, in their order: logits, bf16 logit gradient and input gradient have the same bits; the loss
// is summed per image instead of per half (below one ulp of the fp32 value it becomes) and does not depend on the order of
// the atomics.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf8_t;
typedef __attribute__((ext_vector_type(4))) float f4_t;

constexpr int HL_THREADS = 512, HL_WAVES = HL_THREADS / 64;
constexpr int HL_LD = 17;                         // floats per pixel row of the tap values (16 + 1: no bank conflicts)
constexpr int64_t HL_LDS_MAX = 96 * 1024;         // of the 160 KB of a CU: 32 x 32 pixels at 512 channels need 89 KB

struct HeadLoss {
    const bf16_t* a3;        // [N][H][W][C]: the head's input = the stored activation of the block in front of it
    const bf16_t* wf;        // forward pack [16 taps][C]
    const bf16_t* wd;        // input-gradient pack [C][16 taps] (du != NULL)
    float* logits;           // [N][OH][OW]
    bf16_t* dl;              // bf16 logit gradient or NULL
    float* dl32;             // fp32 logit gradient or NULL
    bf16_t* du;              // [N][H][W][C] or NULL
    const bf16_t* act_src;   // stored activation whose sign carries act' (du != NULL)
    double* loss;
    int N, H, W, C, OH, OW;
    int n_first;             // images below it: (t_first, ls_first, gs_first)
    float t_first, t_rest;
    double ls_first, ls_rest;    // loss_scale / numel of the half
    float gs_first, gs_rest;     // grad_scale / numel of the half
    int act;
    int rg;                  // workgroups per image: each owns H / rg pixel rows of du and recomputes the image's logits
    int xcd;                 // N % 8 == 0: the workgroups of one image are 8 apart (same XCD, same L2)
};

static int64_t head_loss_lds_bytes(int H, int W, int C, bool with_du) {
    const int64_t ys = (((int64_t)H * W * HL_LD * 4) + 15) & ~(int64_t)15;
    const int64_t dls = (((int64_t)(H - 1) * (W - 1) * 4) + 15) & ~(int64_t)15;
    return ys + dls + (with_du ? (int64_t)16 * C * 2 : 0);
}

template <int KS>
__global__ __launch_bounds__(HL_THREADS) void head_loss_k(HeadLoss p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hl_sm[];
    __shared__ double wsum[HL_WAVES];
    const int P = p.H * p.W, Q = p.OH * p.OW;
    float* Ys = (float*)hl_sm;                                                   // [P][HL_LD] tap values
    float* dls = (float*)(hl_sm + ((((size_t)P * HL_LD * 4) + 15) & ~(size_t)15));   // [Q] logit gradient as stored (bf16 -> fp32)
    bf16_t* wt = (bf16_t*)((unsigned char*)dls + ((((size_t)Q * 4) + 15) & ~(size_t)15));   // [16][C]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    int n, rg;
    if (p.xcd) {
        n = (blockIdx.x & 7) + 8 * (blockIdx.x / (8 * p.rg));
        rg = (blockIdx.x >> 3) % p.rg;
    } else {
        n = blockIdx.x / p.rg;
        rg = blockIdx.x - n * p.rg;
    }
    const bool first = n < p.n_first;
    const float tconst = first ? p.t_first : p.t_rest;
    const float gscale = first ? p.gs_first : p.gs_rest;

    if (p.du) {      // the transposed filter of head_dgrad_k
        for (int i = tid; i < p.C * 16; i += HL_THREADS) {
            const int c = i >> 4, t = i & 15;
            wt[t * p.C + c] = p.wd[i];
        }
    }
    // ---- Y[pix][tap] = sum_c W[tap][c] * a3[pix][c]: the fragments and K order of thin_dgrad_gemm_k<1, KS> ----
    bf8_t af[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) af[s] = *(const bf8_t*)(p.wf + (size_t)fr * p.C + 32 * s + 8 * fq);
    const bf16_t* x = p.a3 + (size_t)n * P * p.C;
    for (int p0 = wid * 16; p0 < P; p0 += HL_WAVES * 16) {
        const int m = min(p0 + fr, P - 1);
        bf8_t bfr[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) bfr[s] = *(const bf8_t*)(x + (size_t)m * p.C + 32 * s + 8 * fq);
        f4_t acc = (f4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s], bfr[s], acc, 0, 0, 0);
        if (p0 + fr < P) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Ys[(p0 + fr) * HL_LD + 4 * fq + r] = acc[r];
        }
    }
    __syncthreads();
    // ---- logits (thin_col2im_k: from 0, taps in table order, out-of-image taps skipped), loss and logit gradient ----
    double lsum = 0.0;
    for (int i = tid; i < Q; i += HL_THREADS) {
        const int oy = i / p.OW, ox = i - oy * p.OW;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int iy = oy + (k >> 2) - 1, ix = ox + (k & 3) - 1;
            if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) v += Ys[(iy * p.W + ix) * HL_LD + k];
        }
        const float xv = v;
        // loss_k<L_BCE>: max(x,0) - x*t + log1p(exp(-|x|));  d/dx = sigmoid(x) - t
        const float l = fmaxf(xv, 0.f) - xv * tconst + log1pf(expf(-fabsf(xv)));
        const float g = 1.f / (1.f + expf(-xv)) - tconst;
        const float gs = g * gscale;
        const bf16_t gb = f2bf(gs);
        dls[i] = bf2f(gb);
        lsum += (double)l;
        if (rg == 0) {
            const size_t o = (size_t)n * Q + i;
            p.logits[o] = xv;
            if (p.dl) p.dl[o] = gb;
            if (p.dl32) p.dl32[o] = gs;
        }
    }
    if (rg == 0) {       // (uniform over the workgroup) one fp64 atomic per image
        double v = lsum * (first ? p.ls_first : p.ls_rest);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) wsum[wid] = v;
    }
    __syncthreads();
    if (rg == 0 && tid == 0) {
        double v = wsum[0];
#pragma unroll
        for (int w = 1; w < HL_WAVES; ++w) v += wsum[w];
        // The images' atomics arrive in any order, and the per-image values are sums of fp32 terms over a small count: their
        // exact total lands ON a rounding boundary of the fp32 loss once in a few dozen steps, where the last bit of an fp64
        // sum that depends on the order decides -- two runs from one state then log losses one ulp apart.  Rounded to a
        // multiple of 2^-36 (7e-12, 1e-9 over 128 images against an fp32 ulp of 1e-7 at a loss of 1) every addition is EXACT
        // (|v| < 2^8, up to 2^9 images: 53 bits), so the sum is the same in every order.  Larger values are added as they are.
        if (fabs(v) < 256.0) v = rint(v * 0x1p36) * 0x1p-36;
        atomicAdd(p.loss, v);
    }
    if (!p.du) return;
    // ---- du[pix][c] = bf16(sum_taps dl * w) * act'(a3[pix][c]): the loop and rounding of head_dgrad_k ----
    const int r0 = (p.H * rg) / p.rg, r1 = (p.H * (rg + 1)) / p.rg;
    const int groups = p.C / 8;
    const int items = (r1 - r0) * p.W * groups;
    for (int item = tid; item < items; item += HL_THREADS) {
        const int pix = item / groups, cg = item - pix * groups;
        const int ry = pix / p.W, ox = pix - ry * p.W, oy = r0 + ry;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int sy = oy + 1 - (t >> 2), sx = ox + 1 - (t & 3);
            if ((unsigned)sy >= (unsigned)p.OH || (unsigned)sx >= (unsigned)p.OW) continue;
            const float v = dls[sy * p.OW + sx];
            float wv[8];
            V8<bf16_t>::ld(wt + t * p.C + cg * 8, wv);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf(v, wv[j], acc[j]);
        }
        const size_t o = ((size_t)n * P + (size_t)oy * p.W + ox) * p.C + cg * 8;
        float zv[8];
        V8<bf16_t>::ld(p.act_src + o, zv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float gq = bf2f(f2bf(acc[j]));
            acc[j] = p.act == PAI_ACT_NONE ? gq : gq * act_grad(zv[j], p.act);
        }
        V8<bf16_t>::st(p.du + o, acc);
    }
}

// The shapes the launch takes: the bias-free bf16 k4 s1 p1 convolution to ONE channel whose forward is thin_dgrad_gemm_k +
// thin_col2im_k and whose input gradient is head_dgrad_k, with the image's tap values, logit gradient and transposed filter
// in LDS.  Everything else keeps those launches.
static bool head_loss_shape_ok(const pai_conv_desc* d, int has_bias) {
    if (!d || has_bias || d->dtype != PAI_BF16 || d->transposed || d->kernel != 4 || d->stride != 1 || d->pad != 1) return false;
    if (d->Cout != 1 || d->C2 != 0 || d->relu1 || d->epilogue_act != PAI_ACT_NONE || d->groups > 1) return false;
    if (d->N <= 0 || d->H < 2 || d->W < 2 || (d->C1 % 32) != 0) return false;
    const int ks = d->C1 / 32;
    if (!(ks == 1 || ks == 2 || ks == 4 || ks == 8 || ks == 16)) return false;
    return head_loss_lds_bytes(d->H, d->W, d->C1, true) <= HL_LDS_MAX;
}

extern "C" int pai_head_loss_ok(const pai_conv_desc* d, int has_bias) {
    return pai_tunable("head_fused", 1) && head_loss_shape_ok(d, has_bias) ? 1 : 0;
}

extern "C" int pai_head_loss(const pai_conv_desc* d, const void* a3, const void* w_fwd, const void* w_dgrad, int n_first,
                             float target_first, float target_rest, float loss_scale, double* loss, float grad_scale,
                             float* logits, void* dl, float* dl_f32, void* du, const void* act_src, int act, void* stream) {
    PAI_CHECK(head_loss_shape_ok(d, 0), "pai_head_loss: not a bias-free bf16 k4 s1 p1 C -> 1 head within the LDS bound (ask pai_head_loss_ok)");
    PAI_CHECK(a3 && w_fwd && loss && logits, "pai_head_loss: null pointer");
    PAI_CHECK(!du || (w_dgrad && act_src), "pai_head_loss: du needs w_dgrad and act_src");
    PAI_CHECK(act == PAI_ACT_LRELU || act == PAI_ACT_RELU || act == PAI_ACT_NONE, "pai_head_loss: act=%d", act);
    HeadLoss p;
    memset(&p, 0, sizeof(p));
    p.a3 = (const bf16_t*)a3; p.wf = (const bf16_t*)w_fwd; p.wd = (const bf16_t*)w_dgrad;
    p.logits = logits; p.dl = (bf16_t*)dl; p.dl32 = dl_f32; p.du = (bf16_t*)du; p.act_src = (const bf16_t*)act_src;
    p.loss = loss;
    p.N = d->N; p.H = d->H; p.W = d->W; p.C = d->C1; p.OH = d->H - 1; p.OW = d->W - 1;
    p.n_first = n_first < 0 ? 0 : (n_first > d->N ? d->N : n_first);
    p.t_first = target_first; p.t_rest = target_rest;
    const int64_t per = (int64_t)p.OH * p.OW, nf = per * p.n_first, nr = per * (p.N - p.n_first);
    // (launch_loss: loss_scale / numel in fp64, grad_scale / numel rounded to fp32)
    if (nf > 0) { p.ls_first = (double)loss_scale / (double)nf; p.gs_first = (float)((double)grad_scale / (double)nf); }
    if (nr > 0) { p.ls_rest = (double)loss_scale / (double)nr; p.gs_rest = (float)((double)grad_scale / (double)nr); }
    p.act = act;
    // Geometry: one workgroup per image leaves the store stream of du on 64-128 of the 256 CUs; rg workgroups per image
    // each recompute the image's logits (its 256 KB come from L2 when the rg workgroups share an XCD) and store H / rg rows.
    int rg = du ? pai_tunable("head_loss_rg", 4) : 1;
    if (rg < 1) rg = 1;
    if (rg > p.H) rg = p.H;
    p.rg = rg;
    p.xcd = (p.N % 8) == 0 ? 1 : 0;
    const size_t lds = (size_t)head_loss_lds_bytes(p.H, p.W, p.C, du != nullptr);
    const dim3 grid((unsigned)(p.N * rg));
    hipStream_t s = (hipStream_t)stream;
#define HL_CASE(KK)                                                                                                     \
    case KK: {                                                                                                          \
        static PerDeviceOnce attr;                                                                                      \
        if (attr.first()) {                                                                                             \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&head_loss_k<KK>),                   \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)HL_LDS_MAX);      \
            PAI_CHECK(e == hipSuccess, "pai_head_loss: hipFuncSetAttribute(max dynamic LDS): %s", hipGetErrorString(e)); \
        }                                                                                                               \
        PAI_LAUNCH(head_loss_k<KK>, grid, dim3(HL_THREADS), lds, s, p);                                                 \
        break;                                                                                                          \
    }
    switch (p.C / 32) {
        HL_CASE(1) HL_CASE(2) HL_CASE(4) HL_CASE(8) HL_CASE(16)
        default: PAI_CHECK(false, "pai_head_loss: unsupported C %d", p.C);
    }
#undef HL_CASE
    PAI_LAUNCH_CHECK();
    return 0;
}
