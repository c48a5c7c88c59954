// Report evaluation on the device (reference report.py:78-96,188-233: per-image SSIM / PSNR / MSE, the SSIM over 16 depth
// strips, the SSIM map and the afmhot rendering of every prediction as 8-bit images -- there torchmetrics calls per image
// and strip, then matplotlib and torchvision on the host).
//
//   pai_eval_planes   one pass over an image pair: per-plane SSIM mean and squared error (fp64), the SSIM map as
//                     to_int(clamp(S, 0, 1)) and the prediction through a 256-entry RGB table, both as bytes.  The kernel
//                     (eval_planes_k) lives in ssim.hip beside ssim_k, whose tile stages it runs: the per-pixel S is the
//                     same bits as pai_ssim_sse's full_map.
//   Depth strips need no kernel of their own: a contiguous [N, C, H, W] tensor with H % 16 == 0 is [N*C*16, H/16, W].
#include "common.h"

extern "C" int pai_eval_planes(const float* pred, const float* target, int NC, int H, int W, int denorm, double* ssim_plane,
                               double* sse_plane, unsigned char* ssim_map_u8, const unsigned char* lut_rgb,
                               unsigned char* hot_u8, void* stream) {
    PAI_CHECK(pred && target && (ssim_plane || sse_plane || ssim_map_u8 || hot_u8), "pai_eval_planes: null pointer");
    PAI_CHECK(NC >= 0 && NC <= 65535, "pai_eval_planes: at most 65535 planes per call (got %d)", NC);
    PAI_CHECK(H > 10 && W > 10, "pai_eval_planes: image %dx%d smaller than the 11x11 window", H, W);
    PAI_CHECK((int64_t)NC * H * W * 3 <= INT64_MAX / 4 && (int64_t)H * W <= INT32_MAX, "pai_eval_planes: plane too large");
    PAI_CHECK(!hot_u8 || lut_rgb, "pai_eval_planes: hot_u8 needs the 256 x 3 byte table");
    PAI_CHECK(((((uintptr_t)ssim_map_u8) | ((uintptr_t)hot_u8)) & 3) == 0, "pai_eval_planes: 4-byte aligned byte outputs expected");
    if (NC == 0) return 0;
    return launch_eval_planes(pred, target, NC, H, W, denorm, ssim_plane, sse_plane, ssim_map_u8, lut_rgb, hot_u8,
                              (hipStream_t)stream);
}

extern "C" int pai_eval_kernel_name(int op, char* name, int name_len) {
    PAI_CHECK(name && name_len > 0, "pai_eval_kernel_name: bad arguments");
    PAI_CHECK(op == 0, "pai_eval_kernel_name: op %d (0 pai_eval_planes)", op);
    snprintf(name, (size_t)name_len, "%s", eval_planes_kernel_name());
    return 0;
}
