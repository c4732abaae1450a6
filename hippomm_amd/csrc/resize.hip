// cv2.resize of 8-bit frames on gfx950, for targets no larger than the source: the arithmetic of OpenCV's INTER_LINEAR for uchar
// (modules/imgproc/src/resize.cpp: INTER_RESIZE_COEF_BITS = 11, HResizeLinear, VResizeLinear<uchar, int, short,
// FixedPtCast<int, uchar, 22>>) and of the 2 x 2 area path OpenCV takes instead when both scales are exactly 2
// (ResizeAreaFastVec), as the reference calls it on every recalled frame (hippomm/core/hippocampal_memory.py:2232, :2795:
// cv2.resize(frame, (320, 180))).  Restated from the published source; a build that routes 8-bit resize through another
// back end may differ.
//
//   horizontal   h = S[sx] * a0 + S[sx + 1] * a1                     int32; S[sx] * 2048 where sx + 1 would leave the row
//   vertical     d = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
//   area 2 x 2   d = (s00 + s01 + s10 + s11 + 2) >> 2
//
// The offsets and the 11-bit coefficient pairs are tables the caller builds on the host (segmentation.resize_linear_tables) and
// keeps in device memory.  One launch for all frames of a call, one thread per output pixel (all its channels); at
// 1080p -> 180p a launch reads a third of the source lines and is bound by the launch itself, so batching is the point.  No LDS,
// no scratch.  Offsets are clamped to the frame, so a wrong table gives wrong pixels and never a read outside src.
#include "hmm_common.h"

namespace hmm {

constexpr int kResizeThreads = 256;
constexpr int kResizeOne = 1 << 11;               // INTER_RESIZE_COEF_SCALE

// blockIdx.y = frame, blockIdx.x * 256 + threadIdx.x = output pixel of that frame.
template <int C, int MODE>
__global__ __launch_bounds__(kResizeThreads) void resize_u8_kernel(const uint8_t* __restrict__ src, int src_h, int src_w,
                                                                    uint8_t* __restrict__ dst, int dst_h, int dst_w,
                                                                    const int32_t* __restrict__ xofs, const int16_t* __restrict__ xcoef,
                                                                    const int32_t* __restrict__ yofs, const int16_t* __restrict__ ycoef) {
    const int p = blockIdx.x * kResizeThreads + threadIdx.x;
    if (p >= dst_h * dst_w) return;
    const int dy = p / dst_w, dx = p - dy * dst_w;
    const uint8_t* S = src + (int64_t)blockIdx.y * src_h * src_w * C;
    uint8_t* D = dst + ((int64_t)blockIdx.y * dst_h * dst_w + p) * C;
    if constexpr (MODE == HMM_RESIZE_AREA2X) {
        const uint8_t* r0 = S + ((int64_t)(2 * dy) * src_w + 2 * dx) * C;
        const uint8_t* r1 = r0 + (int64_t)src_w * C;
#pragma unroll
        for (int c = 0; c < C; ++c) D[c] = (uint8_t)((r0[c] + r0[C + c] + r1[c] + r1[C + c] + 2) >> 2);
    } else {
        const int sx = min(max(xofs[dx], 0), src_w - 1), sy = min(max(yofs[dy], 0), src_h - 1);
        const bool edge = sx + 1 >= src_w;
        const int a0 = edge ? kResizeOne : xcoef[2 * dx], a1 = edge ? 0 : xcoef[2 * dx + 1];
        const int b0 = ycoef[2 * dy], b1 = ycoef[2 * dy + 1];
        const int step = edge ? 0 : C;                                    // S[sx] stands in for S[sx + 1]: its weight is 0
        const uint8_t* r0 = S + ((int64_t)sy * src_w + sx) * C;
        const uint8_t* r1 = S + ((int64_t)min(sy + 1, src_h - 1) * src_w + sx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int h0 = r0[c] * a0 + r0[step + c] * a1;
            const int h1 = r1[c] * a0 + r1[step + c] * a1;
            D[c] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

}  // namespace hmm

using namespace hmm;

extern "C" int hmm_resize_linear_u8(const uint8_t* src_dev, int n, int src_h, int src_w, int channels, uint8_t* dst_dev, int dst_h,
                                    int dst_w, const int32_t* xofs_dev, const int16_t* xcoef_dev, const int32_t* yofs_dev,
                                    const int16_t* ycoef_dev, int mode, hmm_stream_t stream) {
    HMM_REQUIRE(mode == HMM_RESIZE_LINEAR || mode == HMM_RESIZE_AREA2X, HMM_E_INVALID, "resize_linear_u8: unknown mode %d", mode);
    HMM_REQUIRE(channels == 1 || channels == 3, HMM_E_INVALID, "resize_linear_u8: channels must be 1 or 3, got %d", channels);
    HMM_REQUIRE(n >= 0 && n <= 65535, HMM_E_INVALID, "resize_linear_u8: n=%d outside 0..65535", n);
    HMM_REQUIRE(src_h >= 1 && src_w >= 1 && dst_h >= 1 && dst_w >= 1 && src_h <= 65535 && src_w <= 65535, HMM_E_INVALID,
                "resize_linear_u8: bad shape %dx%d -> %dx%d (sides of 1..65535)", src_h, src_w, dst_h, dst_w);
    HMM_REQUIRE((int64_t)dst_h * dst_w <= (int64_t)1 << 30, HMM_E_INVALID, "resize_linear_u8: a target of %dx%d pixels is too large",
                dst_h, dst_w);
    HMM_REQUIRE(dst_h <= src_h && dst_w <= src_w, HMM_E_INVALID,
                "resize_linear_u8: %dx%d -> %dx%d enlarges an axis; only targets no larger than the source are built", src_h, src_w,
                dst_h, dst_w);
    HMM_REQUIRE(mode != HMM_RESIZE_AREA2X || (src_h == 2 * dst_h && src_w == 2 * dst_w), HMM_E_INVALID,
                "resize_linear_u8: area2x mode needs a source of exactly twice the target, got %dx%d -> %dx%d", src_h, src_w, dst_h,
                dst_w);
    if (n == 0) return HMM_OK;
    HMM_REQUIRE(src_dev && dst_dev, HMM_E_INVALID, "resize_linear_u8: null pointer (src or dst)");
    if (mode == HMM_RESIZE_LINEAR) {
        HMM_REQUIRE(xofs_dev && xcoef_dev && yofs_dev && ycoef_dev, HMM_E_INVALID, "resize_linear_u8: null pointer (tables)");
        HMM_REQUIRE(((uintptr_t)xofs_dev | (uintptr_t)yofs_dev) % 4 == 0 && ((uintptr_t)xcoef_dev | (uintptr_t)ycoef_dev) % 2 == 0,
                    HMM_E_INVALID, "resize_linear_u8: tables not aligned (offsets to 4 bytes, coefficients to 2)");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((dst_h * dst_w + kResizeThreads - 1) / kResizeThreads), (unsigned)n);
#define HMM_RESIZE_LAUNCH(C, MODE)                                                                                               \
    resize_u8_kernel<C, MODE><<<grid, kResizeThreads, 0, st>>>(src_dev, src_h, src_w, dst_dev, dst_h, dst_w, xofs_dev, xcoef_dev, \
                                                               yofs_dev, ycoef_dev)
    if (mode == HMM_RESIZE_AREA2X) {
        if (channels == 3) HMM_RESIZE_LAUNCH(3, HMM_RESIZE_AREA2X); else HMM_RESIZE_LAUNCH(1, HMM_RESIZE_AREA2X);
    } else {
        if (channels == 3) HMM_RESIZE_LAUNCH(3, HMM_RESIZE_LINEAR); else HMM_RESIZE_LAUNCH(1, HMM_RESIZE_LINEAR);
    }
#undef HMM_RESIZE_LAUNCH
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
