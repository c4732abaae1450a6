// SSIM of gray frames on gfx950: the arithmetic of skimage 0.18.3 structural_similarity with its defaults (7x7 uniform window,
// sample covariance 49/48, K1 = 0.01, K2 = 0.03, mean over S cropped by 3 pixels on every side), as the reference calls it at
// hippomm/core/batch_process.py:32-69 (compute_frame_difference) and hippomm/core/hippocampal_memory.py:980-991
// (_compute_frame_similarity, consulted by _segment_sequence :1002-1114).
//
// Only the (H-6) x (W-6) window positions that lie inside the image count (the crop removes every position scipy's reflect border
// reaches), so no border rule is needed.  The five 7x7 box sums are exact int32 (the largest, 49 * 255^2 = 3 186 225); the rest is
// fp64 in numpy's operation order, with contraction off, so every S is the value the numpy restatement (tests/ssim_oracle.py) has.
// The mean is a fixed-order fp64 sum: per-workgroup partials, then one small kernel per pair.  No float atomics: a pair's score
// does not depend on the run or on the batch it was computed in.
//
// Gray conversion is OpenCV's 8-bit BGR2GRAY rule (CV_DESCALE with yuv_shift 14): g = (1868 B + 9617 G + 4899 R + 8192) >> 14.
#include "hmm_common.h"
#include "ssim_core.h"

#pragma clang fp contract(off)

namespace hmm {

constexpr int kGrayThreads = 256;
constexpr int kGrayBlocksPerFrame = 512;          // grid-stride inside a frame: at most 512 x 2 atomics per frame

constexpr int kSsimChunk = 128;                   // pairs per launch, carried in the kernel arguments (1 KiB)

struct PairChunk {
    int32_t a[kSsimChunk];
    int32_t b[kSsimChunk];
};

__global__ __launch_bounds__(256) void gray_minmax_init_kernel(int32_t* __restrict__ minmax, int n) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n) {
        minmax[2 * f] = 255;
        minmax[2 * f + 1] = 0;
    }
}

// frames (n, hw, C) u8 -> gray (n, hw) u8 and per-frame (min, max).  C = 3: byte order R,G,B (bgr = 0) or B,G,R (bgr = 1); C = 1:
// the frames are gray already and only min / max are taken.  blockIdx.y = frame.
template <int C>
__global__ __launch_bounds__(kGrayThreads) void gray_kernel(const uint8_t* __restrict__ frames, int64_t hw, int bgr,
                                                             uint8_t* __restrict__ gray, int32_t* __restrict__ minmax) {
    __shared__ int32_t s_min[kGrayThreads / kWave], s_max[kGrayThreads / kWave];
    const int f = blockIdx.y;
    const uint8_t* src = frames + (int64_t)f * hw * C;
    uint8_t* dst = (C == 3) ? gray + (int64_t)f * hw : nullptr;
    int lo = 255, hi = 0;
    for (int64_t p = (int64_t)blockIdx.x * kGrayThreads + threadIdx.x; p < hw; p += (int64_t)gridDim.x * kGrayThreads) {
        int g;
        if constexpr (C == 3) {
            const int c0 = src[3 * p], c1 = src[3 * p + 1], c2 = src[3 * p + 2];
            const int r = bgr ? c2 : c0, b = bgr ? c0 : c2;
            g = (1868 * b + 9617 * c1 + 4899 * r + 8192) >> 14;
            dst[p] = (uint8_t)g;
        } else {
            g = src[p];
        }
        lo = min(lo, g);
        hi = max(hi, g);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_min[w] = lo;
        s_max[w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < kGrayThreads / kWave; ++i) {
            lo = min(lo, s_min[i]);
            hi = max(hi, s_max[i]);
        }
        atomicMin(&minmax[2 * f], lo);
        atomicMax(&minmax[2 * f + 1], hi);
    }
}

// One workgroup per (pair, tile of 256 x 36 output positions): the tile body is ssim_tile_partial (ssim_core.h).
__global__ __launch_bounds__(kSsimTW) void ssim_tile_kernel(const uint8_t* __restrict__ gray, int H, int W, PairChunk pairs,
                                                            int pair0, int range_from_a, double data_range,
                                                            const int32_t* __restrict__ minmax, int tiles_x, int n_tiles,
                                                            double* __restrict__ partial) {
    __shared__ SsimTileLds s;
    const int tile = blockIdx.x;
    const int x0 = (tile % tiles_x) * kSsimTW, y0 = (tile / tiles_x) * kSsimTH;
    const int ia = pairs.a[blockIdx.y], ib = pairs.b[blockIdx.y];
    const int64_t hw = (int64_t)H * W;
    double R = data_range;
    if (range_from_a) R = (double)(minmax[2 * ia + 1] - minmax[2 * ia]);
    ssim_tile_partial(gray + ia * hw, gray + ib * hw, H, W, x0, y0, R, s,
                      partial + (int64_t)(pair0 + blockIdx.y) * n_tiles + tile);
}

// score[p] = (sum of pair p's tile partials, in a fixed order: ssim_partials_sum) / count.  blockIdx.x = pair.
__global__ __launch_bounds__(kFinishThreads) void ssim_finish_kernel(const double* __restrict__ partial, int n_tiles, double count,
                                                                     double* __restrict__ scores) {
    __shared__ double s_wave[kFinishThreads / kWave];
    const double s = ssim_partials_sum(partial + (int64_t)blockIdx.x * n_tiles, n_tiles, s_wave);
    if (threadIdx.x == 0) scores[blockIdx.x] = s / count;
}

}  // namespace hmm

using namespace hmm;

extern "C" int hmm_gray_u8(const uint8_t* frames_dev, int n, int H, int W, int channel_order, uint8_t* gray_out_dev,
                           int32_t* minmax_out_dev, hmm_stream_t stream) {
    HMM_REQUIRE(frames_dev && minmax_out_dev, HMM_E_INVALID, "gray_u8: null pointer");
    HMM_REQUIRE(channel_order == HMM_GRAY_FROM_RGB || channel_order == HMM_GRAY_FROM_BGR || channel_order == HMM_GRAY_FROM_GRAY,
                HMM_E_INVALID, "gray_u8: unknown channel_order %d", channel_order);
    HMM_REQUIRE(channel_order == HMM_GRAY_FROM_GRAY || gray_out_dev, HMM_E_INVALID, "gray_u8: null gray output");
    HMM_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1, HMM_E_INVALID, "gray_u8: bad shape n=%d H=%d W=%d", n, H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    gray_minmax_init_kernel<<<(n + 255) / 256, 256, 0, st>>>(minmax_out_dev, n);
    HMM_LAUNCH_CHECK();
    const int64_t hw = (int64_t)H * W;
    const dim3 grid((unsigned)std::min<int64_t>((hw + kGrayThreads - 1) / kGrayThreads, kGrayBlocksPerFrame), (unsigned)n);
    if (channel_order == HMM_GRAY_FROM_GRAY)
        gray_kernel<1><<<grid, kGrayThreads, 0, st>>>(frames_dev, hw, 0, nullptr, minmax_out_dev);
    else
        gray_kernel<3><<<grid, kGrayThreads, 0, st>>>(frames_dev, hw, channel_order == HMM_GRAY_FROM_BGR, gray_out_dev,
                                                      minmax_out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" size_t hmm_ssim_pairs_workspace_bytes(int H, int W, int n_pairs) {
    if (H < 7 || W < 7 || n_pairs < 1) return 0;
    return align_up((size_t)n_pairs * ssim_tiles(H, W, nullptr) * sizeof(double), 256);
}

extern "C" int hmm_ssim_pairs(const uint8_t* gray_dev, int n_frames, int H, int W, const int32_t* pairs_host, int n_pairs,
                              double data_range, const int32_t* minmax_dev, double* scores_out_dev, void* workspace_dev,
                              size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(gray_dev && pairs_host && scores_out_dev && workspace_dev, HMM_E_INVALID, "ssim_pairs: null pointer");
    HMM_REQUIRE(n_frames >= 1 && n_pairs >= 1, HMM_E_INVALID, "ssim_pairs: n_frames=%d n_pairs=%d, both must be >= 1", n_frames,
                n_pairs);
    HMM_REQUIRE(H >= 7 && W >= 7, HMM_E_INVALID, "ssim_pairs: win_size exceeds image extent (%dx%d frames, 7x7 window)", H, W);
    HMM_REQUIRE(n_pairs <= 65535 * kSsimChunk, HMM_E_INVALID, "ssim_pairs: %d pairs in one call is too many", n_pairs);
    const bool from_a = data_range < 0.0;
    HMM_REQUIRE(!from_a || minmax_dev, HMM_E_INVALID, "ssim_pairs: data_range < 0 (range of frame a) needs minmax_dev");
    HMM_REQUIRE(data_range == data_range, HMM_E_INVALID, "ssim_pairs: data_range is NaN");
    for (int p = 0; p < n_pairs; ++p) {
        const int a = pairs_host[2 * p], b = pairs_host[2 * p + 1];
        HMM_REQUIRE(0 <= a && a < n_frames && 0 <= b && b < n_frames, HMM_E_INVALID,
                    "ssim_pairs: pair %d = (%d, %d) outside the %d frames", p, a, b, n_frames);
    }
    HMM_REQUIRE(workspace_bytes >= hmm_ssim_pairs_workspace_bytes(H, W, n_pairs), HMM_E_WORKSPACE,
                "ssim_pairs: workspace of %zu bytes, %zu needed", workspace_bytes, hmm_ssim_pairs_workspace_bytes(H, W, n_pairs));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int tiles_x = 0;
    const int n_tiles = ssim_tiles(H, W, &tiles_x);
    double* partial = static_cast<double*>(workspace_dev);
    for (int p0 = 0; p0 < n_pairs; p0 += kSsimChunk) {
        const int m = std::min(kSsimChunk, n_pairs - p0);
        PairChunk chunk = {};
        for (int i = 0; i < m; ++i) {
            chunk.a[i] = pairs_host[2 * (p0 + i)];
            chunk.b[i] = pairs_host[2 * (p0 + i) + 1];
        }
        ssim_tile_kernel<<<dim3((unsigned)n_tiles, (unsigned)m), kSsimTW, 0, st>>>(gray_dev, H, W, chunk, p0, from_a ? 1 : 0,
                                                                                   data_range, minmax_dev, tiles_x, n_tiles,
                                                                                   partial);
        HMM_LAUNCH_CHECK();
    }
    ssim_finish_kernel<<<(unsigned)n_pairs, kFinishThreads, 0, st>>>(partial, n_tiles, (double)(H - 6) * (double)(W - 6),
                                                                     scores_out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
