// The SSIM tile body and the fixed-order sum of the tile partials, shared by ssim.hip (hmm_ssim_pairs) and extract_walk.hip
// (hmm_extract_walk): one definition of the arithmetic, so a candidate scored inside the walk has the bits of the same pair scored
// by hmm_ssim_pairs.  See ssim.hip for the contract (skimage 0.18.3 structural_similarity, exact int32 box sums, fp64 in numpy's
// operation order with contraction off).
#pragma once
#include "hmm_common.h"

#pragma clang fp contract(off)

namespace hmm {

constexpr int kSsimTW = 256;                      // output columns of a tile: one per thread
constexpr int kSsimTH = 36;                       // output rows of a tile: TH + 6 = 42 input rows = 6 turns of the 7-row ring
constexpr int kSsimIn = kSsimTH + 6;
constexpr int kSsimLdsW = kSsimTW + 8;            // 262 staged bytes per row, padded
constexpr int kFinishThreads = 256;

struct SsimTileLds {
    uint8_t a[kSsimIn][kSsimLdsW];
    uint8_t b[kSsimIn][kSsimLdsW];
    double wave[kSsimTW / kWave];
};

inline int ssim_tiles(int H, int W, int* tiles_x) {
    const int tx = (W - 6 + kSsimTW - 1) / kSsimTW, ty = (H - 6 + kSsimTH - 1) / kSsimTH;
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

// One workgroup of kSsimTW threads, one tile of 256 x 36 output positions whose top-left window is (x0, y0).  Both frames'
// (36 + 6) x (256 + 6) input block is staged in LDS; each thread owns one output column and walks down it: the five horizontal
// 7-sums of every input row go through a 7-deep ring in registers (the loop over a turn of the ring is unrolled, so the ring is
// indexed by constants), and the vertical sums slide by adding the new row and subtracting the one that left.  Output (ox, oy) is
// the window whose top-left pixel is (ox, oy).  A plays skimage's im1.  Thread 0 stores the tile's sum of S to *partial_out.
__device__ __forceinline__ void ssim_tile_partial(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, int H, int W,
                                                  int x0, int y0, double R, SsimTileLds& s, double* __restrict__ partial_out) {
    for (int i = threadIdx.x; i < kSsimIn * (kSsimTW + 6); i += kSsimTW) {
        const int r = i / (kSsimTW + 6), c = i % (kSsimTW + 6);
        const int y = y0 + r, x = x0 + c;
        const bool in = y < H && x < W;
        const int64_t o = (int64_t)y * W + x;
        s.a[r][c] = in ? A[o] : 0;
        s.b[r][c] = in ? B[o] : 0;
    }
    __syncthreads();

    const double k1r = 0.01 * R, k2r = 0.03 * R;
    const double C1 = k1r * k1r, C2 = k2r * k2r;
    const double cov_norm = 49.0 / 48.0;

    const int tx = threadIdx.x;
    const bool col_ok = x0 + tx < W - 6;
    const int rows_out = min(kSsimTH, H - 6 - y0);
    int ring[7][5] = {};
    int vx = 0, vy = 0, vxx = 0, vyy = 0, vxy = 0;
    double acc = 0.0;
    for (int r0 = 0; r0 < kSsimIn; r0 += 7) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int r = r0 + k;
            int hx = 0, hy = 0, hxx = 0, hyy = 0, hxy = 0;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int a = s.a[r][tx + j], b = s.b[r][tx + j];
                hx += a;
                hy += b;
                hxx += a * a;
                hyy += b * b;
                hxy += a * b;
            }
            vx += hx - ring[k][0];
            vy += hy - ring[k][1];
            vxx += hxx - ring[k][2];
            vyy += hyy - ring[k][3];
            vxy += hxy - ring[k][4];
            ring[k][0] = hx;
            ring[k][1] = hy;
            ring[k][2] = hxx;
            ring[k][3] = hyy;
            ring[k][4] = hxy;
            if (r >= 6 && r - 6 < rows_out && col_ok) {
                const double ux = (double)vx / 49.0, uy = (double)vy / 49.0;
                const double uxx = (double)vxx / 49.0, uyy = (double)vyy / 49.0, uxy = (double)vxy / 49.0;
                const double sx = cov_norm * (uxx - ux * ux);
                const double sy = cov_norm * (uyy - uy * uy);
                const double sxy = cov_norm * (uxy - ux * uy);
                const double a1 = 2.0 * ux * uy + C1, a2 = 2.0 * sxy + C2;
                const double b1 = ux * ux + uy * uy + C1, b2 = sx + sy + C2;
                acc += (a1 * a2) / (b1 * b2);
            }
        }
    }
    acc = wave_sum(acc);
    if ((tx & (kWave - 1)) == 0) s.wave[tx / kWave] = acc;
    __syncthreads();
    if (tx == 0) {
        double t = s.wave[0];
#pragma unroll
        for (int i = 1; i < kSsimTW / kWave; ++i) t += s.wave[i];
        *partial_out = t;
    }
}

// The sum of one pair's n_tiles partials in a fixed order, by one workgroup of kFinishThreads threads: the threads strided over
// the tiles, then the wave sum, then the waves in index order.  The value is returned in thread 0 (other threads: unspecified).
__device__ __forceinline__ double ssim_partials_sum(const double* __restrict__ p, int n_tiles, double* s_wave) {
    double acc = 0.0;
    for (int t = threadIdx.x; t < n_tiles; t += kFinishThreads) acc += p[t];
    acc = wave_sum(acc);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = acc;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        s = s_wave[0];
#pragma unroll
        for (int i = 1; i < kFinishThreads / kWave; ++i) s += s_wave[i];
    }
    return s;
}

}  // namespace hmm
