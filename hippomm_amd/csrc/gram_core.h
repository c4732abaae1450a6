// The 64 x 64 x 1024 gram tile behind both consolidation routes of gram_select.hip: gram_bits_kernel (the one-shot relation of a
// finished matrix, and the new rows of a batch against each other) and keyframe_kept_bits_kernel (new rows against the kept rows
// of a growing selection).  One mainloop, so that a pair of rows gets the same bits whichever kernel evaluates it: K slabs of 32
// staged through LDS, v_mfma_f64_16x16x4_f64 in ascending k, every dot accumulated in fp64; the caller rounds (float)acc once
// and compares.
//
// Which operand a row sits in cannot change a bit either: the product of two fp32 values is exact in fp64 and commutes, the
// k order of the sum is the same for every output element, and an element depends on its own A row and B row alone.
#pragma once
#include "hmm_common.h"

namespace hmm {

constexpr int kGT = 64;        // gram tile edge
constexpr int kGK = 32;        // k-slab staged per step
constexpr int kGLd = kGK + 2;  // LDS row stride in floats: bank = 2*row + k -> conflict-free column reads

// One block of 256 threads = 4 waves, each a 32x32 quadrant = 2x2 MFMA blocks of 16x16 (v_mfma_f64_16x16x4_f64:
// A[l&15][k=l>>4], B[k=l>>4][l&15], D col = l&15, row = (l>>4) + 4*reg).  Thread t stages rows (t>>3) and (t>>3)+32 of each
// operand: a0 / a1 and b0 / b1 point at those rows' first element (the caller clamps them into memory it owns).
// acc[a][b][reg] is the dot of A row  qr + 16 a + (lane>>4) + 4 reg  with B row  qc + 16 b + (lane&15),
// qr = (wave>>1)*32, qc = (wave&1)*32.  sa / sb: kGT * kGLd floats of LDS each.
__device__ __forceinline__ void gram_tile_mainloop(const float* __restrict__ a0, const float* __restrict__ a1,
                                                   const float* __restrict__ b0, const float* __restrict__ b1,
                                                   float* __restrict__ sa, float* __restrict__ sb, f64x4 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qr = (w >> 1) * 32, qc = (w & 1) * 32;      // quadrant origin inside the tile
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

    // staging: 64 rows x 32 floats per operand = 512 float4; 256 threads x 2
    const int srow = tid >> 3, scol = (tid & 7) * 4;
    const float* ga[2] = {a0, a1};
    const float* gb[2] = {b0, b1};

    for (int k0 = 0; k0 < HMM_FEATURE_DIM; k0 += kGK) {
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = srow + h * 32;
            const float4 va = *reinterpret_cast<const float4*>(ga[h] + k0 + scol);
            const float4 vb = *reinterpret_cast<const float4*>(gb[h] + k0 + scol);
            float* pa = sa + r * kGLd + scol;
            float* pb = sb + r * kGLd + scol;
            pa[0] = va.x; pa[1] = va.y; pa[2] = va.z; pa[3] = va.w;
            pb[0] = vb.x; pb[1] = vb.y; pb[2] = vb.z; pb[3] = vb.w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kGK; kk += 4) {
            const int kq = kk + (lane >> 4);
            double x0 = (double)sa[(qr + (lane & 15)) * kGLd + kq];
            double x1 = (double)sa[(qr + 16 + (lane & 15)) * kGLd + kq];
            double y0 = (double)sb[(qc + (lane & 15)) * kGLd + kq];
            double y1 = (double)sb[(qc + 16 + (lane & 15)) * kGLd + kq];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, acc[1][1], 0, 0, 0);
        }
    }
}

}  // namespace hmm
