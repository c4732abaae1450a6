// Shared by the scan kernels (cosine_topk.hip) and the bf16-prefilter path (cosine_topk_prefilter.hip): launch geometry, the
// per-row arithmetic that DEFINES a similarity's bits, and the conditional exact scan.
#pragma once
#include "hmm_common.h"

namespace hmm {

constexpr int kChunk = 4096;                 // keys sorted per block
constexpr int kScanBlocks = kNumCU * 8;      // workgroups of a streaming pass
constexpr int kFusedCap = 1024;              // block-local candidate list of the streaming kernels

template <bool NT>
__device__ __forceinline__ float4 ld16(const float4* p) {
    if constexpr (NT) {
        f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
        return make_float4(v[0], v[1], v[2], v[3]);
    } else {
        return *p;
    }
}

__device__ __forceinline__ void fma4(float& dot, float& ss, const float4& x, const float4& q) {
    dot = fmaf(x.x, q.x, dot); ss = fmaf(x.x, x.x, ss);
    dot = fmaf(x.y, q.y, dot); ss = fmaf(x.y, x.y, ss);
    dot = fmaf(x.z, q.z, dot); ss = fmaf(x.z, x.z, ss);
    dot = fmaf(x.w, q.w, dot); ss = fmaf(x.w, x.w, ss);
}

__device__ __forceinline__ int pow2_at_least(int n, int lo) {
    int p = lo;
    while (p < n) p <<= 1;
    return p;
}

// The similarity of one fp32 row as scan_topk_kernel / scan_sims_kernel compute it: lane l holds the float4 at columns
// 4 (64 j + l), j = 0..3 (row_lane = row + lane), q[j] the query's, q_len = sqrtf(wave_sum(sum q^2)) in the same lane order.
// Same loads, same fma order, same wave reduction, same division: the same bits (tests/test_gpu_scan.py compares them).
__device__ __forceinline__ float exact_row_sim(const float4* row_lane, const float4 (&q)[4], float q_len) {
    float4 a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = ld16<true>(row_lane + j * 64);
    float d = 0.f, s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) fma4(d, s, a[j], q[j]);
    d = wave_sum(d);
    s = wave_sum(s);
    return d / (sqrtf(s) * q_len);
}

// Up to four rows at once: all sixteen loads first (one memory latency for the group), then each row's arithmetic exactly as
// exact_row_sim has it -- the same bits.  rows[i] for i >= n are not touched; sim[i] is valid for i < n.
__device__ __forceinline__ void exact_row_sim4(const float4* const (&row_lane)[4], int n, const float4 (&q)[4], float q_len,
                                               float (&sim)[4]) {
    float4 a[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[i][j] = ld16<true>(row_lane[i] + j * 64);
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sim[i] = 0.f;
        if (i < n) {
            float d = 0.f, s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) fma4(d, s, a[i][j], q[j]);
            d = wave_sum(d);
            s = wave_sum(s);
            sim[i] = d / (sqrtf(s) * q_len);
        }
    }
}

// One row of the bf16 shadow, as hmm_shadow_store_build DEFINES its bits, from the registers of one wave: lane l holds elements
// 8 l .. 8 l + 7 (v[0], v[1]) and 512 + 8 l .. + 7 (v[2], v[3]) of the fp32 row -- two 32-B pieces in, two 16-B pieces out.
// shadow_row_out: the row's 2048 bytes.  shadow_build_kernel (cosine_topk_prefilter.hip) and store_ingest_kernel
// (store_ingest.hip) both call it: a row ingested into a store gets the shadow row a whole build would give it.
__device__ __forceinline__ void shadow_row_store(const float4 (&v)[4], int lane, uint4* __restrict__ shadow_row_out) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ss = fmaf(v[i].x, v[i].x, ss); ss = fmaf(v[i].y, v[i].y, ss);
        ss = fmaf(v[i].z, v[i].z, ss); ss = fmaf(v[i].w, v[i].w, ss);
    }
    ss = wave_sum(ss);
    float inv = 1.0f / sqrtf(ss);
    if (!(ss > 0.f) || !(ss < INFINITY)) inv = __uint_as_float(0x7FC00000u);      // zero / non-finite norm: the row is NaN
    uint4 o[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float4 a = v[2 * h], b = v[2 * h + 1];
        bf16x8 t = {(bf16_t)(a.x * inv), (bf16_t)(a.y * inv), (bf16_t)(a.z * inv), (bf16_t)(a.w * inv),
                    (bf16_t)(b.x * inv), (bf16_t)(b.y * inv), (bf16_t)(b.z * inv), (bf16_t)(b.w * inv)};
        o[h] = __builtin_bit_cast(uint4, t);
    }
    shadow_row_out[lane] = o[0];
    shadow_row_out[64 + lane] = o[1];
}

// The per-event selection kernels come in two shapes (see segment_topk_kernel): true when the small one serves this call.
constexpr int kSmallSegChunk = 1024;
bool segments_are_small(int64_t n_rows, int n_segments, int k);
// Per-event selection over fp32 similarities: query y of n_queries reads sims + y * sims_stride and fills slot (y, event) of the
// query-major outputs (cosine_topk.hip).
void launch_segment_topk(const float* sims, int64_t sims_stride, int n_queries, int64_t n_rows, const int64_t* seg_off, int n_segments,
                         int k, int64_t* idx_out, float* sim_out, int32_t* n_out, hipStream_t st);

// An upper bound of hmm_cosine_topk_workspace_bytes(n, k) that is monotone in n and in k (the plan itself is not: it changes shape
// with min(k, n)); kept beside the plan in cosine_topk.hip so that the two change together.
size_t cosine_topk_workspace_envelope(int64_t n, int k);

int cosine_topk_if(const int* run_if, unsigned* ticket, const float* store, int64_t n, const float* query, int k, int64_t* idx_out,
                   float* sim_out, int32_t* n_out, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace hmm
