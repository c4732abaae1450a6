// A store that grows on the device: the two copies behind EventStore.append_event / remove_events / replace_event
// (hippomm_amd/vector_ops.py).
//
//   ingest   store_ingest_kernel reads new rows where they lie (fp32, or fp64 as load_theta_event hands them over) and writes, in
//            ONE pass, the fp32 rows [row_offset, row_offset + n_new) of the store and -- when the store has one -- the same rows
//            of the bf16 shadow.  An fp32 source is copied as bits; an fp64 source is narrowed with round-to-nearest-even
//            (v_cvt_f32_f64 under the default float mode: what ndarray.astype(float32) does on the host, subnormal results and
//            the round-up to infinity included; tests/test_gpu_store_growth.py compares the bits).  The shadow row comes from
//            shadow_row_store (cosine_topk_shared.h), the body of shadow_build_kernel: the same bits by construction.
//   gather   store_gather_kernel moves whole events between two buffers under two offset tables: destination segment j receives
//            source segment src_segment[j] or stays untouched (-1: a hole for the ingest).  Out of place: no workgroup waits for
//            another one.  Every row is re-derived from the tables and clamped, so a wrong table copies less, never elsewhere.
//
// Both are HBM-bound copies: 16-byte loads and stores, eight (ingest) or twelve (gather) loads in flight per lane, a grid capped
// at kScanBlocks workgroups as the scans' is.  No LDS, no scratch, vector stores only.
#include "hmm_common.h"
#include "cosine_topk_shared.h"

namespace hmm {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint4 ld16_stream(const uint4* p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// The lane's four float4 of source row r in shadow_row_store's order: elements 8 l .. 8 l + 7 and 512 + 8 l .. + 7.
template <bool F64>
__device__ __forceinline__ void ingest_load_row(const void* __restrict__ src, int64_t r, int lane, float4 (&v)[4]) {
    if constexpr (!F64) {
        const uint4* p = static_cast<const uint4*>(src) + r * 256;
        const int at[4] = {2 * lane, 2 * lane + 1, 128 + 2 * lane, 128 + 2 * lane + 1};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 b = ld16_stream(p + at[i]);               // moved as bits: NaN payloads, -0.0 and subnormals survive
            v[i] = make_float4(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w));
        }
    } else {
        const f64x2* p = static_cast<const f64x2*>(src) + r * 512;            // 512 pairs of doubles per row
        f64x2 d[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            d[i] = __builtin_nontemporal_load(p + 4 * lane + i);
            d[4 + i] = __builtin_nontemporal_load(p + 256 + 4 * lane + i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)                                           // (float)double: round to nearest even
            v[i] = make_float4((float)d[2 * i][0], (float)d[2 * i][1], (float)d[2 * i + 1][0], (float)d[2 * i + 1][1]);
    }
}

// One wave per group of ROWS consecutive rows; store / shadow point at the first row to write.
template <bool F64, int ROWS>
__global__ __launch_bounds__(256) void store_ingest_kernel(const void* __restrict__ src, int64_t n_new, float4* __restrict__ store,
                                                           uint4* __restrict__ shadow) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r0 = wave * ROWS; r0 < n_new; r0 += n_waves * ROWS) {
        const int have = n_new - r0 >= ROWS ? ROWS : (int)(n_new - r0);       // wave-uniform
        float4 v[ROWS][4];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) ingest_load_row<F64>(src, r0 + (i < have ? i : 0), lane, v[i]);
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            if (i < have) {
                float4* out = store + (r0 + i) * 256;
                out[2 * lane] = v[i][0];
                out[2 * lane + 1] = v[i][1];
                out[128 + 2 * lane] = v[i][2];
                out[128 + 2 * lane + 1] = v[i][3];
                if (shadow != nullptr) shadow_row_store(v[i], lane, shadow + (r0 + i) * 128);
            }
        }
    }
}

// The source row of destination row r, or -1 when r is not to be written: outside every destination segment, in a hole, or
// beyond the rows its source segment has.  Wave-uniform (r is).
__device__ __forceinline__ int64_t gather_source_row(int64_t r, const int64_t* __restrict__ src_off, int n_src, int64_t src_rows,
                                                     const int32_t* __restrict__ src_seg, const int64_t* __restrict__ dst_off,
                                                     int n_dst) {
    int lo = 0, hi = n_dst - 1;                                               // the last segment that starts at or before r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (dst_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int64_t d0 = dst_off[lo], d1 = dst_off[lo + 1];
    if (r < d0 || r >= d1) return -1;
    const int seg = src_seg[lo];
    if (seg < 0 || seg >= n_src) return -1;
    const int64_t s0 = src_off[seg];
    int64_t s1 = src_off[seg + 1];
    if (s1 > src_rows) s1 = src_rows;
    const int64_t s = s0 + (r - d0);
    return (s0 < 0 || s >= s1) ? -1 : s;
}

__global__ __launch_bounds__(256) void store_gather_kernel(const uint4* __restrict__ src_store, const uint4* __restrict__ src_shadow,
                                                           int64_t src_rows, const int64_t* __restrict__ src_off, int n_src,
                                                           const int32_t* __restrict__ src_seg, const int64_t* __restrict__ dst_off,
                                                           int n_dst, uint4* __restrict__ dst_store, uint4* __restrict__ dst_shadow,
                                                           int64_t dst_rows) {
    constexpr int ROWS = 2;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r0 = wave * ROWS; r0 < dst_rows; r0 += n_waves * ROWS) {
        int64_t s[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
            s[i] = r0 + i < dst_rows ? gather_source_row(r0 + i, src_off, n_src, src_rows, src_seg, dst_off, n_dst) : -1;
        uint4 a[ROWS][4], b[ROWS][2];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            if (s[i] >= 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[i][j] = ld16_stream(src_store + s[i] * 256 + j * 64 + lane);
                if (src_shadow != nullptr) {
                    b[i][0] = ld16_stream(src_shadow + s[i] * 128 + lane);
                    b[i][1] = ld16_stream(src_shadow + s[i] * 128 + 64 + lane);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            if (s[i] >= 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dst_store[(r0 + i) * 256 + j * 64 + lane] = a[i][j];
                if (src_shadow != nullptr) {
                    dst_shadow[(r0 + i) * 128 + lane] = b[i][0];
                    dst_shadow[(r0 + i) * 128 + 64 + lane] = b[i][1];
                }
            }
        }
    }
}

static bool bytes_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
    return a != nullptr && b != nullptr && a_bytes != 0 && b_bytes != 0 && x < y + b_bytes && y < x + a_bytes;
}

static unsigned copy_blocks(int64_t rows, int rows_per_wave) {
    const int64_t blocks = (rows + 4 * rows_per_wave - 1) / (4 * rows_per_wave);
    return (unsigned)(blocks > kScanBlocks ? kScanBlocks : blocks);
}

}  // namespace hmm

using namespace hmm;

extern "C" int hmm_store_ingest_rows(const void* src_dev, int src_dtype, int64_t n_new, int dim, float* store_dev, void* shadow_dev,
                                     int64_t capacity_rows, int64_t row_offset, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "store_ingest_rows: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(src_dtype == 0 || src_dtype == 1, HMM_E_INVALID, "store_ingest_rows: src_dtype must be 0 (fp32) or 1 (fp64), got %d",
                src_dtype);
    HMM_REQUIRE(n_new >= 0 && capacity_rows >= 0 && row_offset >= 0, HMM_E_INVALID,
                "store_ingest_rows: negative count (n_new=%lld, capacity_rows=%lld, row_offset=%lld)", (long long)n_new,
                (long long)capacity_rows, (long long)row_offset);
    HMM_REQUIRE(n_new <= capacity_rows && row_offset <= capacity_rows - n_new, HMM_E_INVALID,
                "store_ingest_rows: %lld rows at row %lld exceed the capacity of %lld rows", (long long)n_new,
                (long long)row_offset, (long long)capacity_rows);
    if (n_new == 0) return HMM_OK;                                            // nothing to write: no pointer is looked at
    HMM_REQUIRE(src_dev && store_dev, HMM_E_INVALID, "store_ingest_rows: null pointer");
    HMM_REQUIRE(((uintptr_t)src_dev & 15) == 0 && ((uintptr_t)store_dev & 15) == 0 && ((uintptr_t)shadow_dev & 15) == 0, HMM_E_INVALID,
                "store_ingest_rows: source / store / shadow must be 16-byte aligned");
    float* store_at = store_dev + row_offset * HMM_FEATURE_DIM;
    char* shadow_at = shadow_dev ? static_cast<char*>(shadow_dev) + row_offset * 2048 : nullptr;
    const uint64_t src_bytes = (uint64_t)n_new * HMM_FEATURE_DIM * (src_dtype == 1 ? 8 : 4);
    HMM_REQUIRE(!bytes_overlap(src_dev, src_bytes, store_at, (uint64_t)n_new * 4096) &&
                    !bytes_overlap(src_dev, src_bytes, shadow_at, (uint64_t)n_new * 2048),
                HMM_E_INVALID, "store_ingest_rows: the source overlaps the rows it is ingested into");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (src_dtype == 1)
        store_ingest_kernel<true, 1><<<copy_blocks(n_new, 1), 256, 0, st>>>(src_dev, n_new, reinterpret_cast<float4*>(store_at),
                                                                            reinterpret_cast<uint4*>(shadow_at));
    else
        store_ingest_kernel<false, 2><<<copy_blocks(n_new, 2), 256, 0, st>>>(src_dev, n_new, reinterpret_cast<float4*>(store_at),
                                                                             reinterpret_cast<uint4*>(shadow_at));
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" int hmm_store_gather_segments(const float* src_store_dev, const void* src_shadow_dev, int64_t src_rows,
                                         const int64_t* src_offsets_dev, int n_src_segments, const int32_t* src_segment_dev,
                                         const int64_t* dst_offsets_dev, int n_dst, int dim, float* dst_store_dev, void* dst_shadow_dev,
                                         int64_t dst_rows, int64_t dst_capacity_rows, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "store_gather_segments: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(src_rows >= 0 && n_src_segments >= 0 && n_dst >= 0 && dst_rows >= 0 && dst_capacity_rows >= 0, HMM_E_INVALID,
                "store_gather_segments: negative count (src_rows=%lld, n_src_segments=%d, n_dst=%d, dst_rows=%lld, "
                "dst_capacity_rows=%lld)", (long long)src_rows, n_src_segments, n_dst, (long long)dst_rows, (long long)dst_capacity_rows);
    HMM_REQUIRE(dst_rows <= dst_capacity_rows, HMM_E_INVALID, "store_gather_segments: dst_rows=%lld exceeds the capacity of %lld rows",
                (long long)dst_rows, (long long)dst_capacity_rows);
    HMM_REQUIRE((src_shadow_dev == nullptr) == (dst_shadow_dev == nullptr), HMM_E_INVALID,
                "store_gather_segments: source and destination shadow must both be given or both be null");
    if (n_dst == 0 || dst_rows == 0) return HMM_OK;                           // nothing to write: no other pointer is looked at
    HMM_REQUIRE(src_store_dev && src_offsets_dev && src_segment_dev && dst_offsets_dev && dst_store_dev, HMM_E_INVALID,
                "store_gather_segments: null pointer");
    HMM_REQUIRE(((uintptr_t)src_store_dev & 15) == 0 && ((uintptr_t)src_shadow_dev & 15) == 0 && ((uintptr_t)dst_store_dev & 15) == 0 &&
                    ((uintptr_t)dst_shadow_dev & 15) == 0, HMM_E_INVALID,
                "store_gather_segments: stores / shadows must be 16-byte aligned");
    HMM_REQUIRE(((uintptr_t)src_offsets_dev & 7) == 0 && ((uintptr_t)dst_offsets_dev & 7) == 0 && ((uintptr_t)src_segment_dev & 3) == 0,
                HMM_E_INVALID, "store_gather_segments: offset tables must be aligned to their element size");
    const uint64_t s4 = (uint64_t)src_rows * 4096, s2 = (uint64_t)src_rows * 2048, d4 = (uint64_t)dst_rows * 4096,
                   d2 = (uint64_t)dst_rows * 2048;
    HMM_REQUIRE(!bytes_overlap(src_store_dev, s4, dst_store_dev, d4) && !bytes_overlap(src_store_dev, s4, dst_shadow_dev, d2) &&
                    !bytes_overlap(src_shadow_dev, s2, dst_store_dev, d4) && !bytes_overlap(src_shadow_dev, s2, dst_shadow_dev, d2),
                HMM_E_INVALID, "store_gather_segments: the source overlaps the destination (the gather is out of place)");
    store_gather_kernel<<<copy_blocks(dst_rows, 2), 256, 0, static_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const uint4*>(src_store_dev), static_cast<const uint4*>(src_shadow_dev), src_rows, src_offsets_dev,
        n_src_segments, src_segment_dev, dst_offsets_dev, n_dst, reinterpret_cast<uint4*>(dst_store_dev),
        static_cast<uint4*>(dst_shadow_dev), dst_rows);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
