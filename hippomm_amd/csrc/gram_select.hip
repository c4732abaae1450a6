// Consolidation similarity for gfx950.  Replaces HippocampalMemory._select_key_frames
// (reference hippomm/core/hippocampal_memory.py:944-967).
//
//   normalize_rows_kernel  Fn = F / ||F||_row           (:951)  fp64 sum of squares -> fp32 norm,
//                          fp32 division, exactly one rounding each.
//   gram_bits_kernel       S = Fn Fn^T                  (:952)  v_mfma_f64_16x16x4_f64: every dot
//                          product accumulated in fp64 and rounded to fp32 once, so the value
//                          is within 1 fp32 ulp of what ANY sgemm summation order produces; the
//                          kernel never materialises S: it compares (float)S < thr at once
//                          (:960) and emits one bit per pair, "not (S < thr)", which makes a NaN
//                          similarity block like `nan < thr == False` does in the reference.
//                          Only tile pairs (ti <= tj) are computed; the mirror bits are written
//                          from the same accumulator, so the relation is exactly symmetric.
//   greedy_select_kernel   the ordered scan of :955-961 on the bit matrix: keep 0; keep i iff
//                          no kept k has bit (k,i); one wave, `blocked` bitmap in LDS.
// hmm_keyframe_extend grows the same selection batch by batch (kernels and state further down); the dot products of both
// routes are gram_tile_mainloop's (gram_core.h).
// HBM layout: features (n,1024) fp32 row-major (as stacked at :842); workspace = Fn (n_pad,1024)
// fp32 + adjacency bits (n_pad x n_pad/32 uint32), n_pad = n rounded up to 64.
#include "hmm_common.h"
#include "gram_core.h"

namespace hmm {

__global__ __launch_bounds__(256) void normalize_rows_kernel(const float* __restrict__ f, int n, int n_pad,
                                                             float* __restrict__ fn) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_pad) return;
    float4* dst = reinterpret_cast<float4*>(fn + (size_t)row * HMM_FEATURE_DIM);
    if (row >= n) {                                   // padding rows: zeros (their bits are masked anyway)
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float4* src = reinterpret_cast<const float4*>(f + (size_t)row * HMM_FEATURE_DIM);
    float4 x[4];
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j] = src[j * 64 + lane];
        ss += (double)x[j].x * x[j].x + (double)x[j].y * x[j].y + (double)x[j].z * x[j].z + (double)x[j].w * x[j].w;
    }
    ss = wave_sum(ss);
    const float len = (float)sqrt(ss);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        dst[j * 64 + lane] = make_float4(x[j].x / len, x[j].y / len, x[j].z / len, x[j].w / len);
}

// One block = one 64x64 tile pair (ti <= tj) of the adjacency relation.  4 waves, each a 32x32
// quadrant = 2x2 MFMA blocks of 16x16; the dot products are gram_tile_mainloop's (gram_core.h).
__global__ __launch_bounds__(256) void gram_bits_kernel(const float* __restrict__ fn, int n, int n_pad,
                                                        float thr, uint32_t* __restrict__ adj) {
    // decode (ti, tj) with ti <= tj from the linear block id
    const int T = n_pad / kGT;
    int ti = 0, rem = blockIdx.x;
    while (rem >= T - ti) { rem -= T - ti; ++ti; }
    const int tj = ti + rem;

    __shared__ float sa[kGT * kGLd];
    __shared__ float sb[kGT * kGLd];
    __shared__ uint32_t bits_ij[kGT * 2];   // row i of tile ti -> 64 column bits of tile tj
    __shared__ uint32_t bits_ji[kGT * 2];   // row j of tile tj -> 64 column bits of tile ti

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qr = (w >> 1) * 32, qc = (w & 1) * 32;      // quadrant origin inside the tile
    if (tid < kGT * 2) { bits_ij[tid] = 0; bits_ji[tid] = 0; }

    const float* ga = fn + (size_t)ti * kGT * HMM_FEATURE_DIM + (size_t)(tid >> 3) * HMM_FEATURE_DIM;
    const float* gb = fn + (size_t)tj * kGT * HMM_FEATURE_DIM + (size_t)(tid >> 3) * HMM_FEATURE_DIM;
    f64x4 acc[2][2];
    gram_tile_mainloop(ga, ga + 32 * HMM_FEATURE_DIM, gb, gb + 32 * HMM_FEATURE_DIM, sa, sb, acc);

    // compare and collect bits in LDS
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int li = qr + a * 16 + (lane >> 4) + 4 * reg;   // row inside tile ti
                const int lj = qc + b * 16 + (lane & 15);             // col inside tile tj
                const int gi = ti * kGT + li, gj = tj * kGT + lj;
                const float s = (float)acc[a][b][reg];
                const bool hit = !(s < thr) && gi < n && gj < n;
                if (hit) {
                    atomicOr(&bits_ij[li * 2 + (lj >> 5)], 1u << (lj & 31));
                    atomicOr(&bits_ji[lj * 2 + (li >> 5)], 1u << (li & 31));
                }
            }
    __syncthreads();
    const int W = n_pad / 32;
    if (tid < kGT * 2) {
        const int r = tid >> 1, h = tid & 1;
        adj[(size_t)(ti * kGT + r) * W + tj * 2 + h] = bits_ij[tid];
        if (ti != tj) adj[(size_t)(tj * kGT + r) * W + ti * 2 + h] = bits_ji[tid];
    }
}

// One wave.  blocked[] lives in LDS (n_pad/32 words).  Row k of adj is OR-ed in when k is kept.
__global__ __launch_bounds__(64) void greedy_select_kernel(const uint32_t* __restrict__ adj, int n, int n_pad,
                                                           int64_t* __restrict__ kept, int32_t* __restrict__ n_kept) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blocked[];
    const int lane = threadIdx.x;
    const int W = n_pad / 32;
    for (int w = lane; w < W; w += 64) blocked[w] = 0;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    int count = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t word = blocked[i >> 5];            // same address in every lane: broadcast
        const bool is_blocked = (word >> (i & 31)) & 1u;
        if (i == 0 || !is_blocked) {                       // wave-uniform branch
            if (lane == 0) kept[count] = i;
            ++count;
            const uint32_t* row = adj + (size_t)i * W;
            for (int w = (i >> 5) + lane; w < W; w += 64) blocked[w] |= row[w];
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (lane == 0) *n_kept = count;
}

__global__ void arange_kernel(int n, int64_t* kept, int32_t* n_kept) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) kept[t] = t;
    if (t == 0) *n_kept = n;
}

// ---- a selection that grows (hmm_keyframe_extend) ---------------------------------------------------------------------------
// State in caller-owned memory: kept_rows (capacity,1024) fp32 = the NORMALISED rows of the kept frames in kept order, kept_idx
// int64[capacity] = their global indices, n_kept one int64.  One call appends m rows:
//   1 normalize_rows_kernel        the new rows -> workspace Fn (m_pad,1024), as the one-shot does
//   2 keyframe_kept_bits_kernel    new x kept: one bit per new row, "some kept row blocks it"
//   3 gram_bits_kernel             new x new: the one-shot relation of the batch
//   4 keyframe_greedy_kernel       the ordered scan of the batch, blocked[] seeded with step 2's bits
//   5 keyframe_append_kernel       the rows that were kept -> kept_rows[dest]
// Every (kept k, new i) and (new k, new i) dot runs gram_tile_mainloop on the same normalised bits the one-shot would hold for
// those two rows, so the bit is the one-shot's; the scan applies the same rule in the same order.

// The kept count a kernel works with: what the device holds, clamped to the host's bound and to the capacity -- a stale or wrong
// value reads or copies less, never elsewhere (the rule of store_ingest.hip).  A selection that starts holds nothing, whatever
// the word says.
__device__ __forceinline__ int64_t keyframe_kept_count(const int64_t* __restrict__ n_kept, int64_t n_seen_before,
                                                       int64_t kept_bound, int64_t capacity) {
    if (n_seen_before == 0) return 0;
    int64_t k = *n_kept;
    if (k < 0) k = 0;
    if (k > kept_bound) k = kept_bound;
    if (k > capacity) k = capacity;
    return k;
}

// grid (kept tiles up to the host's bound, new tiles).  A = 64 kept rows, B = 64 new rows: the operand order of the one-shot,
// where the earlier row of a pair is the A row (and, the products being exact and commutative, the other order gives the same
// bits).  Rows of a partial kept tile are read from the last kept row instead (never past the count) and masked.
__global__ __launch_bounds__(256) void keyframe_kept_bits_kernel(const float* __restrict__ fn, int m,
                                                                 const float* __restrict__ kept_rows, int64_t capacity,
                                                                 const int64_t* __restrict__ n_kept, int64_t n_seen_before,
                                                                 int64_t kept_bound, float thr, uint32_t* __restrict__ seed) {
    const int64_t have = keyframe_kept_count(n_kept, n_seen_before, kept_bound, capacity);
    const int64_t k0 = (int64_t)blockIdx.x * kGT;
    if (k0 >= have) return;                                // block-uniform, before any barrier
    const int tn = blockIdx.y;

    __shared__ float sa[kGT * kGLd];
    __shared__ float sb[kGT * kGLd];
    __shared__ uint32_t hit_bits[2];                       // new row j of this tile is blocked by a kept row of this tile

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qr = (w >> 1) * 32, qc = (w & 1) * 32;
    if (tid < 2) hit_bits[tid] = 0;

    const int srow = tid >> 3;
    int64_t ra0 = k0 + srow, ra1 = k0 + srow + 32;
    if (ra0 >= have) ra0 = have - 1;
    if (ra1 >= have) ra1 = have - 1;
    const float* gb = fn + ((size_t)tn * kGT + srow) * HMM_FEATURE_DIM;
    f64x4 acc[2][2];
    gram_tile_mainloop(kept_rows + ra0 * HMM_FEATURE_DIM, kept_rows + ra1 * HMM_FEATURE_DIM, gb, gb + 32 * HMM_FEATURE_DIM,
                       sa, sb, acc);

#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int lj = qc + b * 16 + (lane & 15);          // new row inside the tile
        bool any = false;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int li = qr + a * 16 + (lane >> 4) + 4 * reg;   // kept row inside the tile
                const float s = (float)acc[a][b][reg];
                any |= !(s < thr) && k0 + li < have;
            }
        if (any && tn * kGT + lj < m) atomicOr(&hit_bits[lj >> 5], 1u << (lj & 31));
    }
    __syncthreads();
    if (tid < 2 && hit_bits[tid] != 0) atomicOr(&seed[tn * 2 + tid], hit_bits[tid]);    // OR: order-free, same bits on a rerun
}

// One wave, as greedy_select_kernel; blocked[] starts from the new x kept bits.  Row i of the batch is global row
// n_seen_before + i: kept iff it is global row 0 or not blocked.  dest[i] = its slot in the state, or -1.
__global__ __launch_bounds__(64) void keyframe_greedy_kernel(const uint32_t* __restrict__ adj, const uint32_t* __restrict__ seed,
                                                             int m, int m_pad, int64_t* __restrict__ kept_idx, int64_t capacity,
                                                             int64_t* __restrict__ n_kept, int64_t n_seen_before,
                                                             int64_t kept_bound, int64_t* __restrict__ dest) {
    extern __shared__ __attribute__((aligned(16))) uint32_t blocked[];
    const int lane = threadIdx.x;
    const int W = m_pad / 32;
    const int64_t base = keyframe_kept_count(n_kept, n_seen_before, kept_bound, capacity);
    for (int w = lane; w < W; w += 64) blocked[w] = seed[w];
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    int count = 0;
    for (int i = 0; i < m; ++i) {
        const uint32_t word = blocked[i >> 5];            // same address in every lane: broadcast
        const bool is_blocked = (word >> (i & 31)) & 1u;
        if (n_seen_before + i == 0 || !is_blocked) {       // wave-uniform branch
            const int64_t slot = base + count;
            const bool fits = slot < capacity;             // the host has checked kept_bound + m <= capacity
            if (lane == 0) {
                if (fits) kept_idx[slot] = n_seen_before + i;
                dest[i] = fits ? slot : -1;
            }
            if (fits) ++count;
            const uint32_t* row = adj + (size_t)i * W;
            for (int w = (i >> 5) + lane; w < W; w += 64) blocked[w] |= row[w];
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_wave_barrier();
        } else if (lane == 0) {
            dest[i] = -1;
        }
    }
    if (lane == 0) *n_kept = base + count;
}

// One wave per new row: a kept row's 4 KB go to its slot, 16 bytes per lane and access.
__global__ __launch_bounds__(256) void keyframe_append_kernel(const float4* __restrict__ fn, int m, const int64_t* __restrict__ dest,
                                                              float4* __restrict__ kept_rows, int64_t capacity) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const int64_t d = dest[row];
    if (d < 0 || d >= capacity) return;
    const float4* src = fn + (size_t)row * 256;
    float4* dst = kept_rows + d * 256;
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = src[j * 64 + lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j * 64 + lane] = v[j];
}

struct ExtendPlan { int m_pad; size_t off_fn, off_adj, off_seed, off_dest, total; };
static ExtendPlan extend_plan(int m) {
    ExtendPlan p{};
    p.m_pad = (m + kGT - 1) / kGT * kGT;
    p.off_fn = 0;
    p.off_adj = align_up((size_t)p.m_pad * HMM_FEATURE_DIM * sizeof(float), 256);
    p.off_seed = p.off_adj + align_up((size_t)p.m_pad * (p.m_pad / 32) * sizeof(uint32_t), 256);
    p.off_dest = p.off_seed + align_up((size_t)(p.m_pad / 32) * sizeof(uint32_t), 256);
    p.total = p.off_dest + (size_t)m * sizeof(int64_t);
    return p;
}

static bool ranges_overlap(const void* a, unsigned __int128 a_bytes, const void* b, unsigned __int128 b_bytes) {
    const unsigned __int128 x = (uintptr_t)a, y = (uintptr_t)b;
    return a_bytes != 0 && b_bytes != 0 && x < y + b_bytes && y < x + a_bytes;
}

struct GramPlan { int n_pad; size_t off_fn, off_adj, total; };
static GramPlan gram_plan(int n) {
    GramPlan p{};
    p.n_pad = (n + kGT - 1) / kGT * kGT;
    p.off_fn = 0;
    p.off_adj = align_up((size_t)p.n_pad * HMM_FEATURE_DIM * sizeof(float), 256);
    p.total = p.off_adj + align_up((size_t)p.n_pad * (p.n_pad / 32) * sizeof(uint32_t), 256) + 256;  // + 256: margin only -- no kernel touches it (tests/test_gpu_memory_contract.py, profiles/memory_contract.json)
    return p;
}

}  // namespace hmm

using namespace hmm;

extern "C" size_t hmm_gram_select_workspace_bytes(int n) {
    if (n < 1) return 256;
    return gram_plan(n).total;
}

extern "C" int hmm_gram_select(const float* features_dev, int n, int dim, float threshold,
                               int64_t* kept_out_dev, int32_t* n_kept_out_dev,
                               void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "gram_select: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(n >= 0 && n <= 1000000, HMM_E_INVALID, "gram_select: n=%d out of range", n);
    HMM_REQUIRE(kept_out_dev && n_kept_out_dev, HMM_E_INVALID, "gram_select: null output pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= 2) {                                           // hippocampal_memory.py:947-948
        arange_kernel<<<1, 64, 0, st>>>(n, kept_out_dev, n_kept_out_dev);
        HMM_LAUNCH_CHECK();
        return HMM_OK;
    }
    HMM_REQUIRE(features_dev && workspace_dev, HMM_E_INVALID, "gram_select: null pointer");
    HMM_REQUIRE(((uintptr_t)features_dev & 15) == 0, HMM_E_INVALID, "gram_select: features must be 16-byte aligned");
    const GramPlan p = gram_plan(n);
    HMM_REQUIRE(workspace_bytes >= p.total, HMM_E_WORKSPACE, "gram_select: workspace %zu < required %zu",
                workspace_bytes, p.total);
    const size_t lds = (size_t)(p.n_pad / 32) * sizeof(uint32_t);
    HMM_REQUIRE(lds <= 64 * 1024, HMM_E_INVALID, "gram_select: n=%d too large for the LDS bitmap", n);
    char* base = static_cast<char*>(workspace_dev);
    float* fn = reinterpret_cast<float*>(base + p.off_fn);
    uint32_t* adj = reinterpret_cast<uint32_t*>(base + p.off_adj);

    normalize_rows_kernel<<<(p.n_pad + 3) / 4, 256, 0, st>>>(features_dev, n, p.n_pad, fn);
    HMM_LAUNCH_CHECK();
    const int T = p.n_pad / kGT;
    gram_bits_kernel<<<T * (T + 1) / 2, 256, 0, st>>>(fn, n, p.n_pad, threshold, adj);
    HMM_LAUNCH_CHECK();
    greedy_select_kernel<<<1, 64, lds, st>>>(adj, n, p.n_pad, kept_out_dev, n_kept_out_dev);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

extern "C" size_t hmm_keyframe_extend_workspace_bytes(int m) {
    if (m < 1) return 256;
    return extend_plan(m).total;
}

extern "C" int hmm_keyframe_extend(const float* new_rows_dev, int m, int dim, float threshold, float* kept_rows_dev,
                                   int64_t* kept_idx_dev, int64_t capacity_kept, int64_t* n_kept_dev, int64_t n_seen_before,
                                   int64_t kept_bound, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "keyframe_extend: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(m >= 0 && capacity_kept >= 0 && n_seen_before >= 0 && kept_bound >= 0, HMM_E_INVALID,
                "keyframe_extend: negative count (m=%d, capacity_kept=%lld, n_seen_before=%lld, kept_bound=%lld)", m,
                (long long)capacity_kept, (long long)n_seen_before, (long long)kept_bound);
    HMM_REQUIRE(n_seen_before <= INT64_MAX - m, HMM_E_INVALID, "keyframe_extend: n_seen_before=%lld + m=%d is out of range",
                (long long)n_seen_before, m);
    HMM_REQUIRE(kept_bound <= n_seen_before, HMM_E_INVALID, "keyframe_extend: kept_bound=%lld exceeds the %lld rows seen",
                (long long)kept_bound, (long long)n_seen_before);
    HMM_REQUIRE(m <= capacity_kept && kept_bound <= capacity_kept - m, HMM_E_INVALID,
                "keyframe_extend: %d new rows on up to %lld kept rows exceed the capacity of %lld rows", m, (long long)kept_bound,
                (long long)capacity_kept);
    if (m == 0) return HMM_OK;                                                // nothing to decide: no pointer is looked at
    HMM_REQUIRE(new_rows_dev && kept_rows_dev && kept_idx_dev && n_kept_dev && workspace_dev, HMM_E_INVALID,
                "keyframe_extend: null pointer");
    HMM_REQUIRE(((uintptr_t)new_rows_dev & 15) == 0 && ((uintptr_t)kept_rows_dev & 15) == 0 && ((uintptr_t)workspace_dev & 15) == 0,
                HMM_E_INVALID, "keyframe_extend: new rows / kept rows / workspace must be 16-byte aligned");
    HMM_REQUIRE(((uintptr_t)kept_idx_dev & 7) == 0 && ((uintptr_t)n_kept_dev & 7) == 0, HMM_E_INVALID,
                "keyframe_extend: kept_idx / n_kept must be 8-byte aligned");
    const ExtendPlan p = extend_plan(m);
    const size_t lds = (size_t)(p.m_pad / 32) * sizeof(uint32_t);
    HMM_REQUIRE(lds <= 64 * 1024, HMM_E_INVALID, "keyframe_extend: m=%d too large for the LDS bitmap", m);
    const unsigned __int128 new_bytes = (unsigned __int128)m * 4096, cap = (unsigned __int128)capacity_kept;
    HMM_REQUIRE(!ranges_overlap(new_rows_dev, new_bytes, kept_rows_dev, cap * 4096) &&
                    !ranges_overlap(new_rows_dev, new_bytes, kept_idx_dev, cap * 8) &&
                    !ranges_overlap(new_rows_dev, new_bytes, n_kept_dev, 8),
                HMM_E_INVALID, "keyframe_extend: the new rows overlap the selection's state");
    HMM_REQUIRE(workspace_bytes >= p.total, HMM_E_WORKSPACE, "keyframe_extend: workspace %zu < required %zu", workspace_bytes,
                p.total);
    const int64_t kept_tiles = (kept_bound + kGT - 1) / kGT;
    HMM_REQUIRE(kept_tiles <= INT32_MAX, HMM_E_INVALID, "keyframe_extend: kept_bound=%lld too large for one grid",
                (long long)kept_bound);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(workspace_dev);
    float* fn = reinterpret_cast<float*>(base + p.off_fn);
    uint32_t* adj = reinterpret_cast<uint32_t*>(base + p.off_adj);
    uint32_t* seed = reinterpret_cast<uint32_t*>(base + p.off_seed);
    int64_t* dest = reinterpret_cast<int64_t*>(base + p.off_dest);
    const int T = p.m_pad / kGT;

    HMM_HIP_CHECK(hipMemsetAsync(seed, 0, lds, st));
    normalize_rows_kernel<<<(p.m_pad + 3) / 4, 256, 0, st>>>(new_rows_dev, m, p.m_pad, fn);
    HMM_LAUNCH_CHECK();
    if (kept_tiles > 0) {
        keyframe_kept_bits_kernel<<<dim3((unsigned)kept_tiles, (unsigned)T), 256, 0, st>>>(
            fn, m, kept_rows_dev, capacity_kept, n_kept_dev, n_seen_before, kept_bound, threshold, seed);
        HMM_LAUNCH_CHECK();
    }
    gram_bits_kernel<<<T * (T + 1) / 2, 256, 0, st>>>(fn, m, p.m_pad, threshold, adj);
    HMM_LAUNCH_CHECK();
    keyframe_greedy_kernel<<<1, 64, lds, st>>>(adj, seed, m, p.m_pad, kept_idx_dev, capacity_kept, n_kept_dev, n_seen_before,
                                               kept_bound, dest);
    HMM_LAUNCH_CHECK();
    keyframe_append_kernel<<<(m + 3) / 4, 256, 0, st>>>(reinterpret_cast<const float4*>(fn), m, dest,
                                                        reinterpret_cast<float4*>(kept_rows_dev), capacity_kept);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}
