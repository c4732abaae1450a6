// Batched feature_search: top-k cosine rows for up to 16 queries in ONE pass over the (N,1024)
// fp32 store.  The reference scans once per question and per modality (top_k_cosine_similarity,
// hippomm/utils/vector_ops.py:151-188, called at hippocampal_memory.py:3153 / :3304); with several questions queued
// the store would be read once per question.  Here a row is read once for all of them: HBM-bound like the single-query
// scan (4096 B per row), i.e. up to 16 x the per-query throughput.
//
// The Q x rows similarity block is a GEMM on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: store rows are the
// A operand, queries the B operand, IEEE fp32 products and sums -- no precision is given up): per row 2 x 1024 x 16
// FLOP, ~50 TFLOP/s at the HBM-bound row rate against a ~157 TFLOP/s fp32 matrix peak, so the kernel stays on the
// memory roofline.
//
// Data movement (round 2; round 1 read 16 rows x 64 B per load instruction straight into registers and stopped at
// 5.0 TB/s of loads):
//   * the store is streamed by LDS-DMA in 512-B row pieces: one global_load_lds_dwordx4 fetches 2 rows x 512 B
//     (whole 128-B lines, two contiguous runs), a wave keeps a private ring of 4 slices (16 rows x 128 floats, 8 KiB)
//     with three slices always in flight behind a counted vmcnt -- no registers are spent on loads;
//   * the 16 queries live in REGISTERS: the B operand of lane (q, g) is q[.][32 g + 4 j + s], 256 values per lane for
//     the whole kernel (one wave per SIMD, 512 registers), so the main loop reads nothing but the A fragments from
//     LDS: one ds_read_b128 per four MFMAs;
//   * LDS image of a slice: piece i (rows 2i, 2i+1) at i x 1056 B, inside it 16-B unit 2c + (row & 1) holds chunk c of
//     the row -- the source address of each DMA lane is permuted accordingly.  A fragment read (the 16 rows of a
//     ds_read_b128 lane group, see a_lane below) then touches 16 different 16-B bank slots: conflict-free, measured.
// Selection is fused: every query has a candidate list of order keys in LDS and a threshold = its current k-th best;
// only keys above the threshold are appended (LDS atomic), lists are sorted down to k when they could overflow and at
// the end, and each workgroup leaves its best k keys per query.  (Sharing the thresholds chip-wide through one monotone
// word per query in global memory was built and measured: 0.75 -> 0.83 ms per pass -- the contended line and the atomics
// sit in the in-order VMEM queue in front of the slice waits.  Not kept.)  A second kernel (one workgroup per query) finishes
// exactly as topk_final_kernel does: the global top-k lies in the lists of the k workgroups with the largest maxima.
// Keys, total order (NaN first, higher row first on ties) and outputs are those of hmm_cosine_topk.
#include "cosine_topk_shared.h"
#include "topk_tournament.h"
#include "topk_select.h"

namespace hmm {

constexpr int kMWaves = 4;              // one wave per SIMD: 512 registers each (256 of them hold the queries)
using MultiDealing = RowDealing<kMTileRows, kMWaves>;       // scan_multi_kernel: one tile of kMTileRows rows per wave and round (kMQ, kMTileRows: topk_select.h)
constexpr int kMSlices = 8;             // K slices per tile: 128 floats each
constexpr int kMPiece = 1056;           // LDS bytes per DMA piece: 2 rows x 512 B + 32 B (bank rotation between pieces)
constexpr int kMSliceBytes = 8 * kMPiece;
constexpr int kMRing = 4;               // slices per wave: one being read, three in flight (96 KiB per CU).  Depth is not the limit:
                                        // 2 / 3 / 4 slices 0.648 / 0.654 / 0.651 ms per pass in one session (round 6).  Nor are the
                                        // MFMAs (VALU dot products instead: 0.653) or, mostly, the 512-B pieces: the bare DMA stream of
                                        // this kernel, nothing read or computed, runs 0.613 against 0.650.  1-KiB pieces (one row x 256
                                        // floats per instruction, 16-KiB slices) leave room for only two slices per wave: 0.683
constexpr int kMCap = 128;              // candidate keys per query and workgroup (>= k + MultiDealing::kBlockRows, power of two)
constexpr int kMMaxK = kListMaxK;       // k*k <= 4096 for the one-kernel finish
constexpr int kMMaxBlocks = 2048;
constexpr int kMDmaAux = 2;             // cache policy of the row stream: 2 = non-temporal (each row is read once; 0: 0.724 ms)

struct MultiLds {
    char ring[kMWaves][kMRing][kMSliceBytes];     // 135168 B
    uint64_t keys[kMQ][kMCap];                     //  16384 B
    uint64_t tau[kMQ];
    int cnt[kMQ];
    int need;                                      // workgroup-uniform "sort now" flag (written by wave 0 between barriers)
};

#define HMM_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define HMM_GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

// ---- the arithmetic that DEFINES the bits of a batched similarity ------------------------------------------------------------
// Shared by scan_multi_kernel and the re-scoring of the shadow route (multi_rescore_tile): a (row, query) pair gets the same
// bits from both because both run exactly this sequence.  Lane (r16, g) of a wave holds, for K slice sl and step j, the floats
// 128 sl + 32 g + 4 j + 0..3 of row r16 (A fragment x[j]) and of query r16 (B fragment b[j]).
__device__ __forceinline__ void multi_sumsq4(float& ss, const f32x4& v) {
    ss = fmaf(v[0], v[0], ss); ss = fmaf(v[1], v[1], ss); ss = fmaf(v[2], v[2], ss); ss = fmaf(v[3], v[3], ss);
}
// one K slice: 32 MFMA steps alternating two accumulators, and the row's partial sum of squares
__device__ __forceinline__ void multi_slice_mac(const f32x4 (&x)[8], const f32x4 (&b)[8], f32x4& acc0, f32x4& acc1, float& ss) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][0], b[j][0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][1], b[j][1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][2], b[j][2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][3], b[j][3], acc1, 0, 0, 0);
        multi_sumsq4(ss, x[j]);
    }
}
// the length of row / query r16: its four lanes (r16, g = 0..3) hold the partial sums
__device__ __forceinline__ float multi_len(float ss) {
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    return sqrtf(ss);
}
// after the eight slices: the similarities of query r16 with rows 4 g + 0..3 of the tile (the D layout of the MFMA)
__device__ __forceinline__ f32x4 multi_tile_sims(const f32x4& acc0, const f32x4& acc1, float ss, float my_qlen, int g) {
    const float norm = multi_len(ss);                             // row r16 of the tile
    const f32x4 acc = acc0 + acc1;
    f32x4 sim4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float rn = __shfl(norm, 4 * g + j, 64);
        sim4[j] = acc[j] / (rn * my_qlen);
    }
    return sim4;
}

// SIMS_OUT (hmm_cosine_topk_segmented_multi): the same pass, the same similarities bit for bit, but nothing is selected here --
// the similarity of (query q, row r) goes to sims_out[q * sims_stride + r] (sims_stride = rows rounded up to whole tiles, so a lane
// stores its four rows with one 16-byte store; the entries of the rows past the end are never read) and a per-event selection
// follows in its own launch.  No candidate lists, so the waves of a workgroup never meet after the prologue.
template <bool SIMS_OUT>
__global__ __launch_bounds__(kMWaves * 64) void scan_multi_kernel(const float* __restrict__ store, int64_t n_rows,
                                                                  const float* __restrict__ queries, int n_q, int k,
                                                                  uint64_t* __restrict__ out, float* __restrict__ sims_out,
                                                                  int64_t sims_stride, const int* __restrict__ run_if) {
    if (run_if != nullptr && *run_if == 0) return;                // the conditional exact pass behind the shadow route: flag down
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    MultiLds& L = *reinterpret_cast<MultiLds*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;

    // B operand: lane (q = r16, g) holds q[128 s + 32 g + 4 j + 0..3] for every slice s and step j (zero rows past n_q).
    // The queries pass through LDS once (coalesced 16-B loads, rows padded by 16 B against bank conflicts; the ring is
    // still idle): fetching the 64 fragments per lane straight from global memory serialises 64 L2 round trips.
    {
        constexpr int QS = 1024 + 4;                              // floats per staged query row
        float* qs = reinterpret_cast<float*>(&L.ring[0][0][0]);   // 16 x 4112 B = 65792 B of the 101376-B ring
        for (int i = tid; i < kMQ * 256; i += kMWaves * 64) {
            const int qi = i >> 8, c = i & 255;
            const int src_row = qi < n_q ? qi : n_q - 1;          // clamped row + select: no branch around the load
            f32x4 v = *reinterpret_cast<const f32x4*>(queries + (size_t)src_row * 1024 + 4 * c);
            if (qi >= n_q) v = f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(qs + qi * QS + 4 * c) = v;
        }
        __syncthreads();
    }
    f32x4 bq[kMSlices][8];
    float qss = 0.f;
    {
        constexpr int QS = 1024 + 4;
        const float* qs = reinterpret_cast<const float*>(&L.ring[0][0][0]) + r16 * QS + 32 * g;
#pragma unroll
        for (int sl = 0; sl < kMSlices; ++sl)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(qs + 128 * sl + 4 * j);
                bq[sl][j] = v;
                multi_sumsq4(qss, v);
            }
    }
    const float my_qlen = multi_len(qss);                         // |query r16|, in all four lanes that hold a part of it
    if (tid < kMQ) { L.cnt[tid] = 0; L.tau[tid] = 0ull; }
    if (tid == 0) L.need = 0;
    __syncthreads();                                              // fragments are in registers: the ring may be overwritten

    const int64_t n_tiles = (n_rows + kMTileRows - 1) / kMTileRows;
    const int64_t n_waves = (int64_t)gridDim.x * kMWaves;
    const int64_t wave_gid = (int64_t)blockIdx.x * kMWaves + wave;
    const int64_t n_rounds = (n_tiles + n_waves - 1) / n_waves;   // same for every wave of the grid

    // DMA source of lane l for piece i of (tile, slice): row 16 tile + 2 i + (l & 1), floats 128 slice + 4 (l >> 1) .. + 3
    char* my_ring = L.ring[wave][0];
    auto issue_slice = [&](int64_t tile, int sl, int slot) {
        int64_t row0 = tile * kMTileRows;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int64_t row = row0 + 2 * i + (lane & 1);
            row = row < n_rows ? row : n_rows - 1;                // clamp: rows past the end are masked at selection
            const float* src = store + row * 1024 + 128 * sl + (lane >> 1) * 4;
            __builtin_amdgcn_global_load_lds(HMM_GLB_PTR(src), HMM_LDS_PTR(my_ring + slot * kMSliceBytes + i * kMPiece),
                                             16, 0, kMDmaAux);
        }
    };
    // A fragment of lane (r16, g), step j: chunk c = 8 g + j of row r16 -> unit 2 c + (r16 & 1) of piece r16 >> 1.  k-slot g of
    // the MFMA owns the 32 floats 32 g .. 32 g + 31 of a slice (the B fragments above use the same assignment), so the four
    // k-slots sit 256 B = one full bank row apart: a ds_read_b128 is serviced in the lane groups {0-3, 12-15, 20-27}, ...
    // (MI355X_MICROARCH.md, LDS), i.e. rows {0-3, 12-15} of one k-slot with rows {4-11} of the next -- 16 different rows, 16
    // different 16-B bank slots.  (With chunk 4 j + g, 32 B between k-slots, rows 10 / 11 of one slot met rows 12 / 13 of the
    // other: SQ_LDS_BANK_CONFLICT = 41 % of the kernel's LDS cycles.)
    const int a_lane = (r16 >> 1) * kMPiece + (r16 & 1) * 16 + g * 256;

    // flattened (round, slice) sequence n = 8 round + slice; slot n % kMRing; slices n + 1 .. n + LA are in flight while n is read
    constexpr int LA = kMRing - 1;
    auto tile_of = [&](int64_t round) { return MultiDealing::group(wave_gid, round, n_waves); };
#pragma unroll
    for (int p = 0; p < LA; ++p) issue_slice(tile_of(0), p, p);
    int slot = 0;                                                 // slot of the slice being read
    for (int64_t round = 0; round < n_rounds; ++round) {
        const int64_t tile = tile_of(round);
        f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        float ss = 0.f;
#pragma unroll
        for (int sl = 0; sl < kMSlices; ++sl) {
            // refill the slot read in the previous step (its ds_reads were waited for before that step's MFMAs)
            const int nslot = slot == 0 ? kMRing - 1 : slot - 1;  // (slot + LA) % kMRing
            if (sl + LA < kMSlices) issue_slice(tile, sl + LA, nslot);
            else                    issue_slice(tile_of(round + 1), sl + LA - kMSlices, nslot);   // next round (clamped past the end)
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(LA * 8) : "memory");     // slice n has landed; n + 1 .. n + LA stay in flight
            __builtin_amdgcn_sched_barrier(0);
            const char* ap = my_ring + slot * kMSliceBytes + a_lane;
            f32x4 x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const f32x4*>(ap + j * 32);
            multi_slice_mac(x, bq[sl], acc0, acc1, ss);
            slot = slot == kMRing - 1 ? 0 : slot + 1;
        }
        const f32x4 sim4 = multi_tile_sims(acc0, acc1, ss, my_qlen, g);     // D layout: query r16, rows 4 g + j
        if constexpr (SIMS_OUT) {
            if (tile < n_tiles && r16 < n_q)
                *reinterpret_cast<f32x4*>(sims_out + r16 * sims_stride + tile * kMTileRows + 4 * g) = sim4;
            continue;
        }
        // fused selection: appends above the thresholds, lists sorted down to k when they could overflow (multi_lists_round)
        multi_lists_round<MultiDealing, kMCap>(L, sim4, tile, n_tiles, n_rows, n_q, k, round + 1 >= n_rounds || round == 0, wave, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the look-ahead slices past the end
    if constexpr (SIMS_OUT) return;
    multi_lists_flush<MultiDealing>(L, n_q, k, out);
}

// One workgroup per query: see topk_final_kernel; the lists are scan_multi_kernel's (MultiDealing).
__global__ __launch_bounds__(1024) void topk_final_multi_kernel(const uint64_t* __restrict__ cand, int n_blocks, int k,
                                                                int k_eff, int64_t* __restrict__ idx_out,
                                                                float* __restrict__ sim_out, int32_t* __restrict__ n_out,
                                                                int k_stride, const int* __restrict__ run_if) {
    __shared__ uint64_t mx[kMMaxBlocks];
    __shared__ uint64_t s[4096];
    if (run_if != nullptr && *run_if == 0) return;                // see scan_multi_kernel
    const int qi = blockIdx.x;
    rank_winning_lists<MultiDealing, 1024>(cand + (size_t)qi * n_blocks * k, n_blocks, k, k, mx, s);     // k <= kMMaxK = 64
    write_hits(s, k_eff, k_eff, idx_out + (size_t)qi * k_stride, sim_out + (size_t)qi * k_stride, n_out ? n_out + qi : nullptr);
}

static int multi_grid(int64_t n_rows) {                        // one workgroup per CU (its LDS fills the CU), 64 rows per round
    return MultiDealing::grid(n_rows, kNumCU);
}

}  // namespace hmm

using namespace hmm;

extern "C" size_t hmm_cosine_topk_workspace_bytes(int64_t n_rows, int k);
extern "C" int hmm_cosine_topk(const float* store_dev, int64_t n_rows, int dim, const float* query_dev, int k,
                               int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                               void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

extern "C" size_t hmm_cosine_topk_multi_workspace_bytes(int64_t n_rows, int n_queries, int k) {
    if (n_rows < 1 || n_queries < 1 || k < 1) return 0;
    const int64_t k_eff = k < n_rows ? k : n_rows;
    if (k_eff > kMMaxK) return hmm_cosine_topk_workspace_bytes(n_rows, k);           // per-query fallback
    return align_up((size_t)kMQ * multi_grid(n_rows) * (size_t)k_eff * 8, 256) + 256;  // + 256: margin only -- no kernel touches it (tests/test_gpu_memory_contract.py, profiles/memory_contract.json)
}

extern "C" int hmm_cosine_topk_multi(const float* store_dev, int64_t n_rows, int dim, const float* queries_dev,
                                     int n_queries, int k, int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                     void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "cosine_topk_multi: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(n_rows >= 1 && n_rows < (int64_t)0xFFFFFFFFll, HMM_E_INVALID, "cosine_topk_multi: n_rows=%lld out of range",
                (long long)n_rows);
    HMM_REQUIRE(n_queries >= 1 && k >= 1, HMM_E_INVALID, "cosine_topk_multi: n_queries=%d k=%d", n_queries, k);
    HMM_REQUIRE(store_dev && queries_dev && idx_out_dev && sim_out_dev && workspace_dev, HMM_E_INVALID,
                "cosine_topk_multi: null pointer");
    HMM_REQUIRE(((uintptr_t)store_dev & 15) == 0 && ((uintptr_t)queries_dev & 15) == 0, HMM_E_INVALID,
                "cosine_topk_multi: store/queries must be 16-byte aligned");
    const size_t need = hmm_cosine_topk_multi_workspace_bytes(n_rows, n_queries, k);
    HMM_REQUIRE(workspace_bytes >= need, HMM_E_WORKSPACE, "cosine_topk_multi: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int k_eff = (int)(k < n_rows ? k : n_rows);
    if (k_eff > kMMaxK) {                                          // large k: one ordinary scan per query
        for (int qi = 0; qi < n_queries; ++qi) {
            const int rc = hmm_cosine_topk(store_dev, n_rows, dim, queries_dev + (size_t)qi * dim, k,
                                           idx_out_dev + (size_t)qi * k, sim_out_dev + (size_t)qi * k,
                                           n_out_dev ? n_out_dev + qi : nullptr, workspace_dev, workspace_bytes, stream);
            if (rc != HMM_OK) return rc;
        }
        return HMM_OK;
    }
    HMM_ENSURE_DYN_LDS(scan_multi_kernel<false>, (int)sizeof(MultiLds));
    const int grid = multi_grid(n_rows);
    uint64_t* cand = static_cast<uint64_t*>(workspace_dev);
    return for_each_pass(n_queries, [&](const QuestionPass& pass) -> int {       // 16 queries per pass over the store
        scan_multi_kernel<false><<<grid, kMWaves * 64, sizeof(MultiLds), st>>>(store_dev, n_rows, pass.at(queries_dev, dim), pass.nq, k_eff, cand,
                                                                              nullptr, 0, nullptr);
        HMM_LAUNCH_CHECK();
        topk_final_multi_kernel<<<pass.nq, 1024, 0, st>>>(cand, grid, k_eff, k_eff, pass.at(idx_out_dev, k), pass.at(sim_out_dev, k),
                                                       pass.at(n_out_dev, 1), k, nullptr);
        HMM_LAUNCH_CHECK();
        return HMM_OK;
    });
}

// ------------------------------------------------------------------------------------------------------
// Per-event top-k for a batch of questions: the pass above with SIMS_OUT, then segment_topk_kernel over an (event, query) grid
// (cosine_topk.hip).  The similarities of 16 questions are 64 B per 4096-B row read.
// ------------------------------------------------------------------------------------------------------
extern "C" int hmm_cosine_topk_segmented(const float* store_dev, int64_t n_rows, int dim, const float* query_dev,
                                         const int64_t* seg_offsets_dev, int n_segments, int k,
                                         int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                         void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream);

static int64_t multi_sims_stride(int64_t n_rows) { return (n_rows + kMTileRows - 1) / kMTileRows * kMTileRows; }

// The same for every n_queries and every k: one pass of 16 questions, which also covers the one-question scans behind k > 64.
extern "C" size_t hmm_cosine_topk_segmented_multi_workspace_bytes(int64_t n_rows, int n_segments, int n_queries, int k) {
    if (n_rows < 1 || n_segments < 1 || n_queries < 1 || k < 1) return 0;
    return align_up((size_t)kMQ * multi_sims_stride(n_rows) * sizeof(float), 256) + 256;  // + 256: margin only -- no kernel touches it
}

extern "C" int hmm_cosine_topk_segmented_multi(const float* store_dev, int64_t n_rows, int dim, const float* queries_dev,
                                               int n_queries, const int64_t* seg_offsets_dev, int n_segments, int k,
                                               int64_t* idx_out_dev, float* sim_out_dev, int32_t* n_out_dev,
                                               void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "cosine_topk_segmented_multi: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(n_rows >= 1 && n_rows < (int64_t)0xFFFFFFFFll, HMM_E_INVALID, "cosine_topk_segmented_multi: n_rows=%lld out of range",
                (long long)n_rows);
    HMM_REQUIRE(n_queries >= 1 && n_segments >= 1 && k >= 1 && k <= 1024, HMM_E_INVALID,
                "cosine_topk_segmented_multi: need n_queries >= 1, n_segments >= 1 and 1 <= k <= 1024 (got %d, %d, k=%d)", n_queries,
                n_segments, k);
    HMM_REQUIRE(store_dev && queries_dev && seg_offsets_dev && idx_out_dev && sim_out_dev && n_out_dev && workspace_dev, HMM_E_INVALID,
                "cosine_topk_segmented_multi: null pointer");
    HMM_REQUIRE(((uintptr_t)store_dev & 15) == 0 && ((uintptr_t)queries_dev & 15) == 0 && ((uintptr_t)workspace_dev & 15) == 0,
                HMM_E_INVALID, "cosine_topk_segmented_multi: store/queries/workspace must be 16-byte aligned");
    const size_t need = hmm_cosine_topk_segmented_multi_workspace_bytes(n_rows, n_segments, n_queries, k);
    HMM_REQUIRE(workspace_bytes >= need, HMM_E_WORKSPACE, "cosine_topk_segmented_multi: workspace %zu < required %zu", workspace_bytes,
                need);
    const size_t per_query = (size_t)n_segments * k;
    if (k > kMMaxK) {                                              // large k: one ordinary per-event scan per query
        for (int qi = 0; qi < n_queries; ++qi) {
            const int rc = hmm_cosine_topk_segmented(store_dev, n_rows, dim, queries_dev + (size_t)qi * dim, seg_offsets_dev, n_segments,
                                                     k, idx_out_dev + qi * per_query, sim_out_dev + qi * per_query,
                                                     n_out_dev + (size_t)qi * n_segments, workspace_dev, workspace_bytes, stream);
            if (rc != HMM_OK) return rc;
        }
        return HMM_OK;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HMM_ENSURE_DYN_LDS(scan_multi_kernel<true>, (int)sizeof(MultiLds));
    const int grid = multi_grid(n_rows);
    const int64_t stride = multi_sims_stride(n_rows);
    float* sims = static_cast<float*>(workspace_dev);
    return for_each_pass(n_queries, [&](const QuestionPass& pass) -> int {       // 16 queries per pass over the store
        scan_multi_kernel<true><<<grid, kMWaves * 64, sizeof(MultiLds), st>>>(store_dev, n_rows, pass.at(queries_dev, dim), pass.nq, k, nullptr,
                                                                             sims, stride, nullptr);
        HMM_LAUNCH_CHECK();
        launch_segment_topk(sims, stride, pass.nq, n_rows, seg_offsets_dev, n_segments, k, pass.at(idx_out_dev, per_query),
                            pass.at(sim_out_dev, per_query), pass.at(n_out_dev, n_segments), st);
        HMM_LAUNCH_CHECK();
        return HMM_OK;
    });
}

// ------------------------------------------------------------------------------------------------------
// The batched scans through the bf16 shadow (hmm_cosine_topk_multi_prefilter, hmm_cosine_topk_segmented_multi_prefilter): the
// scheme of cosine_topk_prefilter.hip for 16 questions per pass, 2048 B per row streamed instead of 4096.
//
//   pass 1   shadow_multi_kernel: s~(r, q) = dot(shadow_r, q) / ||q|| on v_mfma_f32_16x16x32_bf16.  The shadow rows are the A
//            operand, read straight into registers: lane (r16, g) of a wave holds, for step t of 32, the 16 bytes (8 bf16)
//            32 t + 8 g .. + 7 of row r16; one load instruction covers 16 rows x 64 B, two consecutive ones whole 128-B lines.  A
//            wave keeps one tile (16 rows, 128 registers) and refills register t for the next tile as soon as step t has used
//            it: 31 loads (31 KiB) per wave stay in flight behind a counted vmcnt, 8 waves per CU.  The questions are the B
//            operand, each split into bf16 hi = bf16(q) and lo = bf16(q - hi), two MFMAs per step; the 64 KiB of fragments live
//            in LDS in fragment order ([step][lane] x 16 B: a wave's read is one contiguous KiB, conflict-free) -- two
//            ds_read_b128 per KiB of rows streamed, a fifth of the LDS bandwidth at the HBM row rate -- which leaves the registers
//            to the row stream.  Selection (or the similarities-out mode) is scan_multi_kernel's.
//   pass 2   flat: multi_prefilter_final_kernel, one workgroup per question: threshold t = the k-th largest s~, candidates = the
//            rows with s~ >= t - 2 eps, re-scored by multi_rescore_tile and ranked.  A saturated list or more candidates than
//            the buffer holds raises ONE flag for the pass, and the exact pass (scan_multi_kernel<false> +
//            topk_final_multi_kernel, both conditional on that flag) answers for all its questions.
//            per event: segment_prefilter_kernel<.., TileRescore> over (event, question): threshold inside the event, candidates re-scored,
//            every row of the event when the candidates do not fit.
//   Re-scoring.  multi_rescore_tile gathers up to 16 candidate rows of the fp32 store into the A layout of scan_multi_kernel and
//            runs its sequence (multi_slice_mac / multi_tile_sims above) with the question in its own slot of the B operand and
//            zeros elsewhere: the bits of hmm_cosine_topk_multi, which depend neither on the row's place nor on the slot
//            (tests/test_gpu_segments_multi.py).
//   Error bound.  Shadow element x~ = (x / ||x||)(1 + d), |d| <= 2^-8 (as cosine_topk_prefilter.hip takes it; round to nearest
//            gives 2^-9): |dot(x~, q) - dot(x / ||x||, q)| <= 2^-8 (1 + 2^-8) ||q||                          -> 0.003922
//            question: hi + lo = q (1 + e), |e| <= 2^-9 * 2^-9 (+ one fp32 rounding of q - hi, exact here) -> 2^-16 = 0.000016
//            the bf16 x bf16 products are exact in fp32; they are summed in fp32 inside the MFMA and along 32 steps, K = 1024
//            terms per chain: at most 1024 * 2^-23 * sum |x~_i q_i| / ||q|| (truncating adds assumed)   -> 0.000123
//            1 / ||q|| in fp32 and the final product: 3 * 2^-24                                             -> 0.0000002
//            total |s~ - s| < 0.004061 < eps = 0.0042.  The candidate argument is that of cosine_topk_prefilter.hip:14-17.
// ------------------------------------------------------------------------------------------------------
namespace hmm {

constexpr float kMPEps = 0.0042f;                   // |s~ - s| on this route: the error bound above
constexpr int kSWaves = 8;                          // two waves per SIMD: ~150 registers each (128 of them one tile of rows)
using ShadowMultiDealing = RowDealing<kMTileRows, kSWaves>;     // shadow_multi_kernel: one tile per wave and round
constexpr int kSSteps = 32;                         // MFMA steps per tile: 32 bf16 of K each
constexpr int kSCap = 256;                          // candidate keys per query and workgroup (>= 64 + ShadowMultiDealing::kBlockRows, power of two)
constexpr int kMPFinalThreads = 512;
constexpr int kMPMinRows = 16384;                   // flat dispatch limit: hmm_cosine_topk_prefilter's, NOT yet measured for a batch
constexpr int kMPMinSegRows = 128;                  // per-event dispatch limit, rows per event on average: inherited likewise, NOT yet measured

struct ShadowLds {
    uint4 bhi[kSSteps][64];                         // 32768 B
    uint4 blo[kSSteps][64];                         // 32768 B
    uint64_t keys[kMQ][kSCap];                      // 32768 B
    uint64_t tau[kMQ];
    float inv_qlen[kMQ];
    int cnt[kMQ];
    int need;
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <bool SIMS_OUT>
__global__ __launch_bounds__(kSWaves * 64) void shadow_multi_kernel(const uint4* __restrict__ shadow, int64_t n_rows,
                                                                    const float* __restrict__ queries, int n_q, int kk,
                                                                    uint64_t* __restrict__ out, float* __restrict__ sims_out,
                                                                    int64_t sims_stride, int* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    ShadowLds& L = *reinterpret_cast<ShadowLds*>(smem_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    if (flag != nullptr && blockIdx.x == 0 && tid == 0) *flag = 0;            // the pass's fallback flag (raised by the finish)

    // 1 / ||q||: wave w takes questions w and w + 8, lane l the floats 4 (64 j + l)
    for (int qi = wave; qi < kMQ; qi += kSWaves) {
        float qs = 0.f;
        if (qi < n_q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) multi_sumsq4(qs, *reinterpret_cast<const f32x4*>(queries + (size_t)qi * 1024 + 4 * (64 * j + lane)));
        }
        qs = wave_sum(qs);
        if (lane == 0) L.inv_qlen[qi] = 1.0f / sqrtf(qs);
    }
    // B fragments: entry (t, lane (q, g)) = bf16 hi / lo of q[32 t + 8 g .. + 7] (zeros past n_q)
    for (int i = tid; i < kSSteps * 64; i += kSWaves * 64) {
        const int t = i >> 6, l = i & 63, qi = l & 15, gg = l >> 4;
        bf16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) { hi[e] = (bf16_t)0.f; lo[e] = (bf16_t)0.f; }
        if (qi < n_q) {
            const float* p = queries + (size_t)qi * 1024 + 32 * t + 8 * gg;
            const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = e < 4 ? a[e & 3] : b[e & 3];
                hi[e] = (bf16_t)v;
                lo[e] = (bf16_t)(v - (float)hi[e]);
            }
        }
        L.bhi[t][l] = __builtin_bit_cast(uint4, hi);
        L.blo[t][l] = __builtin_bit_cast(uint4, lo);
    }
    if (tid < kMQ) { L.cnt[tid] = 0; L.tau[tid] = 0ull; }
    if (tid == 0) L.need = 0;
    __syncthreads();
    const float my_inv_qlen = L.inv_qlen[r16];

    const int64_t n_tiles = (n_rows + kMTileRows - 1) / kMTileRows;
    const int64_t n_waves = (int64_t)gridDim.x * kSWaves;
    const int64_t wave_gid = (int64_t)blockIdx.x * kSWaves + wave;
    const int64_t n_rounds = (n_tiles + n_waves - 1) / n_waves;   // same for every wave of the grid
    auto src_of = [&](int64_t round) {                            // lane's 16 B of step 0; step t is + 4 t (rows past the end: clamped)
        int64_t row = ShadowMultiDealing::first_row(wave_gid, round, n_waves) + r16;
        row = row < n_rows ? row : n_rows - 1;
        return reinterpret_cast<const u32x4*>(shadow) + row * 128 + g;
    };
    u32x4 x[kSSteps];
    {
        const u32x4* p = src_of(0);
#pragma unroll
        for (int t = 0; t < kSSteps; ++t) x[t] = __builtin_nontemporal_load(p + 4 * t);
    }
    for (int64_t round = 0; round < n_rounds; ++round) {
        const int64_t tile = ShadowMultiDealing::group(wave_gid, round, n_waves);
        const u32x4* pn = src_of(round + 1);                      // next tile (clamped past the end, never used then)
        asm volatile("" ::: "memory");                            // the B fragments are re-read from LDS every round: hoisted out of the
                                                                  // loop they would take 256 registers and spill the row stream
        f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
        for (int t = 0; t < kSSteps; ++t) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, x[t]);
            const bf16x8 bh = __builtin_bit_cast(bf16x8, L.bhi[t][lane]);
            const bf16x8 bl = __builtin_bit_cast(bf16x8, L.blo[t][lane]);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bh, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bl, acc1, 0, 0, 0);
            x[t] = __builtin_nontemporal_load(pn + 4 * t);        // register t is free: the same step of the next tile
            __builtin_amdgcn_sched_barrier(0);                    // keep the load HERE: gathered behind the MFMAs, all 32 are waited for at once
        }
        const f32x4 acc = acc0 + acc1;                            // D layout: query r16, rows 4 g + j
        f32x4 sim4;
#pragma unroll
        for (int j = 0; j < 4; ++j) sim4[j] = acc[j] * my_inv_qlen;
        if constexpr (SIMS_OUT) {
            if (tile < n_tiles && r16 < n_q)
                *reinterpret_cast<f32x4*>(sims_out + r16 * sims_stride + tile * kMTileRows + 4 * g) = sim4;
            continue;
        }
        // lists sorted down to kk exactly as scan_multi_kernel sorts its lists down to k (multi_lists_round)
        multi_lists_round<ShadowMultiDealing, kSCap>(L, sim4, tile, n_tiles, n_rows, n_q, kk, round + 1 >= n_rounds || round == 0, wave, lane);
    }
    if constexpr (SIMS_OUT) return;
    multi_lists_flush<ShadowMultiDealing>(L, n_q, kk, out);
}

// Up to 16 rows of the fp32 store against the question in B slot `slot`, with the bits of scan_multi_kernel: lane (r16, g) passes
// row r16 of the gathered tile (nullptr: no row, zeros) and gets, where r16 == slot, the similarities of rows 4 g + 0..3.
// q_lds: the question's 1024 floats in LDS.  Two K slices per memory latency; not a bandwidth path.
__device__ __forceinline__ f32x4 multi_rescore_tile(const float* row, const float* q_lds, int slot, int lane) {
    const int r16 = lane & 15, g = lane >> 4;
    const bool mine = r16 == slot;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc0 = zero, acc1 = zero;
    float ss = 0.f, qss = 0.f;
#pragma unroll 1
    for (int sp = 0; sp < kMSlices / 2; ++sp) {
        f32x4 xa[8], xb[8], ba[8], bb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            xa[j] = row ? *reinterpret_cast<const f32x4*>(row + 256 * sp + 32 * g + 4 * j) : zero;
            xb[j] = row ? *reinterpret_cast<const f32x4*>(row + 256 * sp + 128 + 32 * g + 4 * j) : zero;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ba[j] = mine ? *reinterpret_cast<const f32x4*>(q_lds + 256 * sp + 32 * g + 4 * j) : zero;
            multi_sumsq4(qss, ba[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            bb[j] = mine ? *reinterpret_cast<const f32x4*>(q_lds + 256 * sp + 128 + 32 * g + 4 * j) : zero;
            multi_sumsq4(qss, bb[j]);
        }
        multi_slice_mac(xa, ba, acc0, acc1, ss);
        multi_slice_mac(xb, bb, acc0, acc1, ss);
    }
    return multi_tile_sims(acc0, acc1, ss, multi_len(qss), g);
}

// Flat finish, one workgroup per question of the pass.  lists: [question][n_blocks][kk] keys of shadow_multi_kernel.
__global__ __launch_bounds__(kMPFinalThreads) void multi_prefilter_final_kernel(const uint64_t* __restrict__ lists, int n_blocks, int k,
                                                                                int kk, const float* __restrict__ store,
                                                                                const float* __restrict__ queries,
                                                                                int64_t* __restrict__ idx_out, float* __restrict__ sim_out,
                                                                                int32_t* __restrict__ n_out, int k_stride,
                                                                                int* __restrict__ flag, int32_t* __restrict__ stats) {
    __shared__ uint64_t mx[kNumCU];
    __shared__ uint64_t s[kChunk];
    __shared__ uint32_t cand_row[kCandCap];
    __shared__ __attribute__((aligned(16))) float qs[1024];
    __shared__ int n_cand, n_sat;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, qi = blockIdx.x;
    const uint64_t* c = lists + (size_t)qi * n_blocks * kk;
    if (tid == 0) { n_cand = 0; n_sat = 0; }
    for (int t = tid; t < 256; t += kMPFinalThreads)
        *reinterpret_cast<f32x4*>(qs + 4 * t) = *reinterpret_cast<const f32x4*>(queries + (size_t)qi * 1024 + 4 * t);
    // the k lists with the largest maxima hold the k largest keys (every list keeps kk >= k entries): rank them
    rank_winning_lists<ShadowMultiDealing, kMPFinalThreads>(c, n_blocks, kk, k, mx, s);
    const uint64_t kth = s[k - 1];                                // 0 = fewer than k rows in all (the launcher excludes it)
    __syncthreads();
    const uint32_t thr = threshold_below(key_order(kth), kMPEps);
    // candidates: every entry at or above the threshold; a list whose LAST entry passes may have dropped some (saturated)
    for (int t = tid; t < n_blocks * kk; t += kMPFinalThreads) {
        const uint64_t key = c[t];
        if (key != 0ull && key_order(key) >= thr) {
            const int pos = atomicAdd(&n_cand, 1);
            if (pos < kCandCap) cand_row[pos] = (uint32_t)key_row(key);
            if (t % kk == kk - 1) atomicAdd(&n_sat, 1);
        }
    }
    __syncthreads();
    const int m = n_cand;
    const bool fall = kth == 0ull || n_sat > 0 || m > kCandCap;
    if (tid == 0) {
        if (fall) *flag = 1;                                      // one flag for the pass: the exact pass answers every question of it
        if (stats) { stats[2 * qi] = m; stats[2 * qi + 1] = n_sat; }
    }
    if (fall) return;                                             // block-uniform
    const int m_pad = pow2_at_least(m, 64);
    for (int t = m + tid; t < m_pad; t += kMPFinalThreads) s[t] = 0ull;
    const int r16 = lane & 15, g = lane >> 4;
    for (int tile = wave; tile * kMTileRows < m; tile += kMPFinalThreads / 64) {       // wave-uniform
        const int cc = tile * kMTileRows + r16;
        const float* row = cc < m ? store + (int64_t)cand_row[cc] * 1024 : nullptr;
        const f32x4 sim4 = multi_rescore_tile(row, qs, qi, lane);
        if (r16 == qi) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cj = tile * kMTileRows + 4 * g + j;
                if (cj < m) s[cj] = make_key(sim4[j], cand_row[cj]);
            }
        }
    }
    __syncthreads();
    top64_desc(s, m_pad);
    write_hits(s, k, k, idx_out + (size_t)qi * k_stride, sim_out + (size_t)qi * k_stride, n_out ? n_out + qi : nullptr);
}

// Per-event finish over an (event, question) grid: segment_prefilter_kernel (topk_select.h) with multi_rescore_tile as the
// re-scorer, in tiles of 16 candidate rows per wave; the question waits in LDS.
struct TileRescore {
    static constexpr float kEps = kMPEps;
    struct Lds { __attribute__((aligned(16))) float qs[1024]; };
    template <int THREADS>
    __device__ static __forceinline__ void stage(Lds& l, const float* __restrict__ queries, int y) {
        for (int t = threadIdx.x; t < 256; t += THREADS)
            *reinterpret_cast<f32x4*>(l.qs + 4 * t) = *reinterpret_cast<const f32x4*>(queries + (size_t)y * 1024 + 4 * t);
    }
    const float* qs;
    int y;
    __device__ __forceinline__ TileRescore(Lds& l, const float*, int y_) : qs(l.qs), y(y_) {}
    template <int THREADS, class RowOf>
    __device__ __forceinline__ void score(const float* __restrict__ rows, int take, RowOf row_of, uint64_t* out) const {
        const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
        for (int tile = threadIdx.x >> 6; tile * kMTileRows < take; tile += THREADS / 64) {        // wave-uniform trip count per wave
            const int cc = tile * kMTileRows + r16;
            const f32x4 sim4 = multi_rescore_tile(cc < take ? rows + row_of(cc) * 1024 : nullptr, qs, y, lane);
            if (r16 == y) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int cj = tile * kMTileRows + 4 * g + j;
                    if (cj < take) out[cj] = make_key(sim4[j], (uint32_t)row_of(cj));
                }
            }
        }
    }
};

static int shadow_multi_grid(int64_t n_rows) {                 // one workgroup per CU (its LDS fills the CU), 128 rows per round
    return ShadowMultiDealing::grid(n_rows, kNumCU);
}

struct MultiPrefilterPlan { size_t exact, off_lists, off_flag, total; };

static MultiPrefilterPlan multi_prefilter_plan(int64_t n_rows, int n_queries, int k) {
    MultiPrefilterPlan p{};
    // The exact function runs inside the first part.  Its own query is not monotone in n_rows beyond k = 64 (the one-question scan's
    // plan changes shape with min(k, n_rows)), so this part is an envelope of it that is: the batched pass's lists, and beyond 64 the
    // one-question scan's own envelope (cosine_topk_workspace_envelope, beside its plan in cosine_topk.hip).
    const int64_t k_eff = k < n_rows ? k : n_rows;
    size_t part = align_up((size_t)kMQ * multi_grid(n_rows) * (size_t)(k_eff < kMMaxK ? k_eff : kMMaxK) * 8, 256) + 256;
    if (k_eff > kMMaxK) {
        const size_t one = cosine_topk_workspace_envelope(n_rows, k);
        part = part > one ? part : one;
    }
    const size_t exact = hmm_cosine_topk_multi_workspace_bytes(n_rows, n_queries, k);
    p.exact = part > exact ? part : exact;
    p.off_lists = align_up(p.exact, 256);
    p.off_flag = p.off_lists + (size_t)kMQ * kNumCU * kMMaxK * 8;                         // [16][<= 256 workgroups][<= 64] keys
    p.total = p.off_flag + 256;                                                          // the flag uses 4 of these 256 bytes
    return p;
}

}  // namespace hmm

extern "C" size_t hmm_cosine_topk_multi_prefilter_workspace_bytes(int64_t n_rows, int n_queries, int k) {
    if (n_rows < 1 || n_queries < 1 || k < 1) return 0;
    return multi_prefilter_plan(n_rows, n_queries, k).total;
}

extern "C" int hmm_cosine_topk_multi_prefilter(const float* store_dev, const void* shadow_dev, int64_t n_rows, int dim,
                                               const float* queries_dev, int n_queries, int k, int64_t* idx_out_dev, float* sim_out_dev,
                                               int32_t* n_out_dev, int32_t* stats_out_dev, void* workspace_dev, size_t workspace_bytes,
                                               hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "cosine_topk_multi_prefilter: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(n_rows >= 1 && n_rows < (int64_t)0xFFFFFFFFll, HMM_E_INVALID, "cosine_topk_multi_prefilter: n_rows=%lld out of range",
                (long long)n_rows);
    HMM_REQUIRE(n_queries >= 1 && k >= 1, HMM_E_INVALID, "cosine_topk_multi_prefilter: n_queries=%d k=%d", n_queries, k);
    HMM_REQUIRE(store_dev && shadow_dev && queries_dev && idx_out_dev && sim_out_dev && workspace_dev, HMM_E_INVALID,
                "cosine_topk_multi_prefilter: null pointer");
    HMM_REQUIRE(((uintptr_t)store_dev & 15) == 0 && ((uintptr_t)shadow_dev & 15) == 0 && ((uintptr_t)queries_dev & 15) == 0 &&
                    ((uintptr_t)workspace_dev & 15) == 0,
                HMM_E_INVALID, "cosine_topk_multi_prefilter: store / shadow / queries / workspace must be 16-byte aligned");
    const MultiPrefilterPlan p = multi_prefilter_plan(n_rows, n_queries, k);
    HMM_REQUIRE(workspace_bytes >= p.total, HMM_E_WORKSPACE, "cosine_topk_multi_prefilter: workspace %zu < required %zu", workspace_bytes,
                p.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace_dev);
    // small stores, large k: nothing to win (or no list machinery): the exact pass is the whole call
    if (k > kMMaxK || n_rows < kMPMinRows || n_rows <= k) {
        if (stats_out_dev) HMM_HIP_CHECK(hipMemsetAsync(stats_out_dev, 0xFF, (size_t)n_queries * 2 * sizeof(int32_t), st));  // -1, -1
        return hmm_cosine_topk_multi(store_dev, n_rows, dim, queries_dev, n_queries, k, idx_out_dev, sim_out_dev, n_out_dev, ws, p.exact,
                                     stream);
    }
    HMM_ENSURE_DYN_LDS(shadow_multi_kernel<false>, (int)sizeof(ShadowLds));
    HMM_ENSURE_DYN_LDS(scan_multi_kernel<false>, (int)sizeof(MultiLds));
    const int kk = prefilter_list_len(k);
    const int grid = shadow_multi_grid(n_rows), exact_grid = multi_grid(n_rows);
    uint64_t* lists = reinterpret_cast<uint64_t*>(ws + p.off_lists);
    uint64_t* cand = reinterpret_cast<uint64_t*>(ws);
    int* flag = reinterpret_cast<int*>(ws + p.off_flag);
    return for_each_pass(n_queries, [&](const QuestionPass& pass) -> int {       // 16 queries per pass over the shadow
        const int nq = pass.nq;
        const float* qp = pass.at(queries_dev, dim);
        int64_t* io = pass.at(idx_out_dev, k);
        float* so = pass.at(sim_out_dev, k);
        int32_t* no = pass.at(n_out_dev, 1);
        shadow_multi_kernel<false><<<grid, kSWaves * 64, sizeof(ShadowLds), st>>>(static_cast<const uint4*>(shadow_dev), n_rows, qp, nq, kk,
                                                                                 lists, nullptr, 0, flag);
        HMM_LAUNCH_CHECK();
        multi_prefilter_final_kernel<<<nq, kMPFinalThreads, 0, st>>>(lists, grid, k, kk, store_dev, qp, io, so, no, k, flag,
                                                                     pass.at(stats_out_dev, 2));
        HMM_LAUNCH_CHECK();
        // the exact pass, conditional on the flag (its workgroups return at once otherwise)
        scan_multi_kernel<false><<<exact_grid, kMWaves * 64, sizeof(MultiLds), st>>>(store_dev, n_rows, qp, nq, k, cand, nullptr, 0, flag);
        HMM_LAUNCH_CHECK();
        topk_final_multi_kernel<<<nq, 1024, 0, st>>>(cand, exact_grid, k, k, io, so, no, k, flag);
        HMM_LAUNCH_CHECK();
        return HMM_OK;
    });
}

extern "C" size_t hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes(int64_t n_rows, int n_segments, int n_queries, int k) {
    return hmm_cosine_topk_segmented_multi_workspace_bytes(n_rows, n_segments, n_queries, k);      // s~ of one pass, 16 x 4 B per row
}

extern "C" int hmm_cosine_topk_segmented_multi_prefilter(const float* store_dev, const void* shadow_dev, int64_t n_rows, int dim,
                                                         const float* queries_dev, int n_queries, const int64_t* seg_offsets_dev,
                                                         int n_segments, int k, int64_t* idx_out_dev, float* sim_out_dev,
                                                         int32_t* n_out_dev, int32_t* stats_out_dev, void* workspace_dev,
                                                         size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "cosine_topk_segmented_multi_prefilter: dim must be %d, got %d", HMM_FEATURE_DIM,
                dim);
    HMM_REQUIRE(n_rows >= 1 && n_rows < (int64_t)0xFFFFFFFFll, HMM_E_INVALID,
                "cosine_topk_segmented_multi_prefilter: n_rows=%lld out of range", (long long)n_rows);
    HMM_REQUIRE(n_queries >= 1 && n_segments >= 1 && k >= 1 && k <= 1024, HMM_E_INVALID,
                "cosine_topk_segmented_multi_prefilter: need n_queries >= 1, n_segments >= 1 and 1 <= k <= 1024 (got %d, %d, k=%d)",
                n_queries, n_segments, k);
    HMM_REQUIRE(store_dev && shadow_dev && queries_dev && seg_offsets_dev && idx_out_dev && sim_out_dev && n_out_dev && workspace_dev,
                HMM_E_INVALID, "cosine_topk_segmented_multi_prefilter: null pointer");
    HMM_REQUIRE(((uintptr_t)store_dev & 15) == 0 && ((uintptr_t)shadow_dev & 15) == 0 && ((uintptr_t)queries_dev & 15) == 0 &&
                    ((uintptr_t)workspace_dev & 15) == 0,
                HMM_E_INVALID, "cosine_topk_segmented_multi_prefilter: store / shadow / queries / workspace must be 16-byte aligned");
    const size_t need = hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes(n_rows, n_segments, n_queries, k);
    HMM_REQUIRE(workspace_bytes >= need, HMM_E_WORKSPACE, "cosine_topk_segmented_multi_prefilter: workspace %zu < required %zu",
                workspace_bytes, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // no tournament beyond 64 keys, and nothing to win on events of a few dozen rows: the exact function is the whole call
    if (k > kMMaxK || n_rows / n_segments < kMPMinSegRows) {
        if (stats_out_dev) HMM_HIP_CHECK(hipMemsetAsync(stats_out_dev, 0xFF, 2 * sizeof(int32_t), st));                        // -1, -1
        return hmm_cosine_topk_segmented_multi(store_dev, n_rows, dim, queries_dev, n_queries, seg_offsets_dev, n_segments, k, idx_out_dev,
                                               sim_out_dev, n_out_dev, workspace_dev, workspace_bytes, stream);
    }
    if (stats_out_dev) HMM_HIP_CHECK(hipMemsetAsync(stats_out_dev, 0, 2 * sizeof(int32_t), st));
    HMM_ENSURE_DYN_LDS(shadow_multi_kernel<true>, (int)sizeof(ShadowLds));
    const int grid = shadow_multi_grid(n_rows);
    const int64_t stride = multi_sims_stride(n_rows);
    float* sims = static_cast<float*>(workspace_dev);
    const size_t per_query = (size_t)n_segments * k;
    const bool small = segments_are_small(n_rows, n_segments, k);  // the two shapes of segment_topk_kernel, for the same reason
    return for_each_pass(n_queries, [&](const QuestionPass& pass) -> int {       // 16 queries per pass over the shadow
        const float* qp = pass.at(queries_dev, dim);
        shadow_multi_kernel<true><<<grid, kSWaves * 64, sizeof(ShadowLds), st>>>(static_cast<const uint4*>(shadow_dev), n_rows, qp, pass.nq, 0,
                                                                                nullptr, sims, stride, nullptr);
        HMM_LAUNCH_CHECK();
        const dim3 sgrid(n_segments, pass.nq);
        if (small)
            segment_prefilter_kernel<kSmallSegChunk, 256, TileRescore><<<sgrid, 256, 0, st>>>(
                sims, stride, seg_offsets_dev, k, store_dev, qp, pass.at(idx_out_dev, per_query), pass.at(sim_out_dev, per_query),
                pass.at(n_out_dev, n_segments), stats_out_dev);
        else
            segment_prefilter_kernel<kChunk, 512, TileRescore><<<sgrid, 512, 0, st>>>(
                sims, stride, seg_offsets_dev, k, store_dev, qp, pass.at(idx_out_dev, per_query), pass.at(sim_out_dev, per_query),
                pass.at(n_out_dev, n_segments), stats_out_dev);
        HMM_LAUNCH_CHECK();
        return HMM_OK;
    });
}
