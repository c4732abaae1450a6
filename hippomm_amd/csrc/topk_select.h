// The selection layer of the retrieval kernels (cosine_topk.hip, cosine_topk_prefilter.hip, cosine_topk_multi.hip): everything a
// scan route does with order keys once a similarity exists, written once.
//   keys        make_key / key_row / key_sim / key_order, write_hits (keys -> idx, sim, n with padding), threshold_below;
//   queries     load_query_frags: a lane's part of the query and ||q||, in the fma order that defines the bits;
//   fold_topk   the best k of a run of any length through one LDS chunk, carrying the running best;
//   RowDealing  how a streaming kernel deals rows to the waves of its grid AND the inverse of that (row -> workgroup); the kernel
//               and its finish take both from the same descriptor;
//   rank_winning_lists   "the k lists with the largest maxima hold the answer" (see there);
//   compact_block_list / multi_lists_*   the block-local candidate lists of the streaming kernels;
//   segment_prefilter_kernel   the per-event finish of the shadow routes, templated on the re-scorer;
//   for_each_pass   the questions of a batched call, kMQ per pass over the store.
// Builds on the best-64 tournament (topk_tournament.h).
#pragma once
#include "hmm_common.h"
#include "topk_tournament.h"
#include "cosine_topk_shared.h"

namespace hmm {

// ---- order keys ------------------------------------------------------------------------------------------------------------------
// (order_bits(sim) << 32) | row: "larger key" == "better, higher row first on ties, NaN first"; 0 is the padding key.
__device__ __forceinline__ uint64_t make_key(float sim, uint32_t row) { return ((uint64_t)order_bits(sim) << 32) | (uint64_t)row; }
__device__ __forceinline__ int64_t key_row(uint64_t key) { return (int64_t)(key & 0xFFFFFFFFull); }
__device__ __forceinline__ uint32_t key_order(uint64_t key) { return (uint32_t)(key >> 32); }
__device__ __forceinline__ float key_sim(uint64_t key) { return order_bits_inverse(key_order(key)); }

// s[0 .. k_out): sorted keys -> idx[t], sim[t]; slots k_out .. k_pad get (-1, 0.0f); *n_out = k_out where n_out is given.  The
// per-event outputs are padded to k (k_pad = k), the flat ones are not (k_pad = k_out).  Called by every thread of the workgroup.
__device__ __forceinline__ void write_hits(const uint64_t* s, int k_out, int k_pad, int64_t* __restrict__ idx, float* __restrict__ sim,
                                           int32_t* __restrict__ n_out) {
    if (threadIdx.x == 0 && n_out) *n_out = k_out;
    for (int t = threadIdx.x; t < k_pad; t += blockDim.x) {
        const bool ok = t < k_out;
        idx[t] = ok ? key_row(s[t]) : -1;
        sim[t] = ok ? key_sim(s[t]) : 0.0f;
    }
}

// The order word of (similarity of `order` - 2 eps): every row whose exact similarity can reach the one behind `order` has an
// approximate key at or above it (cosine_topk_prefilter.hip, error bound).  A NaN key -> 0xFFFFFFFF: only NaN rows pass.
__device__ __forceinline__ uint32_t threshold_below(uint32_t order, float eps) {
    return order_bits(order_bits_inverse(order) - 2.0f * eps);
}

constexpr int kCandCap = 1024;       // candidate rows a finish kernel re-scores itself (its LDS list of rows)
constexpr int kListMaxK = 64;        // the tournament's width: no list machinery beyond k = 64

// Entries a block keeps on the shadow routes: at least twice k and at least 32, so that a handful of near-ties inside one block
// (k = 1: ANY second candidate) does not saturate its list; 64 at most (the tournament's width).
inline int prefilter_list_len(int k) {
    const int kk = 2 * k < 32 ? 32 : 2 * k;
    return kk > kListMaxK ? kListMaxK : kk;
}

// ---- the query in a wave's registers ---------------------------------------------------------------------------------------------
// Lane l holds the float4 at columns 4 (64 j + l), j = 0..3; returns ||q|| = sqrtf(wave_sum(sum q^2)) with the squares summed in
// exactly this order -- exact_row_sim and every streaming kernel divide by this value, so the order is part of a similarity's bits.
__device__ __forceinline__ float load_query_frags(const float4* __restrict__ query, int lane, float4 (&q)[4]) {
    float qs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = query[j * 64 + lane];
        qs = fmaf(q[j].x, q[j].x, qs); qs = fmaf(q[j].y, q[j].y, qs);
        qs = fmaf(q[j].z, q[j].z, qs); qs = fmaf(q[j].w, q[j].w, qs);
    }
    return sqrtf(wave_sum(qs));
}

// ---- sorts in LDS ----------------------------------------------------------------------------------------------------------------
// Descending bitonic sort of the first n2 (power of two) keys in LDS by the whole block.
__device__ __forceinline__ void bitonic_sort_desc_rt(uint64_t* s, int n2) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n2 >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (j - 1));
                const int l = i + j;
                const bool desc = (i & k) == 0;
                const uint64_t a = s[i], b = s[l];
                if ((a < b) == desc) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
    }
}

// The best k of n keys, sorted descending at s[0 ..), through one LDS chunk s[0 .. CHUNK): the run is folded in pieces, the best k
// so far carried at the front.  fill(base, have, take) writes the keys of piece [base, base + take) to s[have .. have + take); it
// is called by EVERY thread of the workgroup (the re-scoring producers are wave-cooperative) and needs no barrier of its own.
// ANY_K: k may exceed 64 (full sort of the chunk instead of the best-64 tournament).  n >= 1.  Ends on a barrier.
template <int CHUNK, int THREADS, bool ANY_K, class Fill>
__device__ __forceinline__ void fold_topk(uint64_t* s, int64_t n, int k, Fill fill) {
    int have = 0;                                              // best keys carried from earlier pieces, at s[0..have)
    int64_t base = 0;
    do {
        const int64_t left = n - base;
        const int take = (int)(left < (int64_t)(CHUNK - have) ? left : (int64_t)(CHUNK - have));
        const int total = have + take;
        const int n2 = pow2_at_least(total, 64);
        for (int t = total + threadIdx.x; t < n2; t += THREADS) s[t] = 0ull;
        fill(base, have, take);
        __syncthreads();
        if (!ANY_K || k <= 64) top64_desc(s, n2);              // best-64 tournament: s[0..63] sorted, the rest clobbered
        else                   bitonic_sort_desc_rt(s, n2);
        have = total < k ? total : k;
        base += take;
    } while (base < n);
}

// ---- row dealing -----------------------------------------------------------------------------------------------------------------
// A streaming kernel deals the store to the waves of its grid in groups of ROWS consecutive rows, group after group, wave after
// wave: group p belongs to wave p % n_waves (n_waves = workgroups x WAVES) -- at any moment the waves of the chip read one
// contiguous window of the store.  The finish kernels need the inverse, the workgroup whose list holds row r.  Both directions
// live here, and a kernel and its finish name the same descriptor: change ROWS or WAVES and both follow.
template <int ROWS, int WAVES>
struct RowDealing {
    static constexpr int kRows = ROWS, kWaves = WAVES, kBlockRows = ROWS * WAVES;
    // the group that wave `wave` of the grid takes in iteration `it`, and its first row
    __device__ static __forceinline__ int64_t group(int64_t wave, int64_t it, int64_t n_waves) { return wave + it * n_waves; }
    __device__ static __forceinline__ int64_t first_row(int64_t wave, int64_t it, int64_t n_waves) { return group(wave, it, n_waves) * ROWS; }
    // iterations after which every row is dealt: the same trip count for every wave
    __device__ static __forceinline__ int64_t iterations(int64_t n_rows, int64_t n_waves) { return (n_rows + n_waves * ROWS - 1) / (n_waves * ROWS); }
    // the workgroup that scanned row `row` on a grid of n_blocks workgroups (rows are below 2^32: the low word of a key)
    __device__ static __forceinline__ int block_of_row(uint32_t row, int n_blocks) {
        return (int)(((row / (uint32_t)ROWS) % (uint32_t)(n_blocks * WAVES)) / (uint32_t)WAVES);
    }
    // workgroups that give every wave at least one group, max_blocks at most
    static int grid(int64_t n_rows, int max_blocks) {
        const int64_t blocks = (n_rows + kBlockRows - 1) / kBlockRows;
        return (int)(blocks < max_blocks ? blocks : max_blocks);
    }
};
using ScanDealing = RowDealing<2, 4>;              // scan_topk_body, scan_sims_deferred_kernel: a pair of fp32 rows per wave
using PrefilterDealing = RowDealing<4, 4>;         // prefilter_topk_kernel, prefilter_sims_deferred_kernel: four shadow rows per wave

// ---- "the k lists with the largest maxima hold the answer" -----------------------------------------------------------------------
// Every workgroup of a streaming pass left its best `len` keys, sorted and 0-padded, at lists[b * len ..].  The global top-k can
// only contain keys of the k workgroups with the largest maxima: a key below the k-th largest maximum has k better keys (those
// maxima) ahead of it.  So: rank the maxima, map each winner's row back to the workgroup that scanned it (DEAL), gather those
// lists, rank again.  k <= 64 and k * len <= 4096 (both rankings are best-64 tournaments).
//   rank_list_maxima        mx[0 .. 64) = the largest maxima, sorted (mx holds pow2_at_least(n_blocks, 64) keys);
//   gather_winning_lists    s[0 .. m2) = the lists of the k winners (m2 returned); ends on a barrier;
//   rank_winning_lists      both, then s[0 .. 64) = the largest keys of all lists, sorted.
template <int THREADS>
__device__ __forceinline__ void rank_list_maxima(const uint64_t* __restrict__ lists, int n_blocks, int len, uint64_t* mx) {
    const int n2 = pow2_at_least(n_blocks, 64);
    for (int t = threadIdx.x; t < n2; t += THREADS) mx[t] = t < n_blocks ? lists[(size_t)t * len] : 0ull;
    __syncthreads();
    top64_desc(mx, n2);
}
template <class DEAL, int THREADS>
__device__ __forceinline__ int gather_winning_lists(const uint64_t* __restrict__ lists, const uint64_t* mx, int n_blocks, int len, int k,
                                                    uint64_t* s) {
    const int n_win = n_blocks < k ? n_blocks : k;
    const int m2 = pow2_at_least(n_win * len, 64);
    for (int t = threadIdx.x; t < m2; t += THREADS) {
        uint64_t key = 0ull;
        if (t < n_win * len) {
            const uint64_t top = mx[t / len];
            if (top != 0ull) key = lists[(size_t)DEAL::block_of_row((uint32_t)key_row(top), n_blocks) * len + (t % len)];
        }
        s[t] = key;
    }
    __syncthreads();
    return m2;
}
template <class DEAL, int THREADS>
__device__ __forceinline__ void rank_winning_lists(const uint64_t* __restrict__ lists, int n_blocks, int len, int k, uint64_t* mx,
                                                   uint64_t* s) {
    rank_list_maxima<THREADS>(lists, n_blocks, len, mx);
    top64_desc(s, gather_winning_lists<DEAL, THREADS>(lists, mx, n_blocks, len, k, s));
}

// ---- block-local candidate lists of the streaming kernels ------------------------------------------------------------------------
// One question (scan_topk_body, prefilter_topk_kernel): the waves append the keys of their rows to cand[0 .. count) with an LDS
// atomic; this cuts the list back to its best k, sorted.  Called by every thread of a 256-thread workgroup, block-uniformly,
// whenever the list could overflow before the next call and once at the end.  ANY_K: k may exceed 64.
template <bool ANY_K>
__device__ __forceinline__ void compact_block_list(uint64_t* cand, int& count, int k) {
    __syncthreads();
    const int n = count;
    const int n2 = pow2_at_least(n, 64);
    for (int t = n + threadIdx.x; t < n2; t += 256) cand[t] = 0ull;
    __syncthreads();
    if (!ANY_K || k <= 64) top64_desc<false>(cand, n2);        // block-uniform; leaves cand[0..63] sorted
    else                   bitonic_sort_desc_rt(cand, n2);
    if (threadIdx.x == 0) count = n < k ? n : k;
    __syncthreads();
}
// the workgroup's list, 0-padded to k keys
__device__ __forceinline__ void flush_block_list(const uint64_t* cand, int count, int k, uint64_t* __restrict__ out) {
    for (int t = threadIdx.x; t < k; t += 256) out[(int64_t)blockIdx.x * k + t] = t < count ? cand[t] : 0ull;
}

constexpr int kMQ = 16;                 // questions per pass of the batched kernels
constexpr int kMTileRows = 16;          // rows per wave per round of the batched kernels (one MFMA tile)

// A raw workgroup barrier that leaves LDS-DMA in flight (__syncthreads() would drain vmcnt to 0).
__device__ __forceinline__ void multi_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// Descending bitonic sort, by ONE wave, of the first n2 (power of two) keys of NL lists at once: the lists'
// compare-exchange steps are independent, so walking them in lockstep overlaps their LDS round trips (a single
// list is latency-bound: ~26 us for 512 keys).
template <int NL>
__device__ __forceinline__ void wave_bitonic_desc(uint64_t* (&s)[NL], int n2, int lane) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n2 >> 1); t += 64) {
                const int i = 2 * t - (t & (j - 1));
                const int l = i + j;
                const bool desc = (i & k) == 0;
                uint64_t a[NL], b[NL];
#pragma unroll
                for (int q = 0; q < NL; ++q) { a[q] = s[q][i]; b[q] = s[q][l]; }
#pragma unroll
                for (int q = 0; q < NL; ++q)
                    if ((a[q] < b[q]) == desc) { s[q][i] = b[q]; s[q][l] = a[q]; }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// kMQ questions (scan_multi_kernel, shadow_multi_kernel): every question has a list of CAP keys in LDS and a threshold tau = its
// current k-th best; only keys above the threshold are appended.  L: the kernel's LDS block with keys[kMQ][CAP], tau[kMQ],
// cnt[kMQ] and need.  DEAL: the kernel's row dealing (one tile per wave and round); CAP >= k + DEAL::kBlockRows, a power of two.
// multi_lists_round is called by every wave once per round, after the round's similarities exist:
//   sim4   D layout of the MFMA: lane (r16, g) holds question r16 against rows 4 g + 0..3 of the wave's tile.
template <class DEAL, int CAP, class LDS>
__device__ __forceinline__ void multi_lists_round(LDS& L, const f32x4& sim4, int64_t tile, int64_t n_tiles, int64_t n_rows, int n_q, int k,
                                                  bool first_or_last_round, int wave, int lane) {
    const int r16 = lane & 15, g = lane >> 4;
    if (tile < n_tiles) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = tile * kMTileRows + 4 * g + j;
            const uint64_t key = make_key(sim4[j], (uint32_t)row);
            if (r16 < n_q && row < n_rows && key > L.tau[r16]) {
                const int pos = atomicAdd(&L.cnt[r16], 1);
                L.keys[r16][pos] = key;
            }
        }
    }
    // Sort the lists down to k: at the end, whenever one could overflow in the next round, and once after the very
    // first round -- that sets the thresholds early, so that from the second round on only rows that beat the
    // current k-th best are appended at all.  The decision is taken by ONE wave between two barriers and read by
    // the others after the second one: it is workgroup-uniform by construction (no wave can append again before
    // every wave has read the flag, because the flag is reset only behind the third barrier).
    multi_barrier();                                          // every append of this round is visible
    if (wave == 0) {
        bool need = first_or_last_round;
        if (lane < kMQ) need |= L.cnt[lane] > CAP - DEAL::kBlockRows;
        need = __any(need);
        if (lane == 0) L.need = need ? 1 : 0;
    }
    multi_barrier();
    if (L.need) {
        constexpr int NL = kMQ / DEAL::kWaves;                // lists per wave: wave w owns questions w, w + kWaves, ...
        uint64_t* lists[NL];
        int n[NL], nmax = 0;
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            lists[q] = L.keys[wave + q * DEAL::kWaves];
            n[q] = L.cnt[wave + q * DEAL::kWaves];
            nmax = n[q] > nmax ? n[q] : nmax;
        }
        int n2 = 64;
        while (n2 < nmax) n2 <<= 1;
#pragma unroll
        for (int q = 0; q < NL; ++q)
            for (int t = n[q] + lane; t < n2; t += 64) lists[q][t] = 0ull;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        wave_bitonic_desc<NL>(lists, n2, lane);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const int qi = wave + q * DEAL::kWaves;
                L.cnt[qi] = n[q] < k ? n[q] : k;
                L.tau[qi] = n[q] >= k ? lists[q][k - 1] : 0ull;
            }
        }
        multi_barrier();                                      // new counts / thresholds visible before the next appends
    }
}
// this workgroup's best k per question (sorted, 0-padded) to out[question][workgroup][k]; a workgroup with no tile leaves zeros
template <class DEAL, class LDS>
__device__ __forceinline__ void multi_lists_flush(const LDS& L, int n_q, int k, uint64_t* __restrict__ out) {
    __syncthreads();
    for (int i = threadIdx.x; i < n_q * k; i += DEAL::kWaves * 64) {
        const int qi = i / k, t = i - qi * k;
        out[((size_t)qi * gridDim.x + blockIdx.x) * k + t] = t < L.cnt[qi] ? L.keys[qi][t] : 0ull;
    }
}

// ---- the per-event finish of the shadow routes -----------------------------------------------------------------------------------
// One workgroup per (event, question y).  The event's k-th largest s~ gives the threshold, the rows at or above it are re-scored on
// the fp32 store and the k best of those are the event's answer -- what segment_topk_kernel returns on the exact similarities.
// More candidates than the buffer holds (an event of near-identical rows): every row of the event is re-scored.  k <= 64.
//   sims    s~ of question y at sims + y * sims_stride; outputs are slot (y, event) of the query-major (Q, E, k) arrays.
//   stats   nullable: [0] += 1 when the whole event was re-scored, [1] += rows re-scored.
//   RESCORE the exact arithmetic of the route, which defines the bits of the answer:
//     kEps                         the proven bound of |s~ - s| on this route;
//     Lds                          its LDS block (left untouched by a re-scorer that needs none: the compiler drops it);
//     stage<THREADS>(lds, queries, y)   called by every thread before the first barrier of the kernel;
//     RESCORE(lds, queries, y)     constructed by every thread after the candidates are listed (its registers live from there);
//     score<THREADS>(rows, take, row_of, out)   out[c] = key of candidate c of `take`, its row inside the event being row_of(c),
//                                  rows = the event's first row in the store; called by every thread.
// Two shapes of the same code, as segment_topk_kernel has them: 4096 keys, and 1024 keys / 256 threads for small events.
template <int CHUNK, int THREADS, class RESCORE>
__global__ __launch_bounds__(THREADS) void segment_prefilter_kernel(const float* __restrict__ sims, int64_t sims_stride,
                                                                    const int64_t* __restrict__ seg_off, int k,
                                                                    const float* __restrict__ store, const float* __restrict__ queries,
                                                                    int64_t* __restrict__ idx_out, float* __restrict__ sim_out,
                                                                    int32_t* __restrict__ n_out, int32_t* __restrict__ stats) {
    __shared__ uint64_t s[CHUNK];
    __shared__ uint32_t cand[kCandCap];
    __shared__ typename RESCORE::Lds rescore_lds;
    __shared__ int n_cand;
    const int e = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const int64_t slot = (int64_t)y * gridDim.x + e;
    sims += (int64_t)y * sims_stride;
    const int64_t lo = seg_off[e], hi = seg_off[e + 1];
    const int64_t n = hi - lo;
    const int k_out = (int)(n < k ? (n > 0 ? n : 0) : k);
    idx_out += slot * k; sim_out += slot * k; n_out += slot;
    if (tid == 0) n_cand = 0;
    if (n <= 0) {                                                  // block-uniform
        write_hits(s, 0, k, idx_out, sim_out, n_out);
        return;
    }
    RESCORE::template stage<THREADS>(rescore_lds, queries, y);
    // ---- the k-th largest approximate key of the event ------------------------------------------------------------------------
    uint32_t thr = 0u;                                             // n <= k: every row is a candidate
    if (n > k) {
        fold_topk<CHUNK, THREADS, false>(s, n, k, [&](int64_t base, int have, int take) {
            for (int t = tid; t < take; t += THREADS) s[have + t] = make_key(sims[lo + base + t], (uint32_t)(base + t));
        });
        thr = threshold_below(key_order(s[k - 1]), RESCORE::kEps);
    }
    __syncthreads();
    // ---- candidates -----------------------------------------------------------------------------------------------------------
    for (int64_t r = tid; r < n; r += THREADS) {
        if (order_bits(sims[lo + r]) >= thr) {
            const int pos = atomicAdd(&n_cand, 1);
            if (pos < kCandCap) cand[pos] = (uint32_t)r;
        }
    }
    __syncthreads();
    const bool all_rows = n_cand > kCandCap;                       // block-uniform
    const int64_t m = all_rows ? n : (int64_t)n_cand;
    if (tid == 0 && stats) {                                       // a diagnostic: an int32 sum over all pairs and passes, it may wrap
        if (all_rows) atomicAdd(&stats[0], 1);
        atomicAdd(&stats[1], (int)m);
    }
    // ---- exact re-score, k best -----------------------------------------------------------------------------------------------
    const RESCORE rescore(rescore_lds, queries, y);
    fold_topk<CHUNK, THREADS, false>(s, m, k, [&](int64_t base, int have, int take) {
        rescore.template score<THREADS>(store + lo * 1024, take, [&](int c) { return all_rows ? base + c : (int64_t)cand[base + c]; }, s + have);
    });
    write_hits(s, k_out, k, idx_out, sim_out, n_out);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The questions of a batched call, kMQ per pass over the store: pass(p) launches the pass of questions p.q0 .. p.q0 + p.nq and
// returns its status; the first failure ends the call.  p.at(ptr, n) = where the part of question q0 starts in a per-question array
// of n elements each (nullptr stays nullptr).
struct QuestionPass {
    int q0, nq;
    template <class T>
    T* at(T* p, size_t per_question) const { return p ? p + (size_t)q0 * per_question : nullptr; }
};
template <class F>
int for_each_pass(int n_queries, F pass) {
    for (int q0 = 0; q0 < n_queries; q0 += kMQ) {
        const int rc = pass(QuestionPass{q0, n_queries - q0 < kMQ ? n_queries - q0 : kMQ});
        if (rc != HMM_OK) return rc;
    }
    return HMM_OK;
}

}  // namespace hmm
