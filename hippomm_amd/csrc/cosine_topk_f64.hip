// feature_search in float64 for stores whose float64 source held fp32 values only (include/hippomm_hip.h, "float64-origin
// stores").  The resident rows stay fp32 -- narrowing such a source lost nothing -- and this route widens them in registers and
// accumulates in fp64, so the only roundings are those of the sums.  Opt-in; its own small pipeline beside the fp32 scans.  ONE host
// path: a call is passes of up to 16 queries, each a scan into query-major planes and a selection with the query as the grid's second
// dimension; the single-query entry points are batches of one (scan_flat_f64 / scan_segments_f64 behind every entry's own checks).
//
//   scan_sims_f64_kernel     one wave per row, two rows in flight per wave, the load pattern of scan_topk_kernel (lane l reads the
//                            float4 at columns 4 (64 j + l), j = 0..3: every load instruction of a wave covers 1 KiB contiguous).
//                            One double per row into an [N] workspace array.  4096 B per row, read once.  A pass of one query.
//   scan_sims_f64_multi_kernel  the same pass for 2 to 16 queries: the queries wait in LDS, a wave
//                            holds four rows widened in registers and reads each query fragment once per row block.  One double
//                            per (query, row) into query-major planes, plane q at sims + q N.  Bit for bit the doubles of
//                            scan_sims_f64_kernel for that query alone.
//   select_f64_kernel        top-k of a range of those doubles (or of candidate pairs) under the library's total order, by one
//                            workgroup: k rounds of a block-wide arg-max (k <= 64; a range of up to 16 pairs per thread is read once
//                            and kept in registers), or a bitonic sort of (key, index) pairs through 1024-pair LDS chunks (k <= 1024).  Per event: one workgroup per event.  Flat: G workgroups over
//                            contiguous slices, then one over the G k candidates -- exact selection under a total order, so the
//                            result does not depend on G.
//   bitonic_global_f64_*     flat calls with min(k, N) > 1024: a full sort of all (key, index) pairs.
//   rows_f64_are_f32_kernel  the eligibility check of a float64 source: how many values do not survive (double)(float)v, and the
//                            lowest flat offset of one.
//
// THE FIXED SUMMATION ORDER (a row's similarity bits depend on nothing else -- not on N, the grid, k or the entry point):
//   lane l owns columns 4 (64 j + l) + c, j = 0..3, c = 0..3.  Chain 0 takes j = 0 then j = 1, chain 1 takes j = 2 then j = 3, each in
//   the order c = 0, 1, 2, 3, every step one fma(x, a, chain) on exactly widened operands, starting from +0.0.  The lane's value is
//   chain 0 + chain 1.  The wave reduction is the butterfly v += v[lane ^ off] for off = 32, 16, 8, 4, 2, 1 (every lane ends with the
//   same bits).  D = sum x a and S = sum x x use this order; so does the query's own sum of squares when no norm is handed in.
//   sim = D / (sqrt(S) * A): norms multiplied first, then one division, as the reference has it; sqrt and / correctly rounded.
//
// Keys: order_bits64(sim), a monotone double -> uint64 map with NaN -> all ones and -0.0 == +0.0, paired with a 32-bit position.
// "Larger (key, position) pair" == "better; higher position first on ties; NaN first".  Key 0 belongs to no double: it pads.
// No kernel waits for another workgroup, allocates or synchronises; vector stores only; no scratch.
#include "hmm_common.h"
#include "cosine_topk_shared.h"

namespace hmm {

constexpr int kF64ArgmaxK = 64;          // up to here k rounds of arg-max; above, the LDS bitonic chunks
constexpr int kF64MaxK = 1024;           // the selection kernels' list length
constexpr int kF64Slice = 4096;          // rows per first-level workgroup of the flat call, at least
constexpr int kF64MaxGroups = 256;       // first-level workgroups of the flat call, at most (k <= 64)
constexpr int kF64MaxGroupsSort = 32;    // ... for 64 < k <= 1024, where the second level sorts G k pairs chunk by chunk
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

__device__ __forceinline__ uint64_t order_bits64(double s) {
    if (s != s) return ~0ull;
    s += 0.0;                                                   // -0.0 -> +0.0
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct Pair64 {
    uint64_t key;
    uint32_t pos;
};
__device__ __forceinline__ bool pair_less(const Pair64& a, const Pair64& b) { return a.key < b.key || (a.key == b.key && a.pos < b.pos); }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int off) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((uint64_t)hi << 32) | lo;
}

// ---- the similarity pass ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fma4_f64(double& d, double& s, const float4& x, const double (&a)[4]) {
    const double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;      // v_cvt_f64_f32: exact
    d = fma(x0, a[0], d); s = fma(x0, x0, s);
    d = fma(x1, a[1], d); s = fma(x1, x1, s);
    d = fma(x2, a[2], d); s = fma(x2, x2, s);
    d = fma(x3, a[3], d); s = fma(x3, x3, s);
}

// One row from its four loaded float4: (D, S) in the fixed order, reduced over the wave.
__device__ __forceinline__ void row_sums_f64(const float4 (&x)[4], const double (&a)[4][4], double& D, double& S) {
    double d0 = 0.0, s0 = 0.0, d1 = 0.0, s1 = 0.0;
    fma4_f64(d0, s0, x[0], a[0]);
    fma4_f64(d0, s0, x[1], a[1]);
    fma4_f64(d1, s1, x[2], a[2]);
    fma4_f64(d1, s1, x[3], a[3]);
    D = wave_sum(d0 + d1);
    S = wave_sum(s0 + s1);
}

// The norm of a query that no norm was handed in for: same lane ownership, chains and butterfly as a row's sums.
template <bool Q64>
__device__ __forceinline__ double query_norm_f64(const double (&a)[4][4]) {
    double c0 = 0.0, c1 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (j < 2) c0 = fma(a[j][c], a[j][c], c0);
            else       c1 = fma(a[j][c], a[j][c], c1);
        }
    }
    double A = sqrt(wave_sum(c0 + c1));
    if constexpr (!Q64) A = (double)(float)A;                   // an fp32 query's norm is an fp32 number (numpy's dtype rule)
    return A;
}

// Two rows (32 VGPRs of loads) in flight per wave, as scan_topk_kernel keeps them; the query costs 32 VGPRs as doubles.  The
// arithmetic per row is 2048 fp64 FMAs and 1024 conversions against 4096 bytes: far below the fp64 rate that would hide HBM.
template <bool Q64>
__global__ __launch_bounds__(256) void scan_sims_f64_kernel(const float4* __restrict__ store, int64_t n_rows, const void* __restrict__ query,
                                                            const double* __restrict__ query_norm, double* __restrict__ sims) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)gridDim.x * 4;

    double a[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (Q64) {
            const double* q = static_cast<const double*>(query) + 4 * (64 * j + lane);
#pragma unroll
            for (int c = 0; c < 4; ++c) a[j][c] = q[c];
        } else {
            const float4 q = static_cast<const float4*>(query)[64 * j + lane];
            a[j][0] = (double)q.x; a[j][1] = (double)q.y; a[j][2] = (double)q.z; a[j][3] = (double)q.w;
        }
    }
    const double A = query_norm != nullptr ? *query_norm : query_norm_f64<Q64>(a);

    const int64_t n_pairs = (n_rows + 1) >> 1;
    for (int64_t p = wave; p < n_pairs; p += n_waves) {
        const int64_t r = 2 * p;
        const bool two = (r + 1) < n_rows;                      // wave-uniform
        const float4* p0 = store + r * 256 + lane;
        const float4* p1 = p0 + (two ? 256 : 0);                // the last odd row is read twice, never a row past the end
        float4 x[4], y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = ld16<true>(p0 + j * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = ld16<true>(p1 + j * 64);
        __builtin_amdgcn_sched_barrier(0);                      // all eight loads in flight before the first use
        double D0, S0, D1, S1;
        row_sums_f64(x, a, D0, S0);
        row_sums_f64(y, a, D1, S1);
        const double v0 = D0 / (sqrt(S0) * A), v1 = D1 / (sqrt(S1) * A);
        if (lane == 0) {
            sims[r] = v0;
            if (two) sims[r + 1] = v1;
        }
    }
}

// ---- the similarity pass for a batch of queries -----------------------------------------------------------------------------------
// Up to kF64MultiQ queries per pass.  They wait in LDS in the dtype they came in (fp32: 4 KiB each, widened on read; fp64: 8 KiB),
// laid out so that lane l reads its fragment j with conflict-free 16-byte reads; behind 16 doubles that hold every query's A.
// A wave takes blocks of kF64MultiRows consecutive rows: 16 loads of 1 KiB each, all in flight before the first use, widened ONCE
// into 128 VGPRs, then each query's fragment is read once per block (the next one is fetched while this one is used).
//
// The sums keep THE FIXED SUMMATION ORDER per (row, query): the same two fma chains per lane, lane value = chain 0 + chain 1, and
// the butterfly's operand pairs.  The butterfly is PACKED: at off = 32 lanes 0..31 form v[l] + v[l ^ 32] of rows 0 and 1 only and
// lanes 32..63 of rows 2 and 3 (v_permlane32_swap hands each half what it needs), at off = 16 the lane's two rows become one, and
// off = 8, 4, 2, 1 run on that one value.  Lane l ends with the sum of row l >> 4.  Every sum formed is a butterfly sum of the same
// two operands (IEEE addition is commutative), every sum not formed would have been a bitwise copy of one that is.
// S and sqrt(S) are formed once per row block; D / (sqrt(S) * A) once per (row, query), by the 16 lanes that hold the row.
constexpr int kF64MultiQ = 16;
constexpr int kF64MultiRows = 4;
constexpr int kF64MultiThreads = 512;                          // 8 waves, two per SIMD: one workgroup per CU at up to 256 VGPRs
constexpr size_t kF64MultiNormBytes = kF64MultiQ * sizeof(double);
static size_t multi_lds_bytes(int nq, bool q64) { return kF64MultiNormBytes + (size_t)nq * HMM_FEATURE_DIM * (q64 ? 8 : 4); }

__device__ __forceinline__ double f64_of(uint32_t lo, uint32_t hi) { return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo)); }
__device__ __forceinline__ uint32_t lo_of(double v) { return (uint32_t)(uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ uint32_t hi_of(double v) { return (uint32_t)((uint64_t)__double_as_longlong(v) >> 32); }

// Lanes with bit 5 clear: a[l] + a[l ^ 32]; lanes with it set: b[l ^ 32] + b[l].  (swap: upper half of [0] <-> lower half of [1])
__device__ __forceinline__ double fold32_f64(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane32_swap(lo_of(a), lo_of(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(hi_of(a), hi_of(b), false, false);
    return f64_of(lo[0], hi[0]) + f64_of(lo[1], hi[1]);
}
// Lanes with bit 4 clear: a[l] + a[l ^ 16]; lanes with it set: b[l ^ 16] + b[l].  (swap: odd rows of [0] <-> even rows of [1])
__device__ __forceinline__ double fold16_f64(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane16_swap(lo_of(a), lo_of(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(hi_of(a), hi_of(b), false, false);
    return f64_of(lo[0], hi[0]) + f64_of(lo[1], hi[1]);
}
template <int J>
__device__ __forceinline__ double lane_xor_f64(double v) {
    return f64_of((uint32_t)lane_xor_b32<J>((int)lo_of(v)), (uint32_t)lane_xor_b32<J>((int)hi_of(v)));
}
// The four rows' lane values -> in lane l the wave sum of row l >> 4, with the butterfly's operand pairs.
__device__ __forceinline__ double wave_sum4_f64(const double (&v)[4]) {
    double u = fold16_f64(fold32_f64(v[0], v[2]), fold32_f64(v[1], v[3]));
    u += lane_xor_f64<8>(u);
    u += lane_xor_f64<4>(u);
    u += lane_xor_f64<2>(u);
    u += lane_xor_f64<1>(u);
    return u;
}

// A query fragment as it lies in LDS, and widened.  fp32: float4 [q][j][lane], the layout of the query itself.  fp64: double2
// [q][j][h][lane], h = 0 the columns c = 0, 1 and h = 1 the columns c = 2, 3: lane l's 16-byte reads are 16 bytes apart.
template <bool Q64> struct QueryFrag;
template <> struct QueryFrag<false> {
    float4 v[4];
    __device__ __forceinline__ void load(const unsigned char* lds, int q, int lane) {
        const float4* p = reinterpret_cast<const float4*>(lds) + q * 256 + lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[j * 64];
    }
    __device__ __forceinline__ void widen(double (&a)[4][4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j][0] = (double)v[j].x; a[j][1] = (double)v[j].y; a[j][2] = (double)v[j].z; a[j][3] = (double)v[j].w; }
    }
};
template <> struct QueryFrag<true> {
    double2 v[4][2];
    __device__ __forceinline__ void load(const unsigned char* lds, int q, int lane) {
        const double2* p = reinterpret_cast<const double2*>(lds) + q * 512 + lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j][0] = p[(2 * j) * 64]; v[j][1] = p[(2 * j + 1) * 64]; }
    }
    __device__ __forceinline__ void widen(double (&a)[4][4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j][0] = v[j][0].x; a[j][1] = v[j][0].y; a[j][2] = v[j][1].x; a[j][3] = v[j][1].y; }
    }
};

template <bool Q64>
__global__ __launch_bounds__(kF64MultiThreads) void scan_sims_f64_multi_kernel(const float4* __restrict__ store, int64_t n_rows,
                                                                              const void* __restrict__ queries,
                                                                              const double* __restrict__ query_norms, int nq,
                                                                              double* __restrict__ sims) {
    extern __shared__ __align__(16) unsigned char lds_f64_multi[];
    double* s_norm = reinterpret_cast<double*>(lds_f64_multi);
    unsigned char* s_query = lds_f64_multi + kF64MultiNormBytes;
    const int lane = threadIdx.x & 63, wave_in_block = threadIdx.x >> 6;

    // exactly nq queries are read: 16 bytes per thread and step, coalesced
    if constexpr (Q64) {
        const double2* src = static_cast<const double2*>(queries);
        double2* dst = reinterpret_cast<double2*>(s_query);
        for (int i = threadIdx.x; i < nq * 512; i += kF64MultiThreads) {
            const int q = i >> 9, e = i & 511;                  // e = 2 (64 j + l) + h
            dst[q * 512 + ((e >> 7) * 2 + (e & 1)) * 64 + ((e >> 1) & 63)] = src[i];
        }
    } else {
        const float4* src = static_cast<const float4*>(queries);
        float4* dst = reinterpret_cast<float4*>(s_query);
        for (int i = threadIdx.x; i < nq * 256; i += kF64MultiThreads) dst[i] = src[i];
    }
    __syncthreads();
    for (int q = wave_in_block; q < nq; q += kF64MultiThreads / 64) {
        double A;
        if (query_norms != nullptr) {
            A = query_norms[q];
        } else {
            QueryFrag<Q64> f;
            double a[4][4];
            f.load(s_query, q, lane);
            f.widen(a);
            A = query_norm_f64<Q64>(a);
        }
        if (lane == 0) s_norm[q] = A;
    }
    __syncthreads();

    const int64_t wave = (int64_t)blockIdx.x * (kF64MultiThreads / 64) + wave_in_block;
    const int64_t n_waves = (int64_t)gridDim.x * (kF64MultiThreads / 64);
    const int64_t n_blocks = (n_rows + kF64MultiRows - 1) / kF64MultiRows;
    const int mine = lane >> 4;                                 // the row of the block whose sums this lane ends up with
    for (int64_t b = wave; b < n_blocks; b += n_waves) {
        const int64_t r0 = b * kF64MultiRows;
        float4 x[kF64MultiRows][4];
#pragma unroll
        for (int i = 0; i < kF64MultiRows; ++i) {
            const int64_t r = (r0 + i) < n_rows ? (r0 + i) : (n_rows - 1);      // wave-uniform; the last row again, never a row past the end
            const float4* p = store + r * 256 + lane;
#pragma unroll
            for (int j = 0; j < 4; ++j) x[i][j] = ld16<true>(p + j * 64);
        }
        __builtin_amdgcn_sched_barrier(0);                      // all sixteen loads in flight before the first use
        double xd[kF64MultiRows][4][4], s[kF64MultiRows];
#pragma unroll
        for (int i = 0; i < kF64MultiRows; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {                       // v_cvt_f64_f32: exact
                xd[i][j][0] = (double)x[i][j].x; xd[i][j][1] = (double)x[i][j].y; xd[i][j][2] = (double)x[i][j].z; xd[i][j][3] = (double)x[i][j].w;
            }
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (j < 2) s0 = fma(xd[i][j][c], xd[i][j][c], s0);
                    else       s1 = fma(xd[i][j][c], xd[i][j][c], s1);
                }
            }
            s[i] = s0 + s1;
        }
        const double root = sqrt(wave_sum4_f64(s));             // of row r0 + mine
        const bool writes = (lane & 15) == 0 && (r0 + mine) < n_rows;
        double* out = sims + r0 + mine;

        QueryFrag<Q64> next;
        next.load(s_query, 0, lane);
        for (int q = 0; q < nq; ++q) {
            double a[4][4], d[kF64MultiRows];
            next.widen(a);
            next.load(s_query, (q + 1) < nq ? (q + 1) : q, lane);
#pragma unroll
            for (int i = 0; i < kF64MultiRows; ++i) {
                double d0 = 0.0, d1 = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (j < 2) d0 = fma(xd[i][j][c], a[j][c], d0);
                        else       d1 = fma(xd[i][j][c], a[j][c], d1);
                    }
                }
                d[i] = d0 + d1;
            }
            const double sim = wave_sum4_f64(d) / (root * s_norm[q]);
            if (writes) out[(int64_t)q * n_rows] = sim;
        }
    }
}

// ---- selection over the doubles -----------------------------------------------------------------------------------------------
// What a workgroup selects from: either doubles sims[lo .. lo + n) (position = i + pos_base) or candidate pairs (keys[i], pos[i]),
// i in [0, n), where key 0 marks padding.
struct SelectIn {
    const double* sims;
    const uint64_t* keys;
    const uint32_t* pos;
    int64_t lo;
    uint32_t pos_base;
    uint32_t n;
};
__device__ __forceinline__ Pair64 select_load(const SelectIn& in, uint32_t i) {
    if (in.keys != nullptr) return Pair64{in.keys[i], in.pos[i]};
    return Pair64{order_bits64(in.sims[in.lo + i]), in.pos_base + i};
}

// A range of up to kF64Held pairs per thread is read ONCE and kept in registers (thread t holds elements t + j blockDim.x): the k
// rounds then compare registers.  A longer range is read again from the L2 in every round.
constexpr int kF64Held = 16;

template <int J>
__device__ __forceinline__ void pair_max_step(Pair64& b) {          // all 64 lanes active: the VALU exchanges of hmm_common.h
    const uint32_t lo = (uint32_t)lane_xor_b32<J>((int)(uint32_t)b.key), hi = (uint32_t)lane_xor_b32<J>((int)(uint32_t)(b.key >> 32));
    const Pair64 o{((uint64_t)hi << 32) | lo, (uint32_t)lane_xor_b32<J>((int)b.pos)};
    if (pair_less(b, o)) b = o;
}

// The best (key, pos) pair of the workgroup's range strictly below `last`, key 0 when there is none.  Every thread returns it.
__device__ __forceinline__ Pair64 block_argmax_below(const SelectIn& in, bool held, const uint64_t (&hk)[kF64Held],
                                                     const uint32_t (&hp)[kF64Held], const Pair64& last,
                                                     Pair64* wave_best /* LDS [16] */) {
    Pair64 best{0ull, 0u};
    if (held) {
#pragma unroll
        for (int j = 0; j < kF64Held; ++j) {
            const Pair64 c{hk[j], hp[j]};
            if (c.key != 0ull && pair_less(c, last) && pair_less(best, c)) best = c;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < in.n; i += blockDim.x) {
            const Pair64 c = select_load(in, i);
            if (c.key != 0ull && pair_less(c, last) && pair_less(best, c)) best = c;
        }
    }
    pair_max_step<32>(best); pair_max_step<16>(best); pair_max_step<8>(best);
    pair_max_step<4>(best);  pair_max_step<2>(best);  pair_max_step<1>(best);
    __syncthreads();                                            // the previous round's readers are done with wave_best
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    best = wave_best[0];
    for (unsigned w = 1; w < (blockDim.x >> 6); ++w) {
        const Pair64 o = wave_best[w];
        if (pair_less(best, o)) best = o;
    }
    return best;
}

// keys / pos: LDS [2048], sorted descending by (key, pos) with blockDim.x threads.
__device__ __forceinline__ void lds_bitonic_desc_2048(uint64_t* keys, uint32_t* pos) {
    for (unsigned size = 2; size <= 2048; size <<= 1) {
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (unsigned t = threadIdx.x; t < 1024; t += blockDim.x) {
                const unsigned i = 2 * t - (t & (stride - 1)), j = i + stride;       // i has bit `stride` clear, j < 2048
                const Pair64 a{keys[i], pos[i]}, b{keys[j], pos[j]};
                const bool desc = (i & size) == 0;
                if (desc ? pair_less(a, b) : pair_less(b, a)) {
                    keys[i] = b.key; pos[i] = b.pos;
                    keys[j] = a.key; pos[j] = a.pos;
                }
            }
        }
    }
    __syncthreads();
}

// One workgroup per range.  seg_off != null: range e = rows [seg_off[e], seg_off[e + 1]) clamped into [0, n_rows], positions count
// from the range's first row (the per-event call).  seg_off == null and cand_keys == null: range g = slice g of ceil(n_rows /
// gridDim.x) rows, positions are rows of the store (the flat call's first level).  cand_keys != null: one range, the n_cand pairs.
// The arg-max rounds run with 256 or 1024 threads (the launch decides: up to 16 pairs per thread stay in registers).
// FINAL: idx_out[g k ..] int64 (-1 padded when pad), sim_out[g k ..] = sims[sim_base + position] (0 padded), counts_out[g] (nullable).
// Otherwise: out_keys / out_pos [g k ..], key 0 padded.  SORT: the LDS chunk path (k <= 1024, 1024 threads), else arg-max rounds.
template <bool SORT, bool FINAL>
__global__ __launch_bounds__(1024) void select_f64_kernel(const double* __restrict__ sims, int64_t n_rows,
                                                                       const int64_t* __restrict__ seg_off,
                                                                       const uint64_t* __restrict__ cand_keys,
                                                                       const uint32_t* __restrict__ cand_pos, uint32_t n_cand, int k,
                                                                       uint64_t* __restrict__ out_keys, uint32_t* __restrict__ out_pos,
                                                                       int64_t* __restrict__ idx_out, double* __restrict__ sim_out,
                                                                       int32_t* __restrict__ counts_out, int pad,
                                                                       int64_t plane_stride, int64_t cand_stride) {
    __shared__ Pair64 wave_best[16];
    __shared__ uint64_t s_keys[SORT ? 2048 : 1];
    __shared__ uint32_t s_pos[SORT ? 2048 : 1];
    const unsigned g = blockIdx.x;
    sims += (int64_t)blockIdx.y * plane_stride;                 // the query's plane and candidates (a batched call; else y = 0)
    if (cand_keys != nullptr) { cand_keys += (int64_t)blockIdx.y * cand_stride; cand_pos += (int64_t)blockIdx.y * cand_stride; }
    SelectIn in{sims, cand_keys, cand_pos, 0, 0u, 0u};
    int64_t sim_base = 0;
    if (cand_keys != nullptr) {
        in.n = n_cand;
    } else if (seg_off != nullptr) {
        int64_t lo = seg_off[g], hi = seg_off[g + 1];
        lo = lo < 0 ? 0 : (lo > n_rows ? n_rows : lo);
        hi = hi < lo ? lo : (hi > n_rows ? n_rows : hi);
        in.lo = lo;
        in.n = (uint32_t)(hi - lo);
        sim_base = lo;
    } else {
        const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
        int64_t lo = (int64_t)g * per, hi = lo + per;
        lo = lo > n_rows ? n_rows : lo;
        hi = hi > n_rows ? n_rows : hi;
        in.lo = lo;
        in.pos_base = (uint32_t)lo;
        in.n = (uint32_t)(hi - lo);
    }
    const int64_t range = (int64_t)blockIdx.y * gridDim.x + g, out0 = range * k;
    int found = 0;                                              // block-uniform

    auto emit = [&](int t, const Pair64& p) {                   // one thread writes slot t
        if constexpr (FINAL) {
            idx_out[out0 + t] = (int64_t)p.pos;
            sim_out[out0 + t] = sims[sim_base + p.pos];
        } else {
            out_keys[out0 + t] = p.key;
            out_pos[out0 + t] = p.pos;
        }
    };

    if constexpr (!SORT) {
        const bool held = in.n <= (uint32_t)kF64Held * blockDim.x;       // block-uniform
        uint64_t hk[kF64Held];
        uint32_t hp[kF64Held];
#pragma unroll
        for (int j = 0; j < kF64Held; ++j) {
            const uint32_t i = threadIdx.x + (uint32_t)j * blockDim.x;
            Pair64 c{0ull, kNoPos};
            if (held && i < in.n) c = select_load(in, i);
            hk[j] = c.key;
            hp[j] = c.pos;
        }
        Pair64 last{~0ull, kNoPos};                             // above every valid pair (positions stay below kNoPos)
        for (; found < k; ++found) {
            const Pair64 best = block_argmax_below(in, held, hk, hp, last, wave_best);
            if (best.key == 0ull) break;
            if (threadIdx.x == 0) emit(found, best);
            last = best;
        }
    } else {
        for (unsigned t = threadIdx.x; t < 1024; t += blockDim.x) { s_keys[t] = 0ull; s_pos[t] = kNoPos; }
        for (uint32_t c0 = 0; c0 < in.n; c0 += 1024) {
            for (unsigned t = threadIdx.x; t < 1024; t += blockDim.x) {
                Pair64 p{0ull, kNoPos};
                if (c0 + t < in.n) p = select_load(in, c0 + t);
                if (p.key == 0ull) p.pos = kNoPos;
                s_keys[1024 + t] = p.key;
                s_pos[1024 + t] = p.pos;
            }
            lds_bitonic_desc_2048(s_keys, s_pos);               // the best 1024 so far are the first 1024 again
        }
        __syncthreads();
        for (int t = threadIdx.x; t < k; t += blockDim.x)
            if (s_keys[t] != 0ull) emit(t, Pair64{s_keys[t], s_pos[t]});
        // the number of valid pairs among the first k: they are sorted, so it is the first padding slot
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_keys[mid] != 0ull) lo = mid + 1; else hi = mid;
        }
        found = lo;
    }
    // padding behind the valid slots
    if constexpr (FINAL) {
        if (pad)
            for (int t = found + threadIdx.x; t < k; t += blockDim.x) { idx_out[out0 + t] = -1; sim_out[out0 + t] = 0.0; }
        if (counts_out != nullptr && threadIdx.x == 0) counts_out[range] = found;
    } else {
        for (int t = found + threadIdx.x; t < k; t += blockDim.x) { out_keys[out0 + t] = 0ull; out_pos[out0 + t] = kNoPos; }
    }
}

// ---- min(k, N) > 1024 on the flat call: sort everything -----------------------------------------------------------------------
__global__ void keys_from_sims_f64_kernel(const double* __restrict__ sims, int64_t n, int64_t n_pad, uint64_t* __restrict__ keys,
                                          uint32_t* __restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    keys[i] = i < n ? order_bits64(sims[i]) : 0ull;
    pos[i] = i < n ? (uint32_t)i : kNoPos;
}
__global__ void bitonic_global_f64_step_kernel(uint64_t* __restrict__ keys, uint32_t* __restrict__ pos, int64_t half, int64_t stride,
                                               int64_t size) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half) return;
    const int64_t i = 2 * t - (t & (stride - 1)), j = i + stride;
    const Pair64 a{keys[i], pos[i]}, b{keys[j], pos[j]};
    const bool desc = (i & size) == 0;
    if (desc ? pair_less(a, b) : pair_less(b, a)) {
        keys[i] = b.key; pos[i] = b.pos;
        keys[j] = a.key; pos[j] = a.pos;
    }
}
__global__ void decode_sorted_f64_kernel(const uint32_t* __restrict__ pos, const double* __restrict__ sims, int k_out,
                                         int64_t* __restrict__ idx_out, double* __restrict__ sim_out, int32_t* __restrict__ n_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < k_out) {
        idx_out[t] = (int64_t)pos[t];
        sim_out[t] = sims[pos[t]];
    }
    if (t == 0 && n_out != nullptr) *n_out = k_out;
}

// ---- eligibility of a float64 source --------------------------------------------------------------------------------------------
// report[0] += values v with bits((double)(float)v) != bits(v); report[1] = min(report[1], lowest such flat offset).
__global__ void f64_report_init_kernel(uint64_t* __restrict__ report) {
    if (threadIdx.x == 0) { report[0] = 0ull; report[1] = ~0ull; }
}
__global__ __launch_bounds__(256) void rows_f64_are_f32_kernel(const double* __restrict__ src, int64_t n_values, uint64_t* __restrict__ report) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0ull, first = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_values; i += step) {
        const double v = __builtin_nontemporal_load(src + i);
        const double back = (double)(float)v;
        if (__double_as_longlong(back) != __double_as_longlong(v)) {
            ++bad;
            if (first == ~0ull) first = (unsigned long long)i;                // offsets rise along a thread's walk
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bad += shfl_xor_u64(bad, off);
        const unsigned long long o = shfl_xor_u64(first, off);
        first = o < first ? o : first;
    }
    if ((threadIdx.x & 63) == 0 && bad != 0ull) {
        atomicAdd(reinterpret_cast<unsigned long long*>(report), bad);
        atomicMin(reinterpret_cast<unsigned long long*>(report + 1), first);
    }
}

// ---- plans ----------------------------------------------------------------------------------------------------------------------
struct F64Plan {
    int k_eff;           // min(k, n)
    bool global_sort;    // k_eff > 1024
    int groups;          // first-level workgroups of the two-level selection
    int64_t n_pad;       // pairs of the global sort
    size_t keys_off, pos_off, total;      // the planes lie at offset 0
};
static int64_t next_pow2_i64(int64_t x) { int64_t p = 1; while (p < x) p <<= 1; return p; }

static int planes_of(int n_queries) { return n_queries < kF64MultiQ ? n_queries : kF64MultiQ; }      // of one pass: min(Q, 16)

// The flat call's workspace: `planes` planes of n doubles, then as many candidate lists (one pair buffer for the full sort, which
// takes plane after plane through it).
static F64Plan flat_plan(int64_t n, int planes, int k) {
    F64Plan p{};
    p.k_eff = (int)(k < n ? k : n);
    p.global_sort = p.k_eff > kF64MaxK;
    const int64_t by_slice = (n + kF64Slice - 1) / kF64Slice;
    const int cap = p.k_eff <= kF64ArgmaxK ? kF64MaxGroups : kF64MaxGroupsSort;
    p.groups = (int)(by_slice < 1 ? 1 : (by_slice > cap ? cap : by_slice));
    p.n_pad = p.global_sort ? next_pow2_i64(n) : 0;
    const size_t pairs = p.global_sort ? (size_t)p.n_pad : (size_t)planes * p.groups * p.k_eff;
    p.keys_off = align_up((size_t)planes * n * sizeof(double), 256);
    p.pos_off = p.keys_off + align_up(pairs * sizeof(uint64_t), 256);
    p.total = p.pos_off + align_up(pairs * sizeof(uint32_t), 256);
    return p;
}

// The per-event call's workspace: the planes alone (an empty store still gets a non-empty one).
static size_t segmented_workspace(int64_t n, int planes) { return align_up((size_t)planes * (size_t)(n > 0 ? n : 1) * sizeof(double), 256); }

// Threads of an arg-max workgroup over `n` pairs: 256 while they fit its registers, 1024 beyond.
static unsigned argmax_threads(int64_t n) { return n <= 256 * kF64Held ? 256u : 1024u; }

static unsigned scan_grid_f64(int64_t n) {
    // HBM is saturated by bandwidth x latency of bytes in flight; a wave keeps 8 KB in flight as scan_topk_kernel's does, so the
    // same ~384 workgroups are enough (cosine_topk.hip, g_scan_blocks) and more of them stream slower.
    const int64_t blocks = ((n + 1) / 2 + 3) / 4;
    const int64_t cap = kNumCU * 3 / 2;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

static int check_common(const char* what, const float* store, int64_t n_rows, int dim, const void* query, int query_dtype,
                        const double* query_norm, int k) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "%s: dim must be %d, got %d", what, HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(query_dtype == 0 || query_dtype == 1, HMM_E_INVALID, "%s: query_dtype must be 0 (fp32) or 1 (fp64), got %d", what,
                query_dtype);
    HMM_REQUIRE(n_rows >= 0 && n_rows < (int64_t)0xFFFFFFFFll, HMM_E_INVALID, "%s: n_rows out of range", what);
    HMM_REQUIRE(k >= 1, HMM_E_INVALID, "%s: k must be >= 1", what);
    HMM_REQUIRE(query != nullptr, HMM_E_INVALID, "%s: null query", what);
    HMM_REQUIRE(n_rows == 0 || store != nullptr, HMM_E_INVALID, "%s: null store", what);
    HMM_REQUIRE(((uintptr_t)store & 15) == 0 && ((uintptr_t)query & 15) == 0 && ((uintptr_t)query_norm & 7) == 0, HMM_E_INVALID,
                "%s: store / query must be 16-byte aligned, query_norm 8-byte aligned", what);
    return HMM_OK;
}

// One pass of the scan: nq <= kF64MultiQ queries into nq planes of n doubles.  A pass of one query is the single-query kernel.
static int launch_scan_f64_multi(const float* store, int64_t n, const void* queries, int query_dtype, const double* query_norms, int nq,
                                 double* sims, hipStream_t st) {
    const float4* s4 = reinterpret_cast<const float4*>(store);
    if (nq == 1) {
        if (query_dtype == 1) scan_sims_f64_kernel<true><<<scan_grid_f64(n), 256, 0, st>>>(s4, n, queries, query_norms, sims);
        else                  scan_sims_f64_kernel<false><<<scan_grid_f64(n), 256, 0, st>>>(s4, n, queries, query_norms, sims);
        return HMM_OK;
    }
    const int64_t blocks = ((n + kF64MultiRows - 1) / kF64MultiRows + kF64MultiThreads / 64 - 1) / (kF64MultiThreads / 64);
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : (blocks > kNumCU ? kNumCU : blocks));     // one workgroup per CU: registers and LDS
    const size_t lds = multi_lds_bytes(nq, query_dtype == 1);
    if (query_dtype == 1) {
        HMM_ENSURE_DYN_LDS(scan_sims_f64_multi_kernel<true>, (int)multi_lds_bytes(kF64MultiQ, true));
        scan_sims_f64_multi_kernel<true><<<grid, kF64MultiThreads, lds, st>>>(s4, n, queries, query_norms, nq, sims);
    } else {
        HMM_ENSURE_DYN_LDS(scan_sims_f64_multi_kernel<false>, (int)multi_lds_bytes(kF64MultiQ, false));
        scan_sims_f64_multi_kernel<false><<<grid, kF64MultiThreads, lds, st>>>(s4, n, queries, query_norms, nq, sims);
    }
    return HMM_OK;
}

// ---- selection launches -----------------------------------------------------------------------------------------------------------
// One select_f64_kernel launch: what its workgroups select from and where they write, built in one of three named ways;
// launch_select unpacks it into the kernel's arguments.  The kernel multiplies blockIdx.y by a plane stride and a candidate stride:
// they are n_rows and n_cand, the distances between two queries' planes and candidate lists.  A call with one query passes the same
// values as a batch -- its grid has y == 1, so they are multiplied by blockIdx.y == 0.
struct SelectLaunch {
    const double* sims; int64_t n_rows; int k;                               // the planes: plane y at sims + y n_rows
    const int64_t* seg_off;                                                  // events()
    const uint64_t* cand_keys; const uint32_t* cand_pos; uint32_t n_cand;    // candidates(): list y at cand_keys + y n_cand
    uint64_t* out_keys; uint32_t* out_pos;                                   // !FINAL: candidate lists, key 0 padded
    int64_t* idx_out; double* sim_out; int32_t* counts_out; int pad;         // FINAL: the hits, -1 / 0 padded to k when pad

    // range g = slice g of ceil(n / gridDim.x) rows of the plane -> its k candidates (the flat call's first level)
    static SelectLaunch slices(const double* sims, int64_t n, int k, uint64_t* out_keys, uint32_t* out_pos) {
        SelectLaunch s{}; s.sims = sims; s.n_rows = n; s.k = k; s.out_keys = out_keys; s.out_pos = out_pos; return s;
    }
    // range e = the rows of event e of the offset table -> its hits, padded (the per-event call)
    static SelectLaunch events(const double* sims, int64_t n, int k, const int64_t* seg_off, int64_t* idx, double* sim, int32_t* counts) {
        SelectLaunch s = slices(sims, n, k, nullptr, nullptr);
        s.seg_off = seg_off; s.idx_out = idx; s.sim_out = sim; s.counts_out = counts; s.pad = 1;
        return s;
    }
    // one range: the query's n_cand candidate pairs -> its hits (the flat call's second level)
    static SelectLaunch candidates(const double* sims, int64_t n, int k, const uint64_t* keys, const uint32_t* pos, uint32_t n_cand,
                                   int64_t* idx, double* sim, int32_t* counts) {
        SelectLaunch s = events(sims, n, k, nullptr, idx, sim, counts);
        s.cand_keys = keys; s.cand_pos = pos; s.n_cand = n_cand; s.pad = 0;
        return s;
    }
};

template <bool SORT, bool FINAL>
static void launch_select(dim3 grid, unsigned threads, hipStream_t st, const SelectLaunch& s) {
    select_f64_kernel<SORT, FINAL><<<grid, threads, 0, st>>>(s.sims, s.n_rows, s.seg_off, s.cand_keys, s.cand_pos, s.n_cand, s.k, s.out_keys,
                                                             s.out_pos, s.idx_out, s.sim_out, s.counts_out, s.pad, s.n_rows, (int64_t)s.n_cand);
}

// min(k, n) > 1024: a full sort of one plane's (key, index) pairs through the pair buffer.
static void sort_plane_f64(const double* plane, int64_t n, const F64Plan& p, uint64_t* keys, uint32_t* pos, int64_t* idx_out,
                           double* sim_out, int32_t* n_out, hipStream_t st) {
    const int64_t half = p.n_pad / 2;
    keys_from_sims_f64_kernel<<<(unsigned)((p.n_pad + 255) / 256), 256, 0, st>>>(plane, n, p.n_pad, keys, pos);
    for (int64_t size = 2; size <= p.n_pad; size <<= 1)
        for (int64_t stride = size >> 1; stride > 0; stride >>= 1)
            bitonic_global_f64_step_kernel<<<(unsigned)((half + 255) / 256), 256, 0, st>>>(keys, pos, half, stride, size);
    decode_sorted_f64_kernel<<<(p.k_eff + 255) / 256, 256, 0, st>>>(pos, plane, p.k_eff, idx_out, sim_out, n_out);
}

// The flat selection for nq planes of n doubles into rows q of (nq, k_eff) outputs: two levels with the query as the second grid
// dimension, or plane after plane through the full sort.
static void select_flat_f64(const double* sims, int64_t n, const F64Plan& p, int nq, uint64_t* keys, uint32_t* pos, int64_t* idx_out,
                            double* sim_out, int32_t* n_out, hipStream_t st) {
    const int64_t per = (n + p.groups - 1) / p.groups, cand = (int64_t)p.groups * p.k_eff;
    const dim3 first(p.groups, nq), second(1, nq);
    const SelectLaunch level1 = SelectLaunch::slices(sims, n, p.k_eff, keys, pos);
    const SelectLaunch level2 = SelectLaunch::candidates(sims, n, p.k_eff, keys, pos, (uint32_t)cand, idx_out, sim_out, n_out);
    if (p.global_sort) {
        for (int q = 0; q < nq; ++q)
            sort_plane_f64(sims + (int64_t)q * n, n, p, keys, pos, idx_out + (int64_t)q * p.k_eff, sim_out + (int64_t)q * p.k_eff,
                           n_out ? n_out + q : nullptr, st);
    } else if (p.k_eff <= kF64ArgmaxK) {
        launch_select<false, false>(first, argmax_threads(per), st, level1);
        launch_select<false, true>(second, argmax_threads(cand), st, level2);
    } else {
        launch_select<true, false>(first, 1024, st, level1);
        launch_select<true, true>(second, 1024, st, level2);
    }
}

// The per-event selection for nq planes into (nq, E, k) outputs: one workgroup per (query, event).
static void select_segments_f64(const double* sims, int64_t n, const int64_t* seg_off, int n_segments, int k, int nq, int64_t* idx_out,
                                double* sim_out, int32_t* n_out, hipStream_t st) {
    const dim3 grid(n_segments, nq);
    const SelectLaunch events = SelectLaunch::events(sims, n, k, seg_off, idx_out, sim_out, n_out);
    if (k <= kF64ArgmaxK) launch_select<false, true>(grid, 256, st, events);
    else                  launch_select<true, true>(grid, 1024, st, events);
}

// ---- the two cores: everything behind an entry point's own argument checks ---------------------------------------------------------
// A call of Q queries is ceil(Q / 16) passes that follow each other on the stream and share the workspace; a single query is a batch
// of one (launch_scan_f64_multi gives it scan_sims_f64_kernel).
static int scan_flat_f64(const float* store, int64_t n, const void* queries, int query_dtype, const double* query_norms, int n_queries,
                         const F64Plan& p, int64_t* idx_out, double* sim_out, int32_t* n_out, void* workspace, hipStream_t st) {
    double* sims = static_cast<double*>(workspace);
    uint64_t* keys = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + p.keys_off);
    uint32_t* pos = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + p.pos_off);
    const size_t q_bytes = (size_t)HMM_FEATURE_DIM * (query_dtype == 1 ? 8 : 4);
    for (int q0 = 0; q0 < n_queries; q0 += kF64MultiQ) {
        const int nq = planes_of(n_queries - q0);
        if (int rc = launch_scan_f64_multi(store, n, static_cast<const char*>(queries) + q0 * q_bytes, query_dtype,
                                           query_norms ? query_norms + q0 : nullptr, nq, sims, st); rc != HMM_OK) return rc;
        HMM_LAUNCH_CHECK();
        select_flat_f64(sims, n, p, nq, keys, pos, idx_out + (int64_t)q0 * p.k_eff, sim_out + (int64_t)q0 * p.k_eff,
                        n_out ? n_out + q0 : nullptr, st);
        HMM_LAUNCH_CHECK();
    }
    return HMM_OK;
}

// The per-event form.  Without rows no scan is launched and every event gets its padding.
static int scan_segments_f64(const float* store, int64_t n, const void* queries, int query_dtype, const double* query_norms,
                             int n_queries, const int64_t* seg_off, int n_segments, int k, int64_t* idx_out, double* sim_out,
                             int32_t* n_out, void* workspace, hipStream_t st) {
    double* sims = static_cast<double*>(workspace);
    const size_t q_bytes = (size_t)HMM_FEATURE_DIM * (query_dtype == 1 ? 8 : 4);
    const int64_t cells = (int64_t)n_segments * k;
    for (int q0 = 0; q0 < n_queries; q0 += kF64MultiQ) {
        const int nq = planes_of(n_queries - q0);
        if (n > 0) {
            if (int rc = launch_scan_f64_multi(store, n, static_cast<const char*>(queries) + q0 * q_bytes, query_dtype,
                                               query_norms ? query_norms + q0 : nullptr, nq, sims, st); rc != HMM_OK) return rc;
            HMM_LAUNCH_CHECK();
        }
        select_segments_f64(sims, n, seg_off, n_segments, k, nq, idx_out + q0 * cells, sim_out + q0 * cells,
                            n_out + (int64_t)q0 * n_segments, st);
        HMM_LAUNCH_CHECK();
    }
    return HMM_OK;
}

static int check_multi(const char* what, const float* store, int64_t n_rows, int dim, const void* queries, int query_dtype,
                       const double* query_norms, int n_queries, int k, const int64_t* idx_out, const double* sim_out,
                       const int32_t* n_out, const void* workspace) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "%s: dim must be %d, got %d", what, HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(query_dtype == 0 || query_dtype == 1, HMM_E_INVALID, "%s: query_dtype must be 0 (fp32) or 1 (fp64), got %d", what,
                query_dtype);
    HMM_REQUIRE(n_queries >= 1, HMM_E_INVALID, "%s: n_queries must be >= 1", what);
    HMM_REQUIRE(n_rows >= 0 && n_rows < (int64_t)0xFFFFFFFFll, HMM_E_INVALID, "%s: n_rows out of range", what);
    HMM_REQUIRE(k >= 1, HMM_E_INVALID, "%s: k must be >= 1", what);
    HMM_REQUIRE(queries != nullptr && idx_out != nullptr && sim_out != nullptr && workspace != nullptr &&
                    (n_rows == 0 || store != nullptr), HMM_E_INVALID, "%s: null pointer", what);
    HMM_REQUIRE(((uintptr_t)store & 15) == 0 && ((uintptr_t)queries & 15) == 0 && ((uintptr_t)workspace & 15) == 0, HMM_E_INVALID,
                "%s: store, queries and workspace must be 16-byte aligned", what);
    HMM_REQUIRE(((uintptr_t)query_norms & 7) == 0 && ((uintptr_t)idx_out & 7) == 0 && ((uintptr_t)sim_out & 7) == 0 &&
                    ((uintptr_t)n_out & 3) == 0, HMM_E_INVALID,
                "%s: query_norms, idx_out and sim_out must be 8-byte aligned, n_out 4-byte aligned", what);
    return HMM_OK;
}

}  // namespace hmm

using namespace hmm;

extern "C" size_t hmm_cosine_topk_f64_workspace_bytes(int64_t n_rows, int k) {
    if (n_rows < 1 || n_rows >= (int64_t)0xFFFFFFFFll || k < 1) return 0;
    return flat_plan(n_rows, 1, k).total;
}

extern "C" int hmm_cosine_topk_f64(const float* store_dev, int64_t n_rows, int dim, const void* query_dev, int query_dtype,
                                   const double* query_norm_dev, int k, int64_t* idx_out_dev, double* sim_out_dev, int32_t* n_out_dev,
                                   void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    HMM_REQUIRE(idx_out_dev && sim_out_dev, HMM_E_INVALID, "cosine_topk_f64: null output pointer");
    int rc = check_common("cosine_topk_f64", store_dev, n_rows, dim, query_dev, query_dtype, query_norm_dev, k);
    if (rc != HMM_OK) return rc;
    HMM_REQUIRE(n_rows >= 1, HMM_E_INVALID, "cosine_topk_f64: n_rows must be >= 1");
    HMM_REQUIRE(workspace_dev != nullptr && ((uintptr_t)workspace_dev & 15) == 0, HMM_E_INVALID,
                "cosine_topk_f64: workspace must be given and 16-byte aligned");
    HMM_REQUIRE(((uintptr_t)idx_out_dev & 7) == 0 && ((uintptr_t)sim_out_dev & 7) == 0 && ((uintptr_t)n_out_dev & 3) == 0, HMM_E_INVALID,
                "cosine_topk_f64: outputs must be aligned to their element size");
    const F64Plan p = flat_plan(n_rows, 1, k);
    HMM_REQUIRE(workspace_bytes >= p.total, HMM_E_WORKSPACE, "cosine_topk_f64: workspace too small (%zu < %zu)", workspace_bytes, p.total);
    return scan_flat_f64(store_dev, n_rows, query_dev, query_dtype, query_norm_dev, 1, p, idx_out_dev, sim_out_dev, n_out_dev,
                         workspace_dev, static_cast<hipStream_t>(stream));
}

extern "C" size_t hmm_cosine_topk_segmented_f64_workspace_bytes(int64_t n_rows, int n_segments, int k) {
    if (n_rows < 0 || n_rows >= (int64_t)0xFFFFFFFFll || n_segments < 1 || k < 1) return 0;
    return segmented_workspace(n_rows, 1);
}

extern "C" int hmm_cosine_topk_segmented_f64(const float* store_dev, int64_t n_rows, int dim, const void* query_dev, int query_dtype,
                                             const double* query_norm_dev, const int64_t* seg_offsets_dev, int n_segments, int k,
                                             int64_t* idx_out_dev, double* sim_out_dev, int32_t* n_out_dev, void* workspace_dev,
                                             size_t workspace_bytes, hmm_stream_t stream) {
    int rc = check_common("cosine_topk_segmented_f64", store_dev, n_rows, dim, query_dev, query_dtype, query_norm_dev, k);
    if (rc != HMM_OK) return rc;
    HMM_REQUIRE(n_segments >= 1 && k <= kF64MaxK, HMM_E_INVALID, "cosine_topk_segmented_f64: need n_segments >= 1 and 1 <= k <= %d",
                kF64MaxK);
    HMM_REQUIRE(seg_offsets_dev && idx_out_dev && sim_out_dev && n_out_dev && workspace_dev, HMM_E_INVALID,
                "cosine_topk_segmented_f64: null pointer");
    HMM_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, HMM_E_INVALID, "cosine_topk_segmented_f64: workspace must be 16-byte aligned");
    HMM_REQUIRE(((uintptr_t)seg_offsets_dev & 7) == 0 && ((uintptr_t)idx_out_dev & 7) == 0 && ((uintptr_t)sim_out_dev & 7) == 0 &&
                    ((uintptr_t)n_out_dev & 3) == 0, HMM_E_INVALID,
                "cosine_topk_segmented_f64: offsets / outputs must be aligned to their element size");
    HMM_REQUIRE(workspace_bytes >= hmm_cosine_topk_segmented_f64_workspace_bytes(n_rows, n_segments, k), HMM_E_WORKSPACE,
                "cosine_topk_segmented_f64: workspace too small");
    return scan_segments_f64(store_dev, n_rows, query_dev, query_dtype, query_norm_dev, 1, seg_offsets_dev, n_segments, k, idx_out_dev,
                             sim_out_dev, n_out_dev, workspace_dev, static_cast<hipStream_t>(stream));
}

extern "C" int hmm_rows_f64_are_f32(const double* src_dev, int64_t n_rows, int dim, int64_t* report_dev, hmm_stream_t stream) {
    HMM_REQUIRE(dim == HMM_FEATURE_DIM, HMM_E_INVALID, "rows_f64_are_f32: dim must be %d, got %d", HMM_FEATURE_DIM, dim);
    HMM_REQUIRE(n_rows >= 0 && n_rows < (int64_t)0xFFFFFFFFll, HMM_E_INVALID, "rows_f64_are_f32: n_rows out of range");
    HMM_REQUIRE(report_dev != nullptr && ((uintptr_t)report_dev & 7) == 0, HMM_E_INVALID,
                "rows_f64_are_f32: report must be given and 8-byte aligned");
    HMM_REQUIRE(n_rows == 0 || (src_dev != nullptr && ((uintptr_t)src_dev & 7) == 0), HMM_E_INVALID,
                "rows_f64_are_f32: source must be given and 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t* report = reinterpret_cast<uint64_t*>(report_dev);
    f64_report_init_kernel<<<1, 64, 0, st>>>(report);
    HMM_LAUNCH_CHECK();
    if (n_rows > 0) {
        const int64_t n_values = n_rows * HMM_FEATURE_DIM;
        const int64_t blocks = (n_values + 256 * 16 - 1) / (256 * 16);
        rows_f64_are_f32_kernel<<<(unsigned)(blocks > kScanBlocks ? kScanBlocks : blocks), 256, 0, st>>>(src_dev, n_values, report);
        HMM_LAUNCH_CHECK();
    }
    return HMM_OK;
}

extern "C" size_t hmm_cosine_topk_multi_f64_workspace_bytes(int64_t n_rows, int n_queries, int k) {
    if (n_rows < 1 || n_rows >= (int64_t)0xFFFFFFFFll || n_queries < 1 || k < 1) return 0;
    return flat_plan(n_rows, planes_of(n_queries), k).total;
}

extern "C" int hmm_cosine_topk_multi_f64(const float* store_dev, int64_t n_rows, int dim, const void* queries_dev, int query_dtype,
                                         const double* query_norms_dev, int n_queries, int k, int64_t* idx_out_dev, double* sim_out_dev,
                                         int32_t* n_out_dev, void* workspace_dev, size_t workspace_bytes, hmm_stream_t stream) {
    const char* what = "cosine_topk_multi_f64";
    int rc = check_multi(what, store_dev, n_rows, dim, queries_dev, query_dtype, query_norms_dev, n_queries, k, idx_out_dev, sim_out_dev,
                         n_out_dev, workspace_dev);
    if (rc != HMM_OK) return rc;
    HMM_REQUIRE(n_rows >= 1, HMM_E_INVALID, "%s: n_rows must be >= 1", what);
    const F64Plan p = flat_plan(n_rows, planes_of(n_queries), k);
    HMM_REQUIRE(workspace_bytes >= p.total, HMM_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, p.total);
    return scan_flat_f64(store_dev, n_rows, queries_dev, query_dtype, query_norms_dev, n_queries, p, idx_out_dev, sim_out_dev, n_out_dev,
                         workspace_dev, static_cast<hipStream_t>(stream));
}

extern "C" size_t hmm_cosine_topk_segmented_multi_f64_workspace_bytes(int64_t n_rows, int n_segments, int n_queries, int k) {
    if (n_rows < 0 || n_rows >= (int64_t)0xFFFFFFFFll || n_segments < 1 || n_queries < 1 || k < 1) return 0;
    return segmented_workspace(n_rows, planes_of(n_queries));
}

extern "C" int hmm_cosine_topk_segmented_multi_f64(const float* store_dev, int64_t n_rows, int dim, const void* queries_dev,
                                                   int query_dtype, const double* query_norms_dev, int n_queries,
                                                   const int64_t* seg_offsets_dev, int n_segments, int k, int64_t* idx_out_dev,
                                                   double* sim_out_dev, int32_t* n_out_dev, void* workspace_dev, size_t workspace_bytes,
                                                   hmm_stream_t stream) {
    const char* what = "cosine_topk_segmented_multi_f64";
    int rc = check_multi(what, store_dev, n_rows, dim, queries_dev, query_dtype, query_norms_dev, n_queries, k, idx_out_dev, sim_out_dev,
                         n_out_dev, workspace_dev);
    if (rc != HMM_OK) return rc;
    HMM_REQUIRE(n_segments >= 1 && k <= kF64MaxK, HMM_E_INVALID, "%s: need n_segments >= 1 and 1 <= k <= %d", what, kF64MaxK);
    HMM_REQUIRE(seg_offsets_dev != nullptr && n_out_dev != nullptr, HMM_E_INVALID, "%s: null pointer", what);
    HMM_REQUIRE(((uintptr_t)seg_offsets_dev & 7) == 0, HMM_E_INVALID, "%s: seg_offsets must be 8-byte aligned", what);
    HMM_REQUIRE(workspace_bytes >= hmm_cosine_topk_segmented_multi_f64_workspace_bytes(n_rows, n_segments, n_queries, k), HMM_E_WORKSPACE,
                "%s: workspace too small", what);
    return scan_segments_f64(store_dev, n_rows, queries_dev, query_dtype, query_norms_dev, n_queries, seg_offsets_dev, n_segments, k,
                             idx_out_dev, sim_out_dev, n_out_dev, workspace_dev, static_cast<hipStream_t>(stream));
}
