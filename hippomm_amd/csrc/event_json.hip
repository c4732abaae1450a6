// The feature matrices of an event file as JSON text, written on the GPU: byte for byte what hmm_json_write_matrix_f64
// (event_json.cpp) writes for the same values at the same close_indent, i.e. json.dumps(m.tolist(), indent=2) of
// save_theta_event (hippomm/core/hippocampal_memory.py:331-335) -- without the matrix leaving the device as numbers.
//
// Every value owns one ITEM of the text: what stands in front of its digits (",\n" and the indentation; for the first value of a
// row also the row's "[" and, in front of that, the "," after the previous row or the matrix's own "["), its float.__repr__
// (event_json_core.h) and, behind the last value of a row, the row's "]" -- behind the last value of all also the matrix's.  Items
// are independent given their lengths, so the text is a prefix sum away:
//   1. json_length_kernel: one workgroup per HMM_JSON_VALUES_PER_GROUP values sums its item lengths into the workspace;
//   2. json_scan_kernel:   one workgroup turns those sums into 64-bit start offsets, HMM_JSON_SCAN_SUMS_PER_ROUND per round with a
//                          running carry, and writes the total to *written;
//   3. json_write_kernel:  the same workgroups form each repr again, scan the item lengths of 256 values at a time inside the
//                          workgroup, put the text together in LDS at the alignment it will have in memory and store it in whole
//                          dwords; the up to three bytes left over at the end of a round are carried into the next round's first
//                          dword, so that only a workgroup's first and last dword can be partial -- those are shared with the
//                          neighbouring workgroups and go out as single bytes.
// Three launches on the caller's stream, no allocation, no synchronisation, no scratch, no wait between workgroups of a launch.
// The powers of five are read from global memory (a __device__ array, indexed divergently by the lanes; L1/L2 hold its 10 KB).
#include "hmm_common.h"
#include "event_json_core.h"

namespace {

using namespace hmm;

constexpr int kThreads = 256;
constexpr int kRounds = HMM_JSON_VALUES_PER_GROUP / kThreads;
static_assert(HMM_JSON_VALUES_PER_GROUP % kThreads == 0, "a workgroup's values are whole rounds of one value per thread");
static_assert(HMM_JSON_REPR_BYTES == HMM_JSON_REPR_MAX, "the header states the core's longest repr");
static_assert(HMM_JSON_SCAN_SUMS_PER_ROUND == kThreads, "the scan takes one sum per thread and round");

const uint64_t h_pow5_inv[HMM_JSON_POW5_INV_COUNT][2] = {HMM_JSON_POW5_INV_ENTRIES};
const uint64_t h_pow5[HMM_JSON_POW5_COUNT][2] = {HMM_JSON_POW5_ENTRIES};
__device__ uint64_t d_pow5_inv[HMM_JSON_POW5_INV_COUNT][2] = {HMM_JSON_POW5_INV_ENTRIES};
__device__ uint64_t d_pow5[HMM_JSON_POW5_COUNT][2] = {HMM_JSON_POW5_ENTRIES};

// What surrounds the repr of value v = r * cols + c (see the head of this file).
struct Frame {
    uint32_t before, after;          // bytes in front of and behind the repr
    bool row_start, row_end, first, last, later_row;
};
__device__ __forceinline__ Frame frame_of(uint32_t v, uint32_t n_values, uint32_t cols, uint32_t ind) {
    const uint32_t r = v / cols, c = v - r * cols;
    Frame f;
    f.row_start = c == 0;
    f.row_end = c == cols - 1;
    f.first = v == 0;
    f.last = v == n_values - 1;
    f.later_row = f.row_start && r > 0;
    // row start: "[" or ",", "\n", ind + 2 spaces, "[", "\n", ind + 4 spaces;  else: ",", "\n", ind + 4 spaces
    f.before = f.row_start ? 2 * ind + 10 : ind + 6;
    // row end: "\n", ind + 2 spaces, "]";  matrix end: "\n", ind spaces, "]"
    f.after = (f.row_end ? ind + 4 : 0) + (f.last ? ind + 2 : 0);
    return f;
}
// the longest item there is (a 1 x 1 matrix has all of it): what a round of the write kernel stages per thread
__host__ __device__ constexpr uint32_t max_item_bytes(uint32_t ind) { return (2 * ind + 10) + HMM_JSON_REPR_MAX + (ind + 4) + (ind + 2); }

template <typename T>
__device__ __forceinline__ hmm_json::Decimal decimal_of(const T* m, uint32_t v) {
    return hmm_json::decompose((double)m[v], d_pow5_inv, d_pow5);       // fp32 is widened: what np.asarray(f32).tolist() hands to json
}

// Inclusive scan over the 64 lanes, then over the workgroup's 4 waves through `sums` (kThreads / 64 + 1 words of LDS): the exclusive
// prefix of `x` within the workgroup, and the workgroup's total.  One barrier inside; `sums` may be written again after the caller's next one.
__device__ __forceinline__ uint32_t group_exclusive_scan(uint32_t x, uint32_t* sums, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += up;
    }
    if (lane == 63) sums[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
        const uint32_t s = sums[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + incl - x;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void json_length_kernel(const T* __restrict__ m, uint32_t n_values, uint32_t cols, uint32_t ind,
                                                               uint64_t* __restrict__ group_sums) {
    __shared__ uint32_t sums[kThreads / 64];
    const uint32_t first = blockIdx.x * (uint32_t)HMM_JSON_VALUES_PER_GROUP;
    uint32_t bytes = 0;                                              // at most kRounds items of a few hundred bytes
    for (int round = 0; round < kRounds; ++round) {
        const uint32_t v = first + round * kThreads + threadIdx.x;   // n_values <= 2^31: no wrap
        if (v < n_values) {
            const Frame f = frame_of(v, n_values, cols, ind);
            bytes += f.before + (uint32_t)hmm_json::repr_length(decimal_of(m, v)) + f.after;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bytes += __shfl_xor(bytes, off, 64);
    if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6] = bytes;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0;
        for (int w = 0; w < kThreads / 64; ++w) all += sums[w];
        group_sums[blockIdx.x] = all;
    }
}

// group_sums[0 .. n_groups) -> their exclusive prefix sums in place; *written = the total.  One workgroup.
__global__ __launch_bounds__(kThreads) void json_scan_kernel(uint64_t* __restrict__ group_sums, uint32_t n_groups, uint64_t* __restrict__ written) {
    __shared__ uint64_t wave_sums[kThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_groups; base += HMM_JSON_SCAN_SUMS_PER_ROUND) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t x = i < n_groups ? group_sums[i] : 0;
        uint64_t incl = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)incl, off, 64), hi = __shfl_up((uint32_t)(incl >> 32), off, 64);
            if (lane >= (uint32_t)off) incl += ((uint64_t)hi << 32) | lo;
        }
        if (lane == 63) wave_sums[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kThreads / 64; ++w) {
            const uint64_t s = wave_sums[w];
            before += w < wave ? s : 0;
            all += s;
        }
        if (i < n_groups) group_sums[i] = carry + before + incl - x;
        carry += all;
        __syncthreads();                                             // wave_sums is written again in the next round
    }
    if (threadIdx.x == 0) *written = carry;
}

__device__ __forceinline__ void put_spaces(char* p, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) p[i] = ' ';
}

// Dynamic LDS: 8 words for the scan, then the stage of 4 + kThreads * max_item_bytes(ind) bytes (rounded up to a dword).
template <typename T>
__global__ __launch_bounds__(kThreads) void json_write_kernel(const T* __restrict__ m, uint32_t n_values, uint32_t cols, uint32_t ind,
                                                              const uint64_t* __restrict__ group_starts, char* __restrict__ out) {
    extern __shared__ uint32_t lds[];
    uint32_t* sums = lds;
    char* stage = reinterpret_cast<char*>(lds + 8);
    uint32_t* stage_words = lds + 8;
    const uint32_t tid = threadIdx.x;
    const uint32_t first = blockIdx.x * (uint32_t)HMM_JSON_VALUES_PER_GROUP;
    const uint32_t n_here = n_values - first < (uint32_t)HMM_JSON_VALUES_PER_GROUP ? n_values - first : (uint32_t)HMM_JSON_VALUES_PER_GROUP;
    const uint32_t rounds = (n_here + kThreads - 1) / kThreads;
    char* at = out + group_starts[blockIdx.x];                       // where this workgroup's text begins
    // stage[0] always stands for a dword-aligned address `base`; the text of a round begins at stage[lead], and stage[own .. lead)
    // are bytes of this workgroup carried over from the round before (own == lead in the first round: the bytes in front belong
    // to the previous workgroup)
    uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(at) & 3);
    uint32_t own = lead;
    char* base = at - lead;
    for (uint32_t round = 0; round < rounds; ++round) {
        const uint32_t v = first + round * kThreads + tid;
        const bool valid = v < n_values;
        hmm_json::Decimal d;
        Frame f;
        uint32_t item = 0;
        if (valid) {
            f = frame_of(v, n_values, cols, ind);
            d = decimal_of(m, v);
            item = f.before + (uint32_t)hmm_json::repr_length(d) + f.after;
        }
        uint32_t total;
        const uint32_t offset = group_exclusive_scan(item, sums, &total);
        if (valid) {
            char* p = stage + lead + offset;
            if (f.row_start) {
                *p++ = f.later_row ? ',' : '[';
                *p++ = '\n';
                put_spaces(p, ind + 2);
                p += ind + 2;
                *p++ = '[';
            } else {
                *p++ = ',';
            }
            *p++ = '\n';
            put_spaces(p, ind + 4);
            p += ind + 4;
            p += hmm_json::repr_emit(d, p);
            if (f.row_end) {
                *p++ = '\n';
                put_spaces(p, ind + 2);
                p += ind + 2;
                *p++ = ']';
            }
            if (f.last) {
                *p++ = '\n';
                put_spaces(p, ind);
                p += ind;
                *p++ = ']';
            }
        }
        __syncthreads();
        // flush stage[own, upto): everything in the last round, whole dwords otherwise
        const uint32_t end = lead + total;
        const bool last_round = round + 1 == rounds;
        const uint32_t upto = last_round ? end : (end & ~3u);
        if (upto > own) {
            const uint32_t head_end = ((own + 3) & ~3u) < upto ? ((own + 3) & ~3u) : upto;       // own .. head_end: bytes of a dword shared with the previous workgroup
            const uint32_t body_end = upto & ~3u;
            if (own + tid < head_end) base[own + tid] = stage[own + tid];
            for (uint32_t w = (head_end >> 2) + tid; w < (body_end >> 2); w += kThreads)
                reinterpret_cast<uint32_t*>(base)[w] = stage_words[w];
            if (body_end >= head_end && body_end + tid < upto) base[body_end + tid] = stage[body_end + tid];   // the workgroup's last, partial dword
        }
        if (!last_round) {
            // the bytes behind the last whole dword open the next round's first dword
            const uint32_t keep = end - upto;                        // < 4 when something was flushed; else nothing moved (upto == 0)
            char carried = 0;
            if (upto > 0 && tid < keep) carried = stage[upto + tid];
            __syncthreads();
            if (upto > 0) {
                if (tid < keep) stage[tid] = carried;
                base += upto;
                own = 0;
                lead = keep;
            } else {
                lead = end;                                          // fewer than four bytes so far: they stay where they are
            }
        }
    }
}

template <typename T>
int launch_all(const T* m, uint32_t n_values, uint32_t cols, uint32_t ind, char* out, uint64_t* written, uint64_t* ws, hipStream_t st) {
    const uint32_t groups = (n_values + HMM_JSON_VALUES_PER_GROUP - 1) / HMM_JSON_VALUES_PER_GROUP;
    const size_t lds_bytes = 8 * sizeof(uint32_t) + align_up(4 + (size_t)kThreads * max_item_bytes(ind), 4);
    json_length_kernel<T><<<groups, kThreads, 0, st>>>(m, n_values, cols, ind, ws);
    HMM_LAUNCH_CHECK();
    json_scan_kernel<<<1, kThreads, 0, st>>>(ws, groups, written);
    HMM_LAUNCH_CHECK();
    json_write_kernel<T><<<groups, kThreads, lds_bytes, st>>>(m, n_values, cols, ind, ws, out);
    HMM_LAUNCH_CHECK();
    return HMM_OK;
}

}  // namespace

extern "C" size_t hmm_json_write_matrix_device_workspace_bytes(size_t rows, size_t cols) {
    if (rows < 1 || cols < 1 || rows > HMM_JSON_MAX_VALUES / cols) return 0;
    return (rows * cols + HMM_JSON_VALUES_PER_GROUP - 1) / HMM_JSON_VALUES_PER_GROUP * sizeof(uint64_t);
}

extern "C" int hmm_json_write_matrix_device(const void* m_dev, int dtype, size_t rows, size_t cols, int close_indent, char* out_text_dev,
                                            size_t cap, uint64_t* written_dev, void* workspace_dev, size_t workspace_bytes,
                                            hmm_stream_t stream) {
    HMM_REQUIRE(m_dev && out_text_dev && written_dev && workspace_dev, HMM_E_INVALID, "json_write_matrix_device: null pointer");
    HMM_REQUIRE(dtype == HMM_JSON_DTYPE_F32 || dtype == HMM_JSON_DTYPE_F64, HMM_E_INVALID,
                "json_write_matrix_device: dtype must be %d (fp32) or %d (fp64), got %d", HMM_JSON_DTYPE_F32, HMM_JSON_DTYPE_F64, dtype);
    HMM_REQUIRE(rows >= 1 && cols >= 1, HMM_E_INVALID, "json_write_matrix_device: %zu x %zu values (at least 1 x 1)", rows, cols);
    HMM_REQUIRE(rows <= HMM_JSON_MAX_VALUES / cols, HMM_E_INVALID, "json_write_matrix_device: %zu x %zu values, at most %llu are written in one call",
                rows, cols, (unsigned long long)HMM_JSON_MAX_VALUES);
    HMM_REQUIRE(close_indent >= 0 && close_indent <= HMM_JSON_MAX_INDENT, HMM_E_INVALID,
                "json_write_matrix_device: close_indent %d outside 0 .. %d", close_indent, HMM_JSON_MAX_INDENT);
    HMM_REQUIRE(cap >= hmm_json_matrix_text_bound(rows, cols, close_indent), HMM_E_INVALID,
                "json_write_matrix_device: buffer of %zu bytes, need %zu", cap, hmm_json_matrix_text_bound(rows, cols, close_indent));
    HMM_REQUIRE(workspace_bytes >= hmm_json_write_matrix_device_workspace_bytes(rows, cols), HMM_E_INVALID,
                "json_write_matrix_device: workspace of %zu bytes, need %zu", workspace_bytes,
                hmm_json_write_matrix_device_workspace_bytes(rows, cols));
    const size_t elem = dtype == HMM_JSON_DTYPE_F64 ? 8 : 4;
    HMM_REQUIRE(reinterpret_cast<uintptr_t>(m_dev) % elem == 0 && reinterpret_cast<uintptr_t>(workspace_dev) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(written_dev) % 8 == 0,
                HMM_E_INVALID, "json_write_matrix_device: the matrix must be aligned to its element, workspace and written to 8 bytes");
    const uint32_t n_values = (uint32_t)(rows * cols);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t* ws = static_cast<uint64_t*>(workspace_dev);
    if (dtype == HMM_JSON_DTYPE_F64)
        return launch_all(static_cast<const double*>(m_dev), n_values, (uint32_t)cols, (uint32_t)close_indent, out_text_dev, written_dev, ws, st);
    return launch_all(static_cast<const float*>(m_dev), n_values, (uint32_t)cols, (uint32_t)close_indent, out_text_dev, written_dev, ws, st);
}

// The core of event_json_core.h on the host: n doubles -> their json.dumps characters, HMM_JSON_REPR_MAX bytes apart, and lengths.
extern "C" int hmm_json_float_repr(const double* values, size_t n, char* out_chars, int* out_lengths) {
    HMM_REQUIRE((values && out_chars && out_lengths) || n == 0, HMM_E_INVALID, "json_float_repr: null pointer");
    for (size_t i = 0; i < n; ++i)
        out_lengths[i] = hmm_json::float_repr(values[i], out_chars + i * HMM_JSON_REPR_MAX, h_pow5_inv, h_pow5);
    return HMM_OK;
}
